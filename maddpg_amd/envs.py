"""Scenario metadata for the device MPE environments.

Mirrors what ``experiments/train.py:48-61`` obtains from MPE's
``scenarios.load(name).Scenario().make_world()``: the number of policy agents
(``env.n``), per-agent observation widths (``env.observation_space[i].shape``,
``train.py:83``) and ``Discrete(5)`` action spaces (``train.py:69,73``).
The physics itself runs in ``k_rollout`` (maddpg_amd/csrc/mdp_kernels.hip).
"""
from dataclasses import dataclass, field
from typing import List

import numpy as np

ACT_DIM = 5


class Discrete:
    """Minimal stand-in for ``gym.spaces.Discrete`` (gym is not installed)."""

    def __init__(self, n):
        self.n = int(n)

    def __repr__(self):
        return f"Discrete({self.n})"


class Box:
    """Minimal stand-in for ``gym.spaces.Box`` with a 1-D shape (unbounded floats):
    recognised by having a ``shape`` and no ``n``"""

    def __init__(self, d):
        self.shape = (int(d),)

    def __repr__(self):
        return f"Box({self.shape[0]},)"


@dataclass
class ScenarioSpec:
    name: str
    n_agents: int
    num_adversaries: int
    obs_dims: List[int] = field(default_factory=list)
    act_dims: List[int] = field(default_factory=list)   # Discrete(A_i) per agent; empty: Discrete(5) each
    act_kinds: List[str] = field(default_factory=list)  # "discrete" / "box" per agent; empty: discrete each

    def __post_init__(self):
        if not self.act_dims:
            self.act_dims = [ACT_DIM] * self.n_agents
        if not self.act_kinds:
            self.act_kinds = ["discrete"] * self.n_agents

    @property
    def action_space(self):
        return [Box(a) if k == "box" else Discrete(a) for k, a in zip(self.act_kinds, self.act_dims)]

    def continuous(self):
        """the same scenario with continuous actions (environment.py's
        discrete_action_space = False): every agent that moves and does not
        speak gets a Box(2) space, its action the force itself; the speaker of
        simple_speaker_listener keeps its Discrete(3) words.  (This mirrors what
        the library decides from its own scenario table -- EnvDesc::movable and
        env_silent in csrc/mdp_topo.h -- and mdp_set_act_spaces is the judge: a
        scenario added there with a fixed or speaking agent needs its line here.)"""
        kinds = ["discrete" if (self.name == "simple_speaker_listener" and i == 0) else "box"
                 for i in range(self.n_agents)]
        dims = [2 if k == "box" else a for k, a in zip(kinds, self.act_dims)]
        return ScenarioSpec(self.name, self.n_agents, self.num_adversaries, list(self.obs_dims), dims, kinds)

    @property
    def observation_shapes(self):
        return [(o,) for o in self.obs_dims]


def spec(name, n_agents=None, num_adversaries=None, continuous=False):
    """Scenario table (upstream make_world defaults unless overridden);
    continuous: Box spaces where the scenario allows them (ScenarioSpec.continuous)."""
    if continuous:
        return spec(name, n_agents, num_adversaries).continuous()
    if name == "simple":
        return ScenarioSpec(name, 1, 0, [4])
    if name == "simple_spread":
        n = 3 if n_agents is None else n_agents
        return ScenarioSpec(name, n, 0, [4 + 2 * n + 4 * (n - 1)] * n)
    if name == "simple_adversary":
        n = 3 if n_agents is None else n_agents
        na = 1 if num_adversaries is None else num_adversaries
        dims = [(0 if i < na else 2) + 4 * (n - 1) for i in range(n)]
        return ScenarioSpec(name, n, na, dims)
    if name == "simple_tag":
        n = 4 if n_agents is None else n_agents
        na = 3 if num_adversaries is None else num_adversaries
        ng = n - na
        L = 2
        dims = [4 + 2 * L + 2 * (n - 1) + 2 * (ng if i < na else ng - 1) for i in range(n)]
        return ScenarioSpec(name, n, na, dims)
    if name == "simple_speaker_listener":
        # the speaker (agent 0) sees the goal colour and says one of dim_c = 3 words; the
        # listener sees its velocity, the 3 landmarks and the word (restated: parity UNPINNED)
        return ScenarioSpec(name, 2, 0, [3, 11], [3, 5])
    raise ValueError(f"unknown scenario {name!r}")


def minimax_eps(n_agents, num_adversaries, adv_eps=1e-3, adv_eps_s=1e-5):
    """M3DDPG's perturbation rates eps[i][j] (--minimax): adv_eps where agents i and j
    stand on opposite sides (the first num_adversaries agents are the adversaries),
    adv_eps_s where they stand on the same side; the diagonal is 0 (ignored)."""
    na = max(0, min(int(n_agents), int(num_adversaries)))
    eps = np.zeros((n_agents, n_agents), np.float32)
    for i in range(n_agents):
        for j in range(n_agents):
            if i != j:
                eps[i, j] = adv_eps if (i < na) != (j < na) else adv_eps_s
    return eps


def bench_record(sp, row, i):
    """Python value of agent i's scenario benchmark_data() (MPE returns tuples /
    ints / floats; train.py:141 stores them in info_n['n']) from its device
    record row (mdp_env_step_bench, MDP_BENCH_W floats)."""
    if sp.name == "simple_spread":
        return (float(row[0]), int(round(row[1])), float(row[2]), int(round(row[3])))
    if sp.name == "simple_adversary":
        if i < sp.num_adversaries:
            return float(row[0])
        return tuple(float(x) for x in row[:sp.n_agents])   # n-1 landmarks + goal
    if sp.name == "simple_tag":
        return int(round(row[0]))
    if sp.name == "simple_speaker_listener":
        raise AttributeError("simple_speaker_listener: upstream's benchmark_data raises (undefined name)")
    raise AttributeError(f"scenario {sp.name!r} has no benchmark_data")
