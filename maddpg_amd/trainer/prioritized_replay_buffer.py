"""``PrioritizedReplayMemory`` drop-in (``maddpg/trainer/prioritized_replay_buffer.py``,
proportional prioritization after Schaul et al. 2016).

Same constructor and methods -- ``add``, ``sample(n) -> (b_idx, b_memory,
ISWeights)``, ``batch_update(idx, abs_errors)`` -- and the same constants
(``epsilon``, ``alpha``, ``beta``, ``beta_increment_per_sampling``,
``abs_err_upper``, read when the first transition arrives).  The transitions live in
the replay ring of a private single-agent engine (as a standalone
``ReplayBuffer``), the priorities in its device sum tree (``mdp_per_*``).

Departures from the reference module (DESIGN.md "Prioritized replay"): a new
transition gets the largest priority ``abs_err_upper ** alpha`` (the reference:
``1e6``); the smallest probability is taken over filled leaves only; the leaf
offset is not off by one; ``b_idx`` holds ring positions (what
``batch_update`` takes back), not tree indices.
"""
import numpy as np
import torch

from .replay_buffer import ReplayBuffer


class PrioritizedReplayMemory(object):
    epsilon = 0.01
    alpha = 0.6
    beta = 0.4
    beta_increment_per_sampling = 0.001
    abs_err_upper = 1.

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self._ring = _Ring(self.capacity, self)

    def __len__(self):
        return len(self._ring)

    def add(self, obs_t, action, reward, obs_tp1, done):
        self._ring.add(obs_t, action, reward, obs_tp1, float(done))

    def sample(self, n):
        """n transitions, one per equal segment of the total priority: (positions,
        (obs, act, rew, obs_next, done) columns, importance-sampling weights)"""
        eng = self._ring.sync_ring()
        idx, w = eng.per_sample(0, int(n))
        self.beta = float(eng.per_info(0)["beta"])
        b_idx = idx.cpu().numpy().tolist()
        b_memory = self._ring.sample_index(idx)
        return b_idx, b_memory, w.cpu().numpy().tolist()

    def batch_update(self, tree_idx, abs_errors):
        eng = self._ring.sync_ring()
        pos = np.asarray(list(tree_idx), np.int64).astype(np.int32)
        err = np.abs(np.asarray(abs_errors, np.float32)).reshape(-1)
        eng.per_update_errors(0, torch.from_numpy(pos), torch.from_numpy(err))

    def priorities(self):
        """the filled leaves' priorities, by ring position"""
        eng = self._ring.sync_ring()
        t = eng.per_tree(0)
        return t[len(t) // 2: len(t) // 2 + len(self), 0].copy()


class _Ring(ReplayBuffer):
    """a standalone ReplayBuffer whose private engine carries the sum tree"""

    def __init__(self, size, owner):
        super().__init__(size)
        self._owner = owner

    def _eng(self, obs_dim=None):
        if self._engine is None:
            if obs_dim is None:
                raise RuntimeError("empty PrioritizedReplayMemory")
            from ..engine import Engine
            o = self._owner
            self._engine = Engine([obs_dim], batch_size=1, capacity=self._maxsize, prioritized=True,
                                  per_alpha=o.alpha, per_beta0=o.beta, per_beta_inc=o.beta_increment_per_sampling,
                                  per_eps=o.epsilon, per_abs_err_upper=o.abs_err_upper)
        return self._engine
