"""Batched numpy fp64 restatement of MPE's ``simple_speaker_listener`` in the
style of ``oracle/mpe.py`` (test helper).

Recalled from upstream ``multiagent/scenarios/simple_speaker_listener.py``,
``core.py`` (World.step: update_agent_state sets ``state.c = action.c`` for a
non-silent agent, zero for a silent one, after the positions were integrated)
and ``environment.py`` (_set_action: an immovable agent's Discrete action is
its ``action.c``).  MPE is neither vendored by the reference nor installed
here: parity is UNPINNED, like the scenarios of ``oracle/mpe.py``.

State: ``pos``, ``vel`` [E, 5, 2] (speaker, listener, 3 landmarks), ``goal`` [E]
and ``comm`` [E, 2, 3] (``state.c`` of both agents).
"""
import numpy as np

from oracle import mpe

DIM_C = 3


class SimpleSpeakerListener(mpe.Scenario):
    name = "simple_speaker_listener"
    collaborative = True

    def __init__(self):
        super().__init__()
        self.n_agents, self.n_landmarks = 2, 3
        self.size = [0.075, 0.075] + [0.04] * 3
        self.collide = [False] * 5
        self.movable = [False, True] + [False] * 3        # the speaker does not move
        self.silent = [False, True]                        # the listener does not speak
        self.accel = [None, None]
        self.max_speed = [None] * 5
        self.adversary = [False, False]
        self.act_dims = [DIM_C, 5]

    def reset(self, rng, E):
        goal = rng.integers(0, 3, size=E)
        pos = np.zeros((E, 5, 2))
        for e in range(5):                                 # agents, then landmarks: all U(-1, 1)^2
            pos[:, e] = rng.uniform(-1, 1, (E, 2))
        return {"pos": pos, "vel": np.zeros((E, 5, 2)), "goal": goal, "comm": np.zeros((E, 2, DIM_C))}

    def observation(self, st):
        p, v = st["pos"], st["vel"]
        E = p.shape[0]
        colour = np.full((E, 3), 0.15)
        colour[np.arange(E), st["goal"]] = 0.65            # landmark l: 0.65 in component l
        comm = st.get("comm")
        comm = np.zeros((E, 2, DIM_C)) if comm is None else comm
        listener = np.concatenate([v[:, 1]] + [p[:, 2 + l] - p[:, 1] for l in range(3)] + [comm[:, 0]], 1)
        return [colour, listener]

    def reward(self, st):
        p = st["pos"]
        E = p.shape[0]
        g = p[np.arange(E), 2 + st["goal"]]
        r = -np.sum(np.square(p[:, 1] - g), axis=1)        # each agent's own reward; step() sums them
        return np.stack([r, r], 1)

    def step(self, st, actions):
        """actions [E, 2, 5]: the speaker's 3-vector padded with zeros (its force is
        computed and never integrated: movable is False).  Returns the new state
        (with ``comm``), obs_n, rew [E, 2]."""
        actions = np.asarray(actions, np.float64)
        base = {k: v for k, v in st.items() if k != "comm"}
        nst, _obs, _rew = super().step(base, actions)
        comm = np.zeros((actions.shape[0], 2, DIM_C))
        comm[:, 0] = actions[:, 0, :DIM_C]                 # speaker.state.c = action.c (no noise)
        nst["comm"] = comm                                 # listener.state.c = 0 (silent)
        obs = self.observation(nst)
        rew = np.repeat(self.reward(nst).sum(1, keepdims=True), 2, axis=1)
        return nst, obs, rew
