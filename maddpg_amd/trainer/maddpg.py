"""``MADDPGAgentTrainer`` drop-in (``maddpg/trainer/maddpg.py:112-196``).

Same constructor, methods, attributes and return values.  Every trainer built
in one session shares one device engine (see ``common/tf_util.py``); its
``update`` runs on the GPU in the reference's order: gates (``:162-165``),
``make_index`` from the global ``random`` stream (``:167``), gather of every
agent's buffer with that index (``:173-178``, fused into the grad kernels),
target actors + target critic + fp64 TD target (``:180-187``), critic step
(``:188``), actor step against the updated critic (``:191``), Polyak actor
then critic (``:193-194``).  ``update`` returns the 6 stats of ``:196`` as
the reference does: a ``list`` of numpy scalars with its dtypes (``q_loss``,
``p_loss`` and ``mean(target_q_next)`` fp32, the rest float64 --
``engine.UPDATE_STAT_DTYPES``), read after the update (the reference's
``session.run`` is synchronous too).

With ``args.td3`` (``--td3``, ``args.policy_delay`` default 2) the session's
engine is a MATD3 one (``DESIGN.md`` section 17): ``update`` runs the twin critic step
and, every ``policy_delay``-th time, the actor step and the Polyak updates; the
returned list keeps its dtypes, with ``q_loss`` critic 1's, ``p_loss`` that of
this agent's most recent actor step (0 before the first) and
``mean(target_q_next)`` the mean of the smaller target Q.

With ``args.minimax`` (``--minimax``, ``args.adv_eps`` / ``args.adv_eps_s`` default
1e-3 / 1e-5, sides from ``args.num_adversaries``) the session's engine is an
M3DDPG one (``DESIGN.md`` section 20): ``p_loss`` and ``mean(target_q_next)`` are
taken at the perturbed actions.

With ``args.approx_policies`` (``--approx-policies``, ``args.approx_lambda`` default
1e-3) the session's engine learns approximators of the other agents' policies
from replay and builds every TD target from them (``DESIGN.md`` section 21); the
returned list is unchanged.

``model`` must be the reference's ``mlp_model`` (``train.py:39-46``: two
hidden ReLU layers of ``args.num_units`` and a linear output, TF
``fully_connected`` with Xavier-uniform weights) -- the architecture the HIP
kernels implement, for any ``--num-units`` up to 256.  It is recognised by name
(the reference's own function, or :func:`mlp_model` below), ``None`` selects
it; any other callable raises ``NotImplementedError`` rather than silently
training a different network.
"""
import numpy as np
import torch

from .. import AgentTrainer
from ..common import tf_util as U
from ..engine import update_stats
from .replay_buffer import ReplayBuffer


MAX_UNITS = 256


def mlp_model(input, num_outputs, scope, reuse=False, num_units=64, rnn_cell=None):
    """The reference's model function (``experiments/train.py:39-46``), kept as
    the architecture marker: the network itself is built by the device engine."""
    raise NotImplementedError("mlp_model is realised by the MI355X kernels; pass it to MADDPGAgentTrainer")


def check_model(model, num_units):
    """``model`` must describe the reference's mlp_model (see module doc)."""
    if model is not None and getattr(model, "__name__", None) != "mlp_model":
        raise NotImplementedError(
            f"model {model!r} is not mlp_model: the MI355X kernels implement the reference's 2-hidden-layer "
            "ReLU MLP (experiments/train.py:39-46) only")
    if not 1 <= int(num_units) <= MAX_UNITS:
        raise ValueError(f"--num-units {num_units}: the kernels take 1..{MAX_UNITS} hidden units")


class MADDPGAgentTrainer(AgentTrainer):
    def __init__(self, name, model, obs_shape_n, act_space_n, agent_index, args, local_q_func=False):
        self.name = name
        self.n = len(obs_shape_n)
        self.agent_index = agent_index
        self.args = args
        self.obs_shape_n = [tuple(s) for s in obs_shape_n]
        self.act_space_n = act_space_n
        self.local_q_func = local_q_func
        check_model(model, args.num_units)
        # one space per agent (make_pdtype, distributions.py:408-422): Discrete(k), k in
        # 1..5, or Box(d), d in {1, 2} -- an entry with a 1-D shape and no n (the reference
        # raises on anything else: its MultiDiscrete branch is commented out)
        self.act_dims, self.act_kinds = [], []
        for sp in act_space_n:
            shape = getattr(sp, "shape", None)
            if not hasattr(sp, "n") and shape is not None and len(tuple(shape)) == 1:
                d = int(tuple(shape)[0])
                if d not in (1, 2):
                    raise NotImplementedError(f"action space {sp!r}: Box(d) is supported for d in (1, 2)")
                self.act_dims.append(d)
                self.act_kinds.append("box")
                continue
            k = getattr(sp, "n", 5)
            if not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 5:
                raise NotImplementedError(f"action space {sp!r}: only Discrete(k), 1 <= k <= 5, and Box(d), "
                                          "d in (1, 2), are supported")
            self.act_dims.append(int(k))
            self.act_kinds.append("discrete")
        # args.action_squash "tanh": every Box agent plays tanh of its sample (bounded
        # actions); without the setting a Box entry stays a plain Gaussian
        squash = getattr(args, "action_squash", "none") or "none"
        if squash not in ("none", "tanh"):
            raise ValueError(f"action_squash {squash!r}: none or tanh")
        self.act_squash = [squash if k == "box" else "none" for k in self.act_kinds]
        # args.entropy_alpha: every Box agent's entropy coefficient (soft MADDPG); 0: none
        alpha = float(getattr(args, "entropy_alpha", 0.0) or 0.0)
        if not np.isfinite(alpha) or alpha < 0:
            raise ValueError(f"entropy_alpha {alpha!r}: finite and >= 0")
        self.act_entropy = [alpha if k == "box" else 0.0 for k in self.act_kinds]
        self.session = U.get_session()
        self.session.register(self)
        self.replay_buffer = ReplayBuffer(1e6, _session=self.session, _agent=agent_index)
        self.max_replay_buffer_len = args.batch_size * args.max_episode_len
        self.replay_sample_index = None
        i = agent_index
        self.p_debug = {"p_values": lambda obs: self._eng().actor_logits(i, self._t(obs)).cpu().numpy(),
                        "target_act": lambda obs: self._eng().act(i, self._t(obs), target=True).cpu().numpy()}
        self.q_debug = {"q_values": lambda *a: self._q(a, False), "target_q_values": lambda *a: self._q(a, True)}

    # ------------------------------------------------------------ helpers
    def _eng(self):
        return self.session.engine()

    @staticmethod
    def _t(x):
        return torch.as_tensor(np.asarray(x, np.float32))

    def _q(self, arrays, target):
        n = self.n
        obs_n, act_n = list(arrays[:n]), list(arrays[n:2 * n])
        i = self.agent_index
        if self.local_q_func:                                          # maddpg.py:86-87
            x = [np.asarray(obs_n[i], np.float32), np.asarray(act_n[i], np.float32)]
        else:                                                          # :85
            x = [np.asarray(a, np.float32) for a in obs_n + act_n]
        return self._eng().q_values(i, self._t(np.concatenate(x, 1)), target=target).cpu().numpy()

    # ------------------------------------------------------------ surface
    def action(self, obs):
        """act(obs[None])[0] (maddpg.py:151-152): actor + Gumbel-softmax sample."""
        return self._eng().act(self.agent_index, self._t(np.asarray(obs)[None])).cpu().numpy()[0]

    def experience(self, obs, act, rew, new_obs, done, terminal):
        self.replay_buffer.add(obs, act, rew, new_obs, float(done))    # :154-156

    def preupdate(self):
        self.replay_sample_index = None

    def update(self, agents, t):
        if len(self.replay_buffer) < self.max_replay_buffer_len:    # :162-163
            return None
        if not t % 100 == 0:                                          # :164-165
            return None
        for a in agents:
            if a.session is not self.session:
                raise RuntimeError("all agents of an update must share one session")
        eng = self._eng()
        self.session.flush()
        if eng.prioritized:
            # --prioritized-replay: the rows come from this agent's sum tree on the
            # device (no draw from the global ``random`` stream), the critic step is
            # importance-weighted and writes the rows' priorities back
            self.replay_buffer.sync_ring()
            eng.update(self.agent_index)
            self.replay_sample_index = eng.per_slots(self.agent_index)[0].clone()
        else:
            idx = self.replay_buffer.make_index_device(self.args.batch_size)   # :167
            self.replay_sample_index = idx
            eng.update(self.agent_index, idx=idx)                       # :173-194
        host, ev = eng.stats_future(self.agent_index)
        ev.synchronize()
        if self.session.check_nan:                                      # tf_util.py:366-368
            U.check_nan(eng)
        return update_stats(host.tolist())                              # :196
