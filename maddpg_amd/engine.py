"""Engine: one libmaddpg_hip handle + its device arena (PyTorch storage only).

Everything the reference keeps in the TF session (weights, targets, Adam
slots, beta powers -- ``tf_util.py:189-214``) and in the per-agent Python
replay lists (``replay_buffer.py``) lives in one device arena owned by a
``torch.uint8`` CUDA tensor; all compute is launched by the HIP library on
the engine's stream.  No CPU fallback exists: construction raises without a
GPU or without the built library.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, variants
from ._lib import MdpConfig, MdpTensorInfo

TENSOR_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")

# the dtypes of update()'s return value in the reference (maddpg.py:196):
# q_loss, p_loss are the fp32 scalars U.function fetches from TF1 (:91, :54-56);
# np.mean(target_q_next) is the mean of an fp32 array (fp32, :185); the mean
# and std of the fp64 TD target and the mean reward are float64 (:186)
UPDATE_STAT_DTYPES = (np.float32, np.float32, np.float64, np.float64, np.float32, np.float64)


def update_stats(vals):
    """the 6 device stats (fp64, mdp_get_stats) as the reference's list of numpy scalars"""
    return [dt(v) for dt, v in zip(UPDATE_STAT_DTYPES, list(vals))]


def read_checkpoint(fname, path, n, sets):
    """(state_dict()-style dict, the path that was read) of a checkpoint of `n`
    agents' parameter sets `sets` (Engine.load_state, Engine.bank_write).
    Read from a TF1 tensor bundle at prefix `fname` (the reference's
    tf.train.Saver checkpoint, tf_util.py:259-264) or from the .npz `path`
    that save_state writes.  save_state removes the other format's files, so
    both exist only when another tool wrote one of them: then the newer
    one (nanosecond modification times) is read; on a tie (a copy that
    kept timestamps, a tar archive's whole-second times) the TF1 bundle,
    the reference's own format, is read and a warning names the choice."""
    from .common import tf_checkpoint as tfc
    if tfc.is_bundle(fname) and os.path.isfile(path):
        t_npz, t_tf1 = os.stat(path).st_mtime_ns, os.stat(fname + ".index").st_mtime_ns
        if t_npz == t_tf1:
            import warnings
            warnings.warn(f"both {path} and the TF1 bundle {fname}.index exist with the same modification "
                          f"time; restoring the TF1 bundle (remove it to restore the .npz)")
        use_tf1 = t_tf1 >= t_npz
    else:
        use_tf1 = tfc.is_bundle(fname)
    if use_tf1:
        return tfc.state_from_tf1(tfc.read_bundle(fname), n, sets), fname
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}, path


class Engine:
    def __init__(self, obs_dims, local_q=None, *, num_units=64, batch_size=1024, max_episode_len=25,
                 capacity=int(1e6), num_envs=0, scenario="none", num_adversaries=0, lr=1e-2,
                 gamma=0.95, tau=1e-2, grad_clip=0.5, actor_reg=1e-3, adam_b1=0.9, adam_b2=0.999,
                 adam_eps=1e-8, seed=0, world_size=1, rank=0, device=None, episode_log_rows=0,
                 prioritized=False, per_alpha=0.6, per_beta0=0.4, per_beta_inc=0.001, per_eps=0.01,
                 per_abs_err_upper=1.0, act_dims=None, act_kinds=None, act_squash=None, act_entropy=None, td3=False, policy_delay=2, minimax=False, adv_eps=1e-3,
                 adv_eps_s=1e-5, minimax_eps=None, approx=False, approx_lambda=1e-3):
        """approx: MADDPG with inferred policies (mdp_approx_enable; Lowe et al. 2017,
        section 4.2) -- every agent i with a MADDPG critic learns an approximator of
        every other agent's policy from replay (cross-entropy of the replayed
        action + approx_lambda x entropy) and builds its TD target from the
        approximators' target networks instead of the others' target actors;
        strict mode, one GPU, none of prioritized / td3 / minimax.
        minimax: M3DDPG (mdp_minimax_enable) -- in the critic target and the actor
        loss the other agents' actions move one normalised gradient step against
        this agent's Q; rates adv_eps across the sides of num_adversaries and
        adv_eps_s within a side, or minimax_eps, an n x n array eps[i][j] (which
        alone also enables it); strict mode, one GPU, no prioritized replay, no td3.
        td3: MATD3 (mdp_td3_enable) -- twin critics, the TD target from the smaller
        target critic, the actor and the targets updated every policy_delay-th
        critic step (1..8); strict mode, one GPU, no prioritized replay.
        act_dims: per-agent action widths A_i in 1..5 (Discrete(A_i)); None: 5 for
        every agent, or the scenario's own.  The device keeps every action slot 5
        wide with zero pad entries; this class pads and slices at its boundary.
        act_kinds: per-agent "discrete" / "box" (or MDP_ACT_DISCRETE 0 / MDP_ACT_BOX 1)
        beside act_dims (mdp_set_act_spaces): a "box" agent has a Box(act_dims[i])
        space, act_dims[i] in {1, 2}, and a diagonal-Gaussian policy whose head
        (actor_logits) is [mean | logstd], 2 act_dims[i] wide.  With a scenario,
        act_dims may be None: a box agent is Box(2), the others keep their own
        space.  Strict mode, one GPU, none of prioritized / td3 / minimax / approx.
        act_squash: per-agent None / "none" / "tanh" (or MDP_SQUASH_NONE 0 /
        MDP_SQUASH_TANH 1; mdp_set_act_squash): a "tanh" agent, which must be a box
        agent, plays tanh of its Gaussian sample, an action inside [-1, 1].
        act_entropy: per-agent entropy coefficient alpha_i >= 0 (None: 0;
        mdp_set_act_entropy): a box agent with alpha_i > 0 maximises its reward plus
        alpha_i times its own policy's entropy (soft MADDPG)."""
        # one variant per handle, on one GPU (variants.py): refused here, before
        # anything is allocated or created on the device
        minimax = bool(minimax) or minimax_eps is not None
        why = variants.engine_refusal(dict(prioritized=prioritized, td3=td3, minimax=minimax, approx=approx),
                                      int(world_size))
        if why:
            raise _lib.MdpError(why)
        if approx and not (np.isfinite(float(approx_lambda)) and float(approx_lambda) >= 0):
            raise _lib.MdpError(f"approx_lambda must be finite and >= 0, got {approx_lambda!r}")
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("maddpg_amd runs on a ROCm GPU only (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        n = len(obs_dims)
        local_q = [False] * n if local_q is None else list(local_q)
        self.n = n
        self.obs_dims = [int(o) for o in obs_dims]
        self.local_q = [bool(x) for x in local_q]
        self.update_mode = "strict"
        self.num_units = int(num_units)
        self.batch_size = int(batch_size)
        self.max_episode_len = int(max_episode_len)
        self.capacity = int(capacity)
        self.num_envs = int(num_envs)
        self.scenario = scenario
        self.world_size, self.rank = int(world_size), int(rank)
        self.approx = bool(approx)
        self.approx_lambda = float(approx_lambda)
        self.approx_buf = None
        cfg = MdpConfig()
        cfg.n_agents = n
        for i in range(n):
            cfg.obs_dim[i] = self.obs_dims[i]
            cfg.local_q[i] = 1 if self.local_q[i] else 0
        cfg.act_dim = _lib.ACT_DIM
        cfg.num_units = self.num_units
        cfg.batch_size = self.batch_size
        cfg.max_episode_len = self.max_episode_len
        cfg.capacity = self.capacity
        cfg.num_envs = self.num_envs
        cfg.scenario = _lib.SCN[scenario]
        cfg.num_adversaries = int(num_adversaries)
        cfg.world_size, cfg.rank = self.world_size, self.rank
        cfg.lr, cfg.tau, cfg.grad_clip, cfg.actor_reg = lr, tau, grad_clip, actor_reg
        cfg.adam_b1, cfg.adam_b2, cfg.adam_eps = adam_b1, adam_b2, adam_eps
        cfg.gamma = float(gamma)
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.episode_log_rows = int(episode_log_rows)
        self.cfg = cfg
        pt = ctypes.c_int64()
        nbytes = self.lib.mdp_arena_bytes(ctypes.byref(cfg), ctypes.byref(pt))
        if nbytes < 0:
            raise ValueError(f"invalid maddpg configuration: {self._config_error(cfg)}")
        self.param_floats = pt.value
        with torch.cuda.device(self.device):
            self.arena = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.stream = torch.cuda.Stream(device=self.device)
            h = ctypes.c_void_p()
            rc = self.lib.mdp_create(ctypes.byref(cfg), ctypes.c_void_p(self.arena.data_ptr()), nbytes,
                                     ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(h))
        self.h = h
        if rc != 0:
            msg = self.lib.mdp_last_error(h).decode()
            self.lib.mdp_destroy(h)
            self.h = None
            raise ValueError(f"mdp_create failed: {msg}")
        dims = (ctypes.c_int32 * _lib.MAX_AGENTS)()
        if act_kinds is not None:
            try:
                if len(act_kinds) != n or (act_dims is not None and len(act_dims) != n):
                    raise ValueError(f"act_kinds / act_dims need one entry for each of the {n} agents")
                kinds = [self._act_kind(k) for k in act_kinds]
                if act_dims is None:
                    self._c("mdp_get_act_dims", dims)
                    act_dims = [2 if kinds[i] == _lib.ACT_BOX else int(dims[i]) for i in range(n)]
                self.set_act_spaces(kinds, act_dims)
            except (ValueError, _lib.MdpError) as e:
                self.close()
                raise ValueError(str(e)) from None
        elif act_dims is not None:
            if len(act_dims) != n:
                self.close()
                raise ValueError(f"act_dims has {len(act_dims)} entries for {n} agents")
            for i in range(n):
                dims[i] = int(act_dims[i])
            rc = self.lib.mdp_set_act_dims(self.h, dims)
            if rc != 0:
                msg = self.lib.mdp_last_error(self.h).decode()
                self.close()
                raise ValueError(msg)
        if hasattr(self.lib, "mdp_get_act_dims"):
            self._c("mdp_get_act_dims", dims)
            self.act_dims = [int(dims[i]) for i in range(n)]
        else:   # an older build chosen with MDP_LIB (A/B): every width is 5 there
            self.act_dims = [_lib.ACT_DIM] * n
        self.act_kinds = ["discrete"] * n
        if hasattr(self.lib, "mdp_get_act_spaces"):
            kk = (ctypes.c_int32 * _lib.MAX_AGENTS)()
            self._c("mdp_get_act_spaces", kk, None)
            self.act_kinds = ["box" if kk[i] == _lib.ACT_BOX else "discrete" for i in range(n)]
        if act_squash is not None:
            try:
                if len(act_squash) != n:
                    raise ValueError(f"act_squash needs one entry for each of the {n} agents")
                self.set_act_squash(act_squash)
            except (ValueError, _lib.MdpError) as e:
                self.close()
                raise ValueError(str(e)) from None
        if act_entropy is not None:
            try:
                if len(act_entropy) != n:
                    raise ValueError(f"act_entropy needs one entry for each of the {n} agents")
                self.set_act_entropy(act_entropy)
            except (ValueError, TypeError, _lib.MdpError) as e:
                self.close()
                raise ValueError(str(e)) from None
        lay = (ctypes.c_int32 * 6)()
        self.row_layout = []
        for i in range(n):
            self._c("mdp_row_layout", i, lay)
            self.row_layout.append(tuple(lay[:6]))
        self.row_stride = self.row_layout[0][5]
        self._tensors = {}
        for i in range(n):
            for net in (0, 1):
                infos = []
                for t in range(6):
                    ti = MdpTensorInfo()
                    self._c("mdp_tensor", i, net, t, ctypes.byref(ti))
                    infos.append((ti.offset, ti.rows, ti.cols, ti.dev_rows, ti.dev_cols))
                self._tensors[(i, net)] = infos
        self.prioritized = bool(prioritized)
        self.per_buf = None
        self.td3 = bool(td3)
        self.policy_delay = int(policy_delay)
        self.td3_buf = None
        self.minimax = minimax
        self.minimax_eps = None
        if self.prioritized:
            self._per_enable(per_alpha, per_beta0, per_beta_inc, per_eps, per_abs_err_upper)
        if self.td3:
            self._td3_enable(self.policy_delay)
        if self.minimax:
            from .envs import minimax_eps as _eps
            self._minimax_enable(_eps(n, int(num_adversaries), adv_eps, adv_eps_s) if minimax_eps is None
                                 else minimax_eps)
        if self.approx:
            self._approx_enable(self.approx_lambda)

    # ------------------------------------------------------------ plumbing
    def _c(self, name, *args):
        rc = getattr(self.lib, name)(self.h, *args)
        return _lib.check(self.lib, self.h, rc, name)

    def _config_error(self, cfg):
        """why mdp_arena_bytes refused `cfg`: mdp_create validates the same layout
        first and keeps the message on the handle it returns (no GPU call)"""
        h = ctypes.c_void_p()
        self.lib.mdp_create(ctypes.byref(cfg), None, 0, None, ctypes.byref(h))
        msg = self.lib.mdp_last_error(h).decode() if h.value else "mdp_create returned no handle"
        self.lib.mdp_destroy(h)
        return msg

    def close(self):
        if getattr(self, "h", None):
            self.lib.mdp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync_in(self):
        """engine stream waits for work torch queued on the current stream"""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def sync_out(self):
        """torch's current stream waits for the engine stream"""
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def synchronize(self):
        self._c("mdp_synchronize")

    @staticmethod
    def _ptr(t):
        """device pointer of a tensor for the C ABI (null for None).  A host tensor is
        refused: the kernels would dereference its address on the device."""
        if t is None:
            return ctypes.c_void_p(0)
        if not t.is_cuda:
            raise ValueError("the C ABI takes device tensors; got a host tensor")
        return ctypes.c_void_p(t.data_ptr())

    def region(self, name, dtype=torch.float32):
        off, nb = ctypes.c_int64(), ctypes.c_int64()
        self._c("mdp_region", _lib.REGION[name], ctypes.byref(off), ctypes.byref(nb))
        isz = torch.tensor([], dtype=dtype).element_size()
        return self.arena[off.value: off.value + (nb.value // isz) * isz].view(dtype)

    def net_tensors(self, agent, net):
        return self._tensors[(agent, net)]

    def grad_view(self, agent, net):
        """float32 view of one net's gradient in the GRAD region (all-reduce target)."""
        infos = self._tensors[(agent, net)]
        start = infos[0][0]
        end = infos[5][0] + ((infos[5][3] * infos[5][4] + 3) // 4) * 4
        return self.region("grad")[start:end]

    # ------------------------------------------------------- action widths
    def set_act_dims(self, act_dims):
        """mdp_set_act_dims on this handle (refused once it has been used)"""
        dims = (ctypes.c_int32 * _lib.MAX_AGENTS)(*[int(a) for a in act_dims])
        self._c("mdp_set_act_dims", dims)

    @staticmethod
    def _act_kind(k):
        if k in ("discrete", _lib.ACT_DISCRETE):
            return _lib.ACT_DISCRETE
        if k in ("box", _lib.ACT_BOX):
            return _lib.ACT_BOX
        raise ValueError(f"unknown action kind {k!r} (discrete, box)")

    def set_act_spaces(self, act_kinds, act_dims):
        """mdp_set_act_spaces on this handle (refused once it has been used)"""
        kinds = (ctypes.c_int32 * _lib.MAX_AGENTS)(*[self._act_kind(k) for k in act_kinds])
        dims = (ctypes.c_int32 * _lib.MAX_AGENTS)(*[int(a) for a in act_dims])
        self._c("mdp_set_act_spaces", kinds, dims)

    @staticmethod
    def _squash(s):
        if s in (None, "none", _lib.SQUASH_NONE):
            return _lib.SQUASH_NONE
        if s in ("tanh", _lib.SQUASH_TANH):
            return _lib.SQUASH_TANH
        raise ValueError(f"unknown action squash {s!r} (none, tanh)")

    def set_act_squash(self, act_squash):
        """mdp_set_act_squash on this handle (refused once it has been used)"""
        sq = (ctypes.c_int32 * _lib.MAX_AGENTS)(*[self._squash(s) for s in act_squash])
        self._c("mdp_set_act_squash", sq)

    @property
    def act_squash(self):
        """per agent "none" / "tanh" (mdp_get_act_squash)"""
        if not hasattr(self.lib, "mdp_get_act_squash"):   # an older build chosen with MDP_LIB (A/B)
            return ["none"] * self.n
        sq = (ctypes.c_int32 * _lib.MAX_AGENTS)()
        self._c("mdp_get_act_squash", sq)
        return ["tanh" if sq[i] == _lib.SQUASH_TANH else "none" for i in range(self.n)]

    def set_act_entropy(self, act_entropy):
        """mdp_set_act_entropy on this handle (refused once it has been used); None is 0"""
        al = (ctypes.c_float * _lib.MAX_AGENTS)(*[0.0 if a is None else float(a) for a in act_entropy])
        self._c("mdp_set_act_entropy", al)

    @property
    def act_entropy(self):
        """per agent entropy coefficient (mdp_get_act_entropy)"""
        if not hasattr(self.lib, "mdp_get_act_entropy"):   # an older build chosen with MDP_LIB (A/B)
            return [0.0] * self.n
        al = (ctypes.c_float * _lib.MAX_AGENTS)()
        self._c("mdp_get_act_entropy", al)
        return [float(al[i]) for i in range(self.n)]

    def entropy_info(self, agent):
        """mdp_entropy_info: {"alpha", "logp": mean log pi of the agent's last actor
        step, "logp_target": mean log pi' of its last critic step}"""
        out = (ctypes.c_double * 4)()
        self._c("mdp_entropy_info", int(agent), out)
        return {"alpha": out[0], "logp": out[1], "logp_target": out[2]}

    def is_box(self, agent):
        return self.act_kinds[agent] == "box"

    def head_dim(self, agent):
        """width of agent's actor head: A_i logits, or mean | logstd of a Box(d_i)"""
        return self.act_dims[agent] * (2 if self.is_box(agent) else 1)

    def pad_noise(self, agent, u):
        """uniforms [..., k] -> the device's [..., 5] slot.  A Discrete(A_i) agent reads
        the first A_i, a Box agent the first two (Box-Muller) whatever its width;
        entries that are not given are never read and are set to 0.5"""
        A = _lib.ACT_DIM
        if u.shape[-1] == A:
            return u
        w = 2 if self.is_box(agent) else self.act_dims[agent]
        if u.shape[-1] != w:
            raise ValueError(f"agent {agent}: noise of width {u.shape[-1]}, it reads {w} uniforms")
        out = u.new_full(u.shape[:-1] + (A,), 0.5)
        out[..., :w] = u
        return out

    def pad_act(self, agent, a):
        """[..., A_i] -> the device's [..., 5] slot with zero pad entries; an array
        that is already 5 wide passes as it is"""
        A, w = _lib.ACT_DIM, self.act_dims[agent]
        if a.shape[-1] == A:
            return a
        if a.shape[-1] != w:
            raise ValueError(f"agent {agent}: last dimension {a.shape[-1]}, its action width is {w}")
        out = a.new_zeros(a.shape[:-1] + (A,))
        out[..., :w] = a
        return out

    def cin_columns(self, agent):
        """device column of every logical column of agent's critic input
        concat(obs_n + act_n) (or obs_i + act_i for a DDPG critic)"""
        A = _lib.ACT_DIM
        if self.local_q[agent]:
            o = self.obs_dims[agent]
            return list(range(o + self.act_dims[agent]))
        so = sum(self.obs_dims)
        cols = list(range(so))
        for j in range(self.n):
            cols += [so + A * j + k for k in range(self.act_dims[j])]
        return cols

    def get_grads(self, agent):
        """{'actor': .., 'critic': ..}: the reduced gradients of agent's last update
        (logical shapes, as get_params)"""
        out = {"actor": self.get_params(agent, "g_actor"), "critic": self.get_params(agent, "g_critic")}
        if self.td3:
            out["critic2"] = self.get_params(agent, "g_critic2")
        return out

    # ---------------------------------------------------------- parameters
    def _flat_shapes(self, agent, which):
        net = 1 if "critic" in which else 0
        return [(r, c) for (_o, r, c, _dr, _dc) in self._tensors[(agent, net)]]

    def _flat_params(self, agent, which, params):
        """the logical layout mdp_set_params / mdp_actor_set_write take: a dict of
        the six tensors (reshaped to their logical shapes) or a flat array"""
        shapes = self._flat_shapes(agent, which)
        if isinstance(params, dict):
            for k, s in zip(TENSOR_NAMES, shapes):
                if np.size(params[k]) != s[0] * s[1]:
                    raise ValueError(f"agent {agent} {which}/{k}: shape {np.shape(params[k])} does not match the "
                                     f"handle's {s} (its action space: {self.act_kinds[agent]} "
                                     f"{self.act_dims[agent]})")
            parts = [np.asarray(params[k], np.float32).reshape(s) for k, s in zip(TENSOR_NAMES, shapes)]
            flat = np.concatenate([p.ravel() for p in parts])
        else:
            flat = np.asarray(params, np.float32).ravel()
        return np.ascontiguousarray(flat, np.float32)

    def set_params(self, agent, which, params):
        flat = self._flat_params(agent, which, params)
        self._c("mdp_set_params", agent, _lib.WHICH[which], _lib.fptr(flat), flat.size)

    def _read_params(self, agent, which, name, *ids):
        """the six tensors (logical shapes) that getter `name` writes as one flat array"""
        shapes = self._flat_shapes(agent, which)
        n = sum(r * c for r, c in shapes)
        flat = np.empty(n, np.float32)
        self._c(name, *ids, _lib.fptr(flat), n)
        out, s = {}, 0
        for k, (r, c) in zip(TENSOR_NAMES, shapes):
            a = flat[s:s + r * c].reshape(r, c)
            out[k] = a[0].copy() if k.startswith("b") else a.copy()
            s += r * c
        return out

    def get_params(self, agent, which):
        return self._read_params(agent, which, "mdp_get_params", agent, _lib.WHICH[which])

    def get_beta_powers(self, agent, net):
        b = np.empty(2, np.float32)
        self._c("mdp_get_beta_powers", agent, net, _lib.fptr(b))
        return b

    def set_beta_powers(self, agent, net, b):
        b = np.ascontiguousarray(b, np.float32)
        self._c("mdp_set_beta_powers", agent, net, _lib.fptr(b))

    def init_params(self, seed=0):
        """tf.contrib.layers xavier_initializer (uniform) for all four nets per
        agent, each drawn independently (targets are NOT copies: maddpg.py:66,104).
        A TD3 engine draws every agent's second critic and its target after all
        of those, from the same generator: the four nets' values for a seed are
        the same with and without td3."""
        rng = np.random.default_rng(seed)
        H = self.num_units

        def draw(i, which, write=True):
            shapes = self._flat_shapes(i, which)
            p = {}
            for k, (r, c) in zip(TENSOR_NAMES, shapes):
                if k.startswith("W"):
                    lim = np.sqrt(6.0 / (r + c))
                    p[k] = rng.uniform(-lim, lim, size=(r, c)).astype(np.float32)
                else:
                    p[k] = np.zeros((r, c), np.float32)
            if write:
                self.set_params(i, which, p)
            return p

        for i in range(self.n):
            for which in ("actor", "critic", "tgt_actor", "tgt_critic"):
                draw(i, which)
        if self.td3:
            for i in range(self.n):
                for which in ("critic2", "tgt_critic2"):
                    draw(i, which)
        # the approximators after all of those (a seed's existing nets do not
        # move); each target starts as a copy of its approximator
        for i, j in self.approx_pairs():
            p = draw(j, "actor", write=False)
            self.set_approx_params(i, j, "net", p)
            self.set_approx_params(i, j, "tgt", p)
        return H

    # --------------------------------------------------------- checkpoint
    SETS = ("actor", "critic", "tgt_actor", "tgt_critic", "m_actor", "v_actor", "m_critic", "v_critic")
    TD3_SETS = ("critic2", "tgt_critic2", "m_critic2", "v_critic2")

    def state_dict(self):
        """Every variable tf.train.Saver would save (tf_util.py:259-273): weights,
        targets, Adam slots and beta powers, keyed like the TF1 scopes.  A TD3
        engine adds the second critic's sets (TD3_SETS) and its beta powers; the
        per-agent update counters are not part of it (they restart at 0)."""
        out = {}
        for i in range(self.n):
            for w in self.SETS + (self.TD3_SETS if self.td3 else ()):
                for k, v in self.get_params(i, w).items():
                    out[f"agent_{i}/{w}/{k}"] = v
            out[f"agent_{i}/actor/beta_power"] = self.get_beta_powers(i, 0)
            out[f"agent_{i}/critic/beta_power"] = self.get_beta_powers(i, 1)
            if self.td3:
                out[f"agent_{i}/critic2/beta_power"] = self.get_beta_powers(i, 2)
        for i, j in self.approx_pairs():
            for w in self.APPROX_SETS:
                for k, v in self.get_approx_params(i, j, w).items():
                    out[f"agent_{i}/approx_{j}/{w}/{k}"] = v
            out[f"agent_{i}/approx_{j}/beta_power"] = self.get_approx_beta_powers(i, j)
        return out

    def load_state_dict(self, sd, agents=None):
        """agents: restore only these agents' parameter sets (None: every agent).
        sd["act_squash"] (an npz checkpoint's, Engine.load_state; a TF1 bundle has
        no place for it) must be the handle's for every agent restored: the actors
        were trained behind that squash."""
        todo = list(range(self.n)) if agents is None else sorted({int(a) for a in agents})
        for i in todo:
            if not 0 <= i < self.n:
                raise ValueError(f"agent {i} out of range for {self.n} agents")
        if "act_squash" in sd:
            want = [int(v) for v in np.asarray(sd["act_squash"]).ravel()]
            have = [self._squash(s) for s in self.act_squash]
            if len(want) != self.n or any(want[i] != have[i] for i in todo):
                names = {_lib.SQUASH_NONE: "none", _lib.SQUASH_TANH: "tanh"}
                raise ValueError(f"the checkpoint's action squash {[names.get(v, v) for v in want]} differs from the "
                                 f"handle's {[names[v] for v in have]} (Engine(act_squash=...), --action-squash)")
        if "act_entropy" in sd:
            want = [float(np.float32(v)) for v in np.asarray(sd["act_entropy"]).ravel()]
            have = self.act_entropy
            if len(want) != self.n or any(want[i] != have[i] for i in todo):
                raise ValueError(f"the checkpoint's entropy coefficients {want} differ from the handle's {have} "
                                 f"(Engine(act_entropy=...), --entropy-alpha)")
        for i in todo:
            for w in self.SETS:
                self.set_params(i, w, {k: sd[f"agent_{i}/{w}/{k}"] for k in TENSOR_NAMES})
            self.set_beta_powers(i, 0, sd[f"agent_{i}/actor/beta_power"])
            self.set_beta_powers(i, 1, sd[f"agent_{i}/critic/beta_power"])
            # the second critic's sets: restored when the engine has them and the
            # checkpoint holds them (a MADDPG checkpoint leaves the twin as it is;
            # a non-TD3 engine ignores the keys)
            if self.td3 and f"agent_{i}/critic2/beta_power" in sd:
                for w in self.TD3_SETS:
                    self.set_params(i, w, {k: sd[f"agent_{i}/{w}/{k}"] for k in TENSOR_NAMES})
                self.set_beta_powers(i, 2, sd[f"agent_{i}/critic2/beta_power"])
            # the approximators: restored when the engine has them and the checkpoint
            # holds them (a MADDPG checkpoint leaves them as they are)
            for oi, j in self.approx_pairs():
                if oi == i and f"agent_{i}/approx_{j}/beta_power" in sd:
                    for w in self.APPROX_SETS:
                        self.set_approx_params(i, j, w, {k: sd[f"agent_{i}/approx_{j}/{w}/{k}"] for k in TENSOR_NAMES})
                    self.set_approx_beta_powers(i, j, sd[f"agent_{i}/approx_{j}/beta_power"])

    @staticmethod
    def checkpoint_path(fname):
        if fname.endswith(".npz"):
            return fname
        if fname.endswith("/") or os.path.isdir(fname):
            return os.path.join(fname, "maddpg_amd_state.npz")
        return fname + ".npz"

    def save_state(self, fname, fmt="npz"):
        """fmt "npz": one .npz keyed like state_dict(); fmt "tf1": a TF1 tensor
        bundle at prefix `fname` with the reference's variable names, as
        tf.train.Saver().save(sess, fname) writes it (tf_util.py:267-273;
        `fname`.index + `fname`.data-00000-of-00001 + the `checkpoint` state
        file; no .meta -- the graph is built by code on both sides)."""
        for r in variants.VARIANTS:
            if fmt == "tf1" and r.npz_only and getattr(self, r.kw):
                raise ValueError(f"save_state(fmt='tf1') on an engine with {r.name} ({r.kw}): its state has no "
                                 "reference variable names; save as npz")
        if fmt == "tf1":
            from .common import tf_checkpoint as tfc
            self._drop_stale(fname, keep="tf1")
            tfc.write_bundle(fname, tfc.tf1_from_state(self.state_dict()))
            d = os.path.dirname(os.path.abspath(fname + "x"))
            with open(os.path.join(d, "checkpoint"), "w") as fh:
                p = os.path.abspath(fname) + ("/" if fname.endswith("/") else "")
                fh.write(f'model_checkpoint_path: "{p}"\nall_model_checkpoint_paths: "{p}"\n')
            return fname
        if fmt != "npz":
            raise ValueError(f"unknown checkpoint format {fmt!r} (npz, tf1)")
        path = self.checkpoint_path(fname)
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        self._drop_stale(fname, keep="npz")
        sd = self.state_dict()
        sq = self.act_squash
        if "tanh" in sq:    # (a TF1 bundle has no place for it: the squash is given again on restore)
            sd["act_squash"] = np.array([self._squash(s) for s in sq], np.int32)
        al = self.act_entropy
        if any(al):         # (as the squash: a TF1 bundle has no place for it)
            sd["act_entropy"] = np.array(al, np.float32)
        np.savez(path, **sd)
        return path

    def _drop_stale(self, fname, keep):
        """a save in one format removes the other format's files at the same
        prefix, so a later --restore cannot pick up an older checkpoint"""
        if keep == "npz":
            for f in (fname + ".index", fname + ".data-00000-of-00001"):
                if os.path.isfile(f):
                    os.remove(f)
        elif os.path.isfile(self.checkpoint_path(fname)):
            os.remove(self.checkpoint_path(fname))

    def load_state(self, fname, agents=None):
        """agents: a list restores only those agents' parameter sets (cross-play of
        two checkpoints); None restores every agent.  The checkpoint is read as
        read_checkpoint reads it."""
        sd, used = read_checkpoint(fname, self.checkpoint_path(fname), self.n, self.SETS)
        if str(used).endswith(".npz") and "act_squash" not in sd:
            sd["act_squash"] = np.zeros(self.n, np.int32)   # an npz without the array: no squash
        if str(used).endswith(".npz") and "act_entropy" not in sd:
            sd["act_entropy"] = np.zeros(self.n, np.float32)   # ... and no entropy coefficient
        more = () if agents is None else (agents,)
        self.load_state_dict(sd, *more)
        return used

    # ------------------------------------------------------------- replay
    def buffer_len(self):
        return int(self.lib.mdp_buffer_len(self.h))

    def add_rows(self, rows):
        rows = rows.to(self.device, torch.float32).contiguous()
        assert rows.dim() == 2 and rows.shape[1] == self.row_stride
        self.sync_in()
        self._c("mdp_buffer_add_rows", self._ptr(rows), rows.shape[0])
        self._keep = rows  # keep alive until the stream consumed it
        self.sync_out()

    def put_agent(self, agent, pos, cols):
        pos = pos.to(self.device, torch.int64).contiguous()
        cols = cols.to(self.device, torch.float32).contiguous()
        self.sync_in()
        self._c("mdp_buffer_put_agent", agent, self._ptr(pos), self._ptr(cols), pos.shape[0])
        self.sync_out()

    def set_ring(self, length, next_idx, rows_total=None):
        """host ring state to the device; rows_total: rows ever added (prioritized
        replay then resets exactly the rows added since the last call)"""
        if rows_total is None:
            self._c("mdp_buffer_set_len", int(length), int(next_idx))
        else:
            self._c("mdp_buffer_set_ring", int(length), int(next_idx), int(rows_total))

    def seed_py_random(self, seed):
        self._c("mdp_seed_py_random", int(seed) & 0xFFFFFFFFFFFFFFFF)

    def set_rng_state(self, state625):
        st = np.ascontiguousarray(np.asarray(state625, dtype=np.uint64).astype(np.uint32))
        assert st.size == 625
        self._c("mdp_set_rng_state", st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))

    def get_rng_state(self):
        st = np.empty(625, np.uint32)
        self._c("mdp_get_rng_state", st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        return st

    def make_index(self, count, out=None):
        if out is None:
            out = torch.empty(count, dtype=torch.int32, device=self.device)
        self.sync_in()
        self._c("mdp_make_index", int(count), self._ptr(out))
        self.sync_out()
        return out

    def sample_rows(self, idx, out=None):
        idx = idx.to(self.device, torch.int32).contiguous()
        if out is None:
            out = torch.empty((idx.shape[0], self.row_stride), dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_sample_rows", self._ptr(idx), idx.shape[0], self._ptr(out))
        self.sync_out()
        return out

    # -------------------------------------------------- prioritized replay
    def _per_enable(self, alpha, beta0, beta_inc, eps, upper):
        """device-side prioritized replay (mdp_per_enable): one sum tree per agent in
        a second device buffer; before the first update / train call"""
        nbytes = self.lib.mdp_per_bytes(ctypes.byref(self.cfg))
        if nbytes < 0:
            raise ValueError("mdp_per_bytes refused the configuration")
        with torch.cuda.device(self.device):
            self.per_buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        try:
            self._c("mdp_per_enable", self._ptr(self.per_buf), nbytes, float(alpha), float(beta0),
                    float(beta_inc), float(eps), float(upper))
        except _lib.MdpError:
            self.per_buf = None
            self.close()
            raise
        self.per_nodes = int(self.lib.mdp_per_tree_nodes(self.h))

    # --------------------------------------------------------------- MATD3
    def _td3_enable(self, policy_delay):
        """twin critics + delayed policy updates (mdp_td3_enable): the second
        critic's state in a second device buffer; before the first update / train call"""
        nbytes = self.lib.mdp_td3_bytes(ctypes.byref(self.cfg))
        if nbytes < 0:
            raise ValueError("mdp_td3_bytes refused the configuration")
        with torch.cuda.device(self.device):
            self.td3_buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        try:
            self._c("mdp_td3_enable", self._ptr(self.td3_buf), nbytes, int(policy_delay))
        except _lib.MdpError:
            self.td3_buf = None
            self.close()
            raise

    # -------------------------------------------------------------- M3DDPG
    def _minimax_enable(self, eps):
        """minimax critic targets and actor loss (mdp_minimax_enable) with the rates
        eps [n][n]; before the first update / train call"""
        eps = np.ascontiguousarray(np.asarray(eps, np.float32))
        if eps.shape != (self.n, self.n):
            self.close()
            raise ValueError(f"minimax_eps has shape {eps.shape} for {self.n} agents")
        try:
            self._c("mdp_minimax_enable", _lib.fptr(eps))
        except _lib.MdpError:
            self.close()
            raise
        self.minimax_eps = self.minimax_info()

    def minimax_info(self):
        """eps [n][n] as enabled, diagonal 0 (mdp_minimax_info)"""
        out = np.zeros((self.n, self.n), np.float32)
        self._c("mdp_minimax_info", _lib.fptr(out))
        return out

    def minimax_debug_adv(self, critic=True, actor=True):
        """debug buffers [B][n][5] (float32, device) that receive the actions the second
        forward of the next minimax critic / actor steps reads (mdp_minimax_debug_adv);
        returns (critic_adv, actor_adv), None where not asked for"""
        with torch.cuda.device(self.device):
            bufs = [torch.zeros(self.batch_size, self.n, _lib.ACT_DIM, dtype=torch.float32, device=self.device)
                    if on else None for on in (critic, actor)]
        self._c("mdp_minimax_debug_adv", *[None if b is None else self._ptr(b) for b in bufs])
        self._adv_bufs = bufs   # keep them alive while the handle points at them
        return tuple(bufs)

    # ------------------------------------------------- inferred policies
    APPROX_SETS = ("net", "tgt", "m", "v")

    def _approx_enable(self, lam):
        """approximators of the other agents' policies (mdp_approx_enable): their
        nets, targets, Adam slots, partials and sync area live in a second device
        buffer owned here"""
        nbytes = self.lib.mdp_approx_bytes(ctypes.byref(self.cfg))
        if nbytes < 0:
            raise ValueError("mdp_approx_bytes refused the configuration")
        with torch.cuda.device(self.device):
            self.approx_buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        try:
            self._c("mdp_approx_enable", self._ptr(self.approx_buf), nbytes, float(lam))
        except Exception:
            self.approx_buf = None
            self.close()
            raise

    def approx_pairs(self):
        """(observer, agent) of every approximator: observers with a MADDPG critic"""
        if not getattr(self, "approx", False):
            return []
        return [(i, j) for i in range(self.n) if not self.local_q[i] for j in range(self.n) if j != i]

    def set_approx_params(self, observer, agent, which, params):
        """set `which` (net, tgt, m, v, grad) of observer's approximator of agent, in
        agent's actor layout (mdp_approx_set_params)"""
        flat = self._flat_params(agent, "actor", params)
        self._c("mdp_approx_set_params", observer, agent, _lib.APX_WHICH[which], _lib.fptr(flat), flat.size)

    def get_approx_params(self, observer, agent, which):
        return self._read_params(agent, "actor", "mdp_approx_get_params", observer, agent, _lib.APX_WHICH[which])

    def get_approx_beta_powers(self, observer, agent):
        b = np.empty(2, np.float32)
        self._c("mdp_approx_get_beta_powers", observer, agent, _lib.fptr(b))
        return b

    def set_approx_beta_powers(self, observer, agent, b):
        b = np.ascontiguousarray(b, np.float32)
        self._c("mdp_approx_set_beta_powers", observer, agent, _lib.fptr(b))

    def approx_info(self, observer, agent):
        """{cross_entropy, entropy, loss, updates} of the pair's last gradient launch (mdp_approx_info)"""
        out = (ctypes.c_double * 4)()
        self._c("mdp_approx_info", int(observer), int(agent), out)
        return {"cross_entropy": out[0], "entropy": out[1], "loss": out[2], "updates": int(out[3])}

    def approx_logits(self, observer, agent, obs, target=False):
        """actor_logits on observer's approximator of agent (mdp_approx_logits)"""
        obs = obs.to(self.device, torch.float32).contiguous()
        out = torch.empty((obs.shape[0], _lib.ACT_DIM), dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_approx_logits", observer, agent, 1 if target else 0, self._ptr(obs), self._ptr(out), obs.shape[0])
        self.sync_out()
        return self._narrow(agent, out)

    def _approx_rows(self, name, observer, idx):
        if idx is None:
            raise ValueError(f"{name}: idx (the batch_size replay rows) is required")
        self._sized("idx", idx, self.batch_size)
        idx = idx.to(self.device, torch.int32).contiguous()
        self.sync_in()
        self._c(name, observer, self._ptr(idx))
        self._keep = [idx]
        self.sync_out()

    def approx_grad(self, observer, idx):
        """only the gradient kernel of observer's approximators on rows idx [batch_size]
        (mdp_approx_grad); get_approx_params(.., 'grad') then reads the raw gradients"""
        self._approx_rows("mdp_approx_grad", observer, idx)

    def approx_step(self, observer, idx):
        """one gradient step of every approximator of observer on rows idx (mdp_approx_step)"""
        self._approx_rows("mdp_approx_step", observer, idx)

    def approx_kl(self, observer, agent, obs):
        """mean KL(softmax(actor_agent) || softmax(approximator)) over the rows of obs"""
        lp = torch.log_softmax(self.actor_logits(agent, obs).double(), -1)
        lq = torch.log_softmax(self.approx_logits(observer, agent, obs).double(), -1)
        return float((lp.exp() * (lp - lq)).sum(-1).mean())

    def approx_quality(self, idx=None):
        """How well the approximators fit on replay rows idx (None: a fresh draw of
        batch_size rows that leaves the training index stream where it was).  Per
        pair (observer, agent): the mean cross-entropy of the replayed actions
        under the approximator ("ce"), under the agent's own policy ("ce_true") and
        the mean KL(policy || approximator) ("kl"); plus the means over all pairs."""
        if idx is None:
            st = self.get_rng_state()
            idx = self.make_index(self.batch_size)
            self.set_rng_state(st)
        rows = self.sample_rows(idx.to(self.device, torch.int32))
        self.sync_out()
        A = _lib.ACT_DIM
        pairs = {}
        for i, j in self.approx_pairs():
            lay, w = self.row_layout[j], self.act_dims[j]
            obs = rows[:, lay[0]:lay[0] + self.obs_dims[j]].contiguous()
            act = rows[:, lay[1]:lay[1] + A][:, :w].double()
            lq = torch.log_softmax(self.approx_logits(i, j, obs).double(), -1)
            lp = torch.log_softmax(self.actor_logits(j, obs).double(), -1)
            pairs[(i, j)] = dict(ce=float(-(act * lq).sum(-1).mean()), ce_true=float(-(act * lp).sum(-1).mean()),
                                 kl=float((lp.exp() * (lp - lq)).sum(-1).mean()))
        out = dict(pairs=pairs)
        for k in ("ce", "ce_true", "kl"):
            out["mean_" + k] = float(np.mean([v[k] for v in pairs.values()])) if pairs else float("nan")
        return out

    APPROX_REGIONS = ("net", "target", "adam_m", "adam_v", "grad")

    def approx_region(self, observer, name):
        """float32 view of one of observer's five param-space regions in the
        approximator buffer (APPROX_REGIONS), laid out as the arena's regions:
        its approximator of agent j lies in agent j's actor span"""
        if not self.approx:
            raise _lib.MdpError("approx_region: inferred policies are not enabled")
        stride = (4 * self.param_floats + 255) // 256 * 256
        k = 5 * observer + self.APPROX_REGIONS.index(name)
        return self.approx_buf[k * stride: k * stride + 4 * self.param_floats].view(torch.float32)

    TD3_REGIONS = ("theta2", "target2", "adam_m2", "adam_v2", "grad2")

    def td3_region(self, name):
        """float32 view of one of the second critic's param-space regions in the TD3
        buffer (the arena regions' offsets: mdp_tensor(agent, 1, t).offset)"""
        if not self.td3:
            raise _lib.MdpError("td3_region: MATD3 is not enabled")
        stride = (4 * self.param_floats + 255) // 256 * 256
        k = self.TD3_REGIONS.index(name)
        return self.td3_buf[k * stride: k * stride + 4 * self.param_floats].view(torch.float32)

    def td3_info(self, agent):
        """{critic_updates, actor_updates, q_loss, q_loss2} of agent's last update (mdp_td3_info)"""
        out = (ctypes.c_double * 4)()
        self._c("mdp_td3_info", int(agent), out)
        return {"critic_updates": int(out[0]), "actor_updates": int(out[1]), "q_loss": np.float32(out[2]),
                "q_loss2": np.float32(out[3])}

    def per_sample(self, agent, count, u=None):
        """(positions int32 [count], IS weights float32 [count]) from agent's tree:
        the stratified draw with injected uniforms u or the device Philox
        (mdp_per_sample; advances the agent's beta and sample counter)"""
        count = int(count)
        self._sized("u", u, count)
        u = None if u is None else u.to(self.device, torch.float32).contiguous()
        idx = torch.empty(count, dtype=torch.int32, device=self.device)
        w = torch.empty(count, dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_per_sample", int(agent), count, self._ptr(u), self._ptr(idx), self._ptr(w))
        self._keep = (u, idx, w)
        self.sync_out()
        return idx, w

    def _per_write(self, name, agent, pos, val):
        pos = torch.as_tensor(pos).to(self.device, torch.int32).contiguous().reshape(-1)
        val = torch.as_tensor(val).to(self.device, torch.float32).contiguous().reshape(-1)
        self._sized("values", val, pos.numel())
        self.sync_in()
        self._c(name, int(agent), self._ptr(pos), self._ptr(val), pos.numel())
        self._keep = (pos, val)
        self.sync_out()

    def per_set_priorities(self, agent, pos, p):
        """leaves of ring positions pos <- raw priorities p (mdp_per_set_priorities)"""
        self._per_write("mdp_per_set_priorities", agent, pos, p)

    def per_update_errors(self, agent, pos, abs_err):
        """leaves of pos <- min(|err| + eps, upper) ** alpha (mdp_per_update_errors)"""
        self._per_write("mdp_per_update_errors", agent, pos, abs_err)

    def per_tree(self, agent):
        """agent's tree [2 P, 2] float32 {sum, min}: node 1 the root, node P + i ring
        position i, brought up to date with the ring first (mdp_per_get_tree)"""
        if not self.prioritized:
            raise _lib.MdpError("per_tree: prioritized replay is not enabled")
        out = np.empty((self.per_nodes, 2), np.float32)
        self._c("mdp_per_get_tree", int(agent), _lib.fptr(out))
        return out

    def per_info(self, agent):
        out = (ctypes.c_double * 5)()
        self._c("mdp_per_info", int(agent), out)
        return {"beta": np.float32(out[0]), "total": np.float32(out[1]), "p_min": np.float32(out[2]),
                "rows_synced": int(out[3]), "samples": int(out[4])}

    def per_slots(self, agent):
        """(idx int32, weights, |TD errors|) views [B] of agent's slots of the last update"""
        off = (ctypes.c_int64 * 3)()
        self._c("mdp_per_slots", int(agent), off)
        sl = lambda k, dt: self.per_buf[off[k]: off[k] + 4 * self.batch_size].view(dt)
        return sl(0, torch.int32), sl(1, torch.float32), sl(2, torch.float32)

    # ------------------------------------------------------------ policies
    def act(self, agent, obs, target=False, u=None):
        """[rows, A_i] Gumbel-softmax samples (a Box(d_i) agent: [rows, d_i] Gaussian
        samples); u: injected uniforms [rows, A_i] (Box: [rows, 2]) or [rows, 5]"""
        obs = obs.to(self.device, torch.float32).contiguous()
        out = torch.empty((obs.shape[0], _lib.ACT_DIM), dtype=torch.float32, device=self.device)
        if u is not None:
            u = u.to(self.device, torch.float32)
            u = (self.pad_noise(agent, u) if self.is_box(agent) else self.pad_act(agent, u)).contiguous()
            self._sized("u", u, obs.shape[0] * _lib.ACT_DIM)
        self.sync_in()
        self._c("mdp_act", agent, 1 if target else 0, self._ptr(obs), self._ptr(out), obs.shape[0], self._ptr(u))
        self.sync_out()
        return self._narrow(agent, out)

    def _narrow(self, agent, out):
        w = self.act_dims[agent]
        return out if w == _lib.ACT_DIM else out[:, :w].contiguous()

    def actor_logits(self, agent, obs, target=False):
        obs = obs.to(self.device, torch.float32).contiguous()
        out = torch.empty((obs.shape[0], _lib.ACT_DIM), dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_actor_logits", agent, 1 if target else 0, self._ptr(obs), self._ptr(out), obs.shape[0])
        self.sync_out()
        w = self.head_dim(agent)    # a Box agent: flat = [mean | logstd]
        return out if w == _lib.ACT_DIM else out[:, :w].contiguous()

    def q_values(self, agent, x, target=False):
        """x: the critic input in its logical width (A_j columns per action), or in
        the device's (5 per action, pad columns zero)"""
        x = x.to(self.device, torch.float32)
        cols = self.cin_columns(agent)
        dev_w = self._tensors[(agent, 1)][0][3]
        if x.shape[1] != dev_w:
            if x.shape[1] != len(cols):
                raise ValueError(f"critic input of agent {agent} is {len(cols)} wide, got {x.shape[1]}")
            xd = x.new_zeros((x.shape[0], dev_w))
            xd[:, cols] = x
            x = xd
        x = x.contiguous()
        out = torch.empty(x.shape[0], dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_q_values", agent, 1 if target else 0, self._ptr(x), self._ptr(out), x.shape[0])
        self.sync_out()
        return out

    # ------------------------------------------------------------ training
    @staticmethod
    def _sized(what, t, want):
        """the C side reads exactly `want` elements of an injected index / noise
        tensor: a short one would be an out-of-bounds device read, so refuse it"""
        if t is not None and t.numel() != want:
            raise ValueError(f"{what}: {t.numel()} elements, the update reads {want}")

    def update(self, agent, idx=None, u_tgt=None, u_act=None):
        B, n, A = self.batch_size, self.n, _lib.ACT_DIM
        self._sized("idx", idx, B)
        self._sized("u_tgt", u_tgt, n * B * A)
        self._sized("u_act", u_act, B * A)
        args = []
        for t, dt in ((idx, torch.int32), (u_tgt, torch.float32), (u_act, torch.float32)):
            args.append(None if t is None else t.to(self.device, dt).contiguous())
        self.sync_in()
        self._c("mdp_update", agent, *[self._ptr(a) for a in args])
        self._keep = args
        self.sync_out()

    UPDATE_MODES = {"strict": 0, "throughput": 1}

    def set_update_mode(self, mode):
        """'strict' (the reference's order, default) or 'throughput' (every
        agent's gradients from the round-start parameters, then every optimizer
        step: SURVEY.md 8e, not the reference's semantics).  mdp_set_update_mode."""
        self._c("mdp_set_update_mode", self.UPDATE_MODES[mode])
        self.update_mode = mode

    def update_all(self, idx=None, u_tgt=None, u_act=None):
        """one throughput-mode round; idx [n, B], u_tgt [n, n, B, 5], u_act [n, B, 5]
        (injected randomness for parity; None: device streams).  mdp_update_all."""
        B, n, A = self.batch_size, self.n, _lib.ACT_DIM
        self._sized("idx", idx, n * B)
        self._sized("u_tgt", u_tgt, n * n * B * A)
        self._sized("u_act", u_act, n * B * A)
        args = []
        for t, dt in ((idx, torch.int32), (u_tgt, torch.float32), (u_act, torch.float32)):
            args.append(None if t is None else t.to(self.device, dt).contiguous())
        self.sync_in()
        self._c("mdp_update_all", *[self._ptr(a) for a in args])
        self._keep = args
        self.sync_out()

    def agent_update(self, agent, t, idx=None, u=None):
        """MADDPGAgentTrainer.update(agents, t) in one C call (mdp_agent_update):
        None below the gates (maddpg.py:162-165), else the 6 stats.  u: None or
        [n * B * 5 target-actor uniforms | B * 5 actor-loss uniforms] (flat)."""
        B, n, A = self.batch_size, self.n, _lib.ACT_DIM
        self._sized("idx", idx, B)
        self._sized("u", u, (n + 1) * B * A)
        args = []
        for a, dt in ((idx, torch.int32), (u, torch.float32)):
            args.append(None if a is None else a.to(self.device, dt).contiguous().reshape(-1))
        out = (ctypes.c_double * 6)()
        self.sync_in()
        rc = self._c("mdp_agent_update", int(agent), int(t), *[self._ptr(a) for a in args], out)
        self._keep = args
        self.sync_out()
        return None if rc == 1 else update_stats(out)

    def update_gate(self, t):
        return self._c("mdp_update_gate", int(t))

    def update_round(self):
        self._c("mdp_update_round")

    def train_step(self, rounds):
        """one vector env step + `rounds` update rounds, as one graph replay
        (mdp_train_step; single-GPU path)."""
        self._c("mdp_train_step", int(rounds))

    def train_steps(self, rounds, launch=True):
        """len(rounds) consecutive vector steps (step i: rollout + rounds[i] update
        rounds) as ONE graph replay (mdp_train_steps); launch=False only
        captures and instantiates that graph ahead of time."""
        ks = (ctypes.c_int32 * len(rounds))(*[int(k) for k in rounds])
        self._c("mdp_train_steps", len(rounds), ks, 1 if launch else 0)

    def dp_init(self, world, rank, uid=None):
        """Native data parallelism: join an RCCL communicator of `world` ranks
        (mdp_dp_init).  `uid` (128 bytes) comes from rank 0's dp_unique_id();
        with torch.distributed initialised, dp_init_from_dist() shares it."""
        if uid is None:
            uid = Engine.dp_unique_id()
        self._c("mdp_dp_init", bytes(uid), int(world), int(rank))

    @staticmethod
    def dp_unique_id():
        buf = ctypes.create_string_buffer(128)
        if _lib.load().mdp_dp_unique_id(buf) != 0:
            raise _lib.MdpError("mdp_dp_unique_id failed (librccl.so.1 not loadable?)")
        return buf.raw

    def dp_init_from_dist(self, world, rank):
        """rank 0 makes the RCCL id, torch.distributed broadcasts it, every rank
        joins; returns False on every rank if rank 0 could not make one."""
        import torch.distributed as dist
        obj = [None]
        if rank == 0:
            try:
                obj[0] = Engine.dp_unique_id()
            except Exception:
                obj[0] = None
        dist.broadcast_object_list(obj, src=0)
        if obj[0] is None:
            return False
        self.dp_init(world, rank, obj[0])
        return True

    def dp_xgmi_open(self, world, rank):
        """export this rank's exchange buffer; returns its 64-byte IPC handle"""
        buf = ctypes.create_string_buffer(64)
        self._c("mdp_dp_xgmi_open", int(world), int(rank), buf)
        return buf.raw

    def dp_xgmi_connect(self, handles):
        self._c("mdp_dp_xgmi_connect", b"".join(bytes(x) for x in handles))

    def dp_xgmi_probe(self):
        bad = ctypes.c_int32(0)
        self._c("mdp_dp_xgmi_probe", ctypes.byref(bad))
        return bad.value

    def dp_xgmi_init_from_dist(self, world, rank):
        """Direct xGMI gradient exchange (mdp_dp_xgmi_*): the handshake of
        parallel.xgmi_handshake over torch.distributed.  Returns False
        (everything torn down on every rank) when any rank failed, so the
        caller can fall back to dp_init_from_dist."""
        from .parallel import xgmi_handshake
        eng = self

        class _Ops:
            device = eng.device
            open = staticmethod(eng.dp_xgmi_open)
            connect = staticmethod(eng.dp_xgmi_connect)
            probe = staticmethod(eng.dp_xgmi_probe)

            @staticmethod
            def enable():
                eng._c("mdp_dp_xgmi_enable")

            @staticmethod
            def close():
                eng._c("mdp_dp_xgmi_close")

        ok, err = xgmi_handshake(_Ops, world, rank)
        if not ok and err is not None:
            import sys
            print(f"[rank {rank}] xGMI exchange unavailable ({err}); using RCCL", file=sys.stderr)
        return ok

    DP_KINDS = {0: None, 1: "rccl", 2: "xgmi"}

    def dp_info(self):
        """{kind, ranks, rank, peers}: the communicator this rank's gradient
        exchange runs over (mdp_dp_info)."""
        out = (ctypes.c_int32 * 4)()
        self._c("mdp_dp_info", out)
        return {"kind": self.DP_KINDS[out[0]], "ranks": out[1], "rank": out[2], "peers": out[3]}

    def dp_exchange_stats(self, reset=False):
        """direct xGMI exchange wait of this rank's chunk workgroups since the
        last reset (mdp_dp_exchange_stats): {chunk_exchanges, mean_us, max_us,
        total_us}."""
        out = (ctypes.c_double * 4)()
        self._c("mdp_dp_exchange_stats", out, 1 if reset else 0)
        return {"chunk_exchanges": int(out[0]), "mean_us": out[1], "max_us": out[2], "total_us": out[3]}

    def dp_exchange_stats_enable(self, on=True):
        """stamp the xGMI exchange waits in the optimizer launches issued while
        enabled (mdp_dp_exchange_stats_enable; default off)"""
        self._c("mdp_dp_exchange_stats_enable", 1 if on else 0)

    def param_checksum(self):
        """exact fingerprint of every replicated state region (weights, targets,
        Adam moments, beta powers): int64 sums of the raw 32-bit words, plus a
        position-weighted sum so permutations differ"""
        out = []
        for name in ("theta", "target", "adam_m", "adam_v", "beta"):
            w = self.region(name, torch.int32).to(torch.int64)
            pos = torch.arange(1, w.numel() + 1, device=w.device, dtype=torch.int64)
            out += [int(w.sum().item()), int(((w & 0xFFFF) * pos).sum().item())]
        return out

    def set_graphs(self, on=True):
        """hipGraph replay of update_round (default on; per-kernel profiling runs eager)."""
        self._c("mdp_set_graphs", 1 if on else 0)

    def critic_grad(self, agent, idx, u_tgt=None):
        B, n, A = self.batch_size, self.n, _lib.ACT_DIM
        self._sized("idx", idx, B)
        self._sized("u_tgt", u_tgt, n * B * A)
        idx = idx.to(self.device, torch.int32).contiguous()
        u_tgt = None if u_tgt is None else u_tgt.to(self.device, torch.float32).contiguous()
        self._c("mdp_critic_grad", agent, self._ptr(idx), self._ptr(u_tgt))
        self._keep = (idx, u_tgt)

    def actor_grad(self, agent, idx, u_act=None):
        B, A = self.batch_size, _lib.ACT_DIM
        self._sized("idx", idx, B)
        self._sized("u_act", u_act, B * A)
        idx = idx.to(self.device, torch.int32).contiguous()
        u_act = None if u_act is None else u_act.to(self.device, torch.float32).contiguous()
        self._c("mdp_actor_grad", agent, self._ptr(idx), self._ptr(u_act))
        self._keep = (idx, u_act)

    def reduce_grad(self, agent, net):
        self._c("mdp_reduce_grad", agent, net)

    def apply_grad(self, agent, net, scale=1.0):
        self._c("mdp_apply_grad", agent, net, float(scale))

    def index_slot(self, agent):
        """int32 view of the device index slot used by agent's update this round."""
        return self.region("index", torch.int32)[agent * self.batch_size:(agent + 1) * self.batch_size]

    def stats(self, agent):
        out = (ctypes.c_double * 6)()
        self._c("mdp_get_stats", agent, out)
        return list(out)

    def check_finite(self):
        """NaN / Inf values in every parameter set (weights, targets, Adam m, v)
        and in the agents' update stats, counted on the device (mdp_check_finite:
        the reference's opt-in check_nan, tf_util.py:322,366-368)"""
        out = ctypes.c_int64()
        self._c("mdp_check_finite", ctypes.byref(out))
        return int(out.value)

    def stats_future(self, agent):
        """Snapshot of agent's 6 update stats, copied D2H in stream order (no sync);
        returns (host tensor, event) -- wait on the event before reading."""
        src = self.region("stats", torch.float64)[agent * 8:agent * 8 + 6]
        dst = torch.empty(6, dtype=torch.float64, pin_memory=True)
        with torch.cuda.stream(self.stream):
            dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return dst, ev

    # ----------------------------------------------------------------- env
    @property
    def n_entities(self):
        """agents + landmarks (scenario make_world)."""
        landmarks = {"simple": 1, "simple_spread": self.n, "simple_adversary": self.n - 1,
                     "simple_tag": 2, "simple_speaker_listener": 3}.get(self.scenario, 0)
        return self.n + landmarks

    def env_reset(self):
        self._c("mdp_env_reset")

    def env_step(self, act_in=None, u=None):
        """act_in / u: [E, n, 5] injected actions / uniforms (a narrower agent's pad
        entries of act_in must be zero: pad_act)"""
        a = None if act_in is None else act_in.to(self.device, torch.float32).contiguous()
        uu = None if u is None else u.to(self.device, torch.float32).contiguous()
        self._sized("act_in", a, self.num_envs * self.n * _lib.ACT_DIM)
        self._sized("u", uu, self.num_envs * self.n * _lib.ACT_DIM)
        if a is not None or uu is not None:
            self.sync_in()
        self._c("mdp_env_step", self._ptr(a), self._ptr(uu))
        if a is not None or uu is not None:
            self._keep = (a, uu)
            self.sync_out()

    def env_step_bench(self, out=None, u=None):
        """one vector env step (policy actions) that also returns every agent's
        scenario benchmark_data() record, [E, n, BENCH_W] float32 on the device
        (mdp_env_step_bench; --benchmark mode, train.py:139-141).  u: [E, n, 5]
        injected Gumbel uniforms, as env_step's."""
        if out is None:
            out = torch.empty((self.num_envs, self.n, _lib.BENCH_W), dtype=torch.float32, device=self.device)
        if u is None:
            self._c("mdp_env_step_bench", self._ptr(out))
        else:
            uu = u.to(self.device, torch.float32).contiguous()
            self._sized("u", uu, self.num_envs * self.n * _lib.ACT_DIM)
            self.sync_in()
            self._c("mdp_env_step_bench_u", self._ptr(out), self._ptr(uu))
            self._keep = (uu,)
        self.sync_out()
        return out

    # ---------------------------------------------------------- evaluation
    def evaluate(self, episodes, first_episode=0, mode="sample", bench=False, u=None):
        """Score the current actors on evaluation episodes [first_episode,
        first_episode + episodes) (mdp_evaluate): whole episodes on the device,
        nothing training uses is read or written.  An id's result depends only
        on the actor parameters, the seed, the scenario, the id and the mode.
        mode "sample": the reference's act; "mean": the softmax of the logits
        without noise.  u: [episodes, max_episode_len, n, 5] injected uniforms
        (sample mode).  Returns a dict: `returns` [episodes, n] float32 device
        tensor, `bench` [episodes, n, BENCH_W] record sums or None, `summary`
        per-agent mean / population std / min / max of the returns in fp64."""
        if mode not in _lib.EVAL_MODE:
            raise ValueError(f"unknown evaluation mode {mode!r} (sample, mean)")
        episodes, first_episode = int(episodes), int(first_episode)
        uu = None if u is None else u.to(self.device, torch.float32).contiguous()
        self._sized("u", uu, episodes * self.max_episode_len * self.n * _lib.ACT_DIM)
        ret = torch.empty((max(episodes, 0), self.n), dtype=torch.float32, device=self.device)
        rec = None
        if bench:
            rec = torch.empty((max(episodes, 0), self.n, _lib.BENCH_W), dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_evaluate", first_episode, episodes, _lib.EVAL_MODE[mode], self._ptr(uu), self._ptr(ret),
                self._ptr(rec))
        self._keep = (uu,)
        self.sync_out()
        r64 = ret.double()
        summary = {"mean": r64.mean(0).tolist(), "std": r64.std(0, unbiased=False).tolist(),
                   "min": r64.min(0).values.tolist(), "max": r64.max(0).values.tolist()}
        return {"returns": ret, "bench": rec, "summary": summary}

    def eval_q_window(self, scored=None, tail=0.01):
        """the default (steps, scored) of evaluate_q: scored = max_episode_len,
        steps = scored + the smallest W with gamma^W <= tail (90 at gamma 0.95),
        inside the call's step limit"""
        scored = self.max_episode_len if scored is None else int(scored)
        gamma, w = float(self.cfg.gamma), 1
        while gamma ** w > tail and scored + w < _lib.EVAL_Q_MAX_STEPS:
            w += 1
        return scored + w, scored

    def evaluate_q(self, episodes, steps=None, scored=None, first_episode=0, mode="sample", u=None):
        """Score the live critics against the returns their policies then collect
        (mdp_evaluate_q): evaluate's episode ids, played `steps` steps without
        reset -- the reference never stores done = 1 for these scenarios, so a
        critic estimates the continuing world's return -- with Q_j(o_t, a_t) of
        every agent's critic (and its twin on a td3 engine: C = 2) taken in the
        same launch.  The first `scored` steps are compared: their returns-to-go
        lack at most a factor gamma^(steps - scored + 1) of the return's scale.
        scored defaults to max_episode_len, steps to eval_q_window()'s.  u:
        [episodes, steps, n, 5] injected uniforms (sample mode).  Nothing training
        uses is read or written.  Returns a dict of float32 device tensors `q`
        [episodes, steps, n, C], `rew` and `g` [episodes, steps, n] (step rewards;
        return-to-go, formed in fp64), `gap` [episodes, n, C] (mean over the
        scored steps of q - g), `steps`, `scored`, and `summary`: per agent and
        critic ([n][C] lists, fp64) `q_mean` and `g_mean` over episodes and scored
        steps, `gap_mean`, `gap_rms` (over episodes), and `truncation`."""
        if mode not in _lib.EVAL_MODE:
            raise ValueError(f"unknown evaluation mode {mode!r} (sample, mean)")
        episodes, first_episode = int(episodes), int(first_episode)
        if scored is None:
            scored = self.max_episode_len if steps is None else min(self.max_episode_len, int(steps))
        if steps is None:
            steps = self.eval_q_window(scored)[0]
        steps, scored = int(steps), int(scored)
        C = 2 if self.td3 else 1
        ne, ns = max(episodes, 0), max(steps, 0)
        uu = None if u is None else u.to(self.device, torch.float32).contiguous()
        self._sized("u", uu, ne * ns * self.n * _lib.ACT_DIM)
        q = torch.empty((ne, ns, self.n, C), dtype=torch.float32, device=self.device)
        rew = torch.empty((ne, ns, self.n), dtype=torch.float32, device=self.device)
        g = torch.empty((ne, ns, self.n), dtype=torch.float32, device=self.device)
        gap = torch.empty((ne, self.n, C), dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_evaluate_q", first_episode, episodes, _lib.EVAL_MODE[mode], steps, scored, self._ptr(uu),
                self._ptr(q), self._ptr(rew), self._ptr(g), self._ptr(gap))
        self._keep = (uu,)
        self.sync_out()
        gap64 = gap.double()
        g_mean = g[:, :scored].double().mean((0, 1))
        summary = {"q_mean": q[:, :scored].double().mean((0, 1)).tolist(),
                   "g_mean": [[v] * C for v in g_mean.tolist()],
                   "gap_mean": gap64.mean(0).tolist(),
                   "gap_rms": gap64.pow(2).mean(0).sqrt().tolist(),
                   "truncation": float(self.cfg.gamma) ** (steps - scored + 1)}
        return {"q": q, "rew": rew, "g": g, "gap": gap, "steps": steps, "scored": scored, "summary": summary}

    def eval_initial_state(self, episodes, first_episode=0):
        """start states of those evaluation ids (mdp_eval_initial_state): pos / vel
        [episodes, n_entities, 2] float32, goal [episodes] int32 (host arrays)"""
        episodes, ne = int(episodes), self.n_entities
        pos = np.empty((max(episodes, 0), ne, 2), np.float32)
        vel = np.empty((max(episodes, 0), ne, 2), np.float32)
        goal = np.empty(max(episodes, 0), np.int32)
        self._c("mdp_eval_initial_state", int(first_episode), episodes, _lib.fptr(pos), _lib.fptr(vel),
                goal.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        return {"pos": pos, "vel": vel, "goal": goal}

    # ------------------------------------------------- matchup evaluation
    def actor_set_floats(self):
        """floats of one actor set, the stride of a bank (mdp_actor_set_floats)"""
        v = int(self.lib.mdp_actor_set_floats(self.h))
        if v < 0:
            raise _lib.MdpError("mdp_actor_set_floats: unusable handle")
        return v

    def actor_bank(self, n_sets):
        """a zero-filled bank of `n_sets` actor sets: float32 device tensor
        [n_sets, set_floats], each set laid out as the theta region (agent j's
        actor tensor t at mdp_tensor(j, 0, t).offset)"""
        n_sets = int(n_sets)
        if not 1 <= n_sets <= _lib.EVAL_MAX_SETS:
            raise ValueError(f"actor_bank: 1 <= n_sets <= {_lib.EVAL_MAX_SETS}, got {n_sets}")
        return torch.zeros((n_sets, self.actor_set_floats()), dtype=torch.float32, device=self.device)

    def _bank_slot(self, bank, k):
        sf = self.actor_set_floats()
        if (not isinstance(bank, torch.Tensor) or bank.dtype != torch.float32 or bank.device != self.device
                or not bank.is_contiguous()):
            raise ValueError("bank: a contiguous float32 tensor on the engine's device (actor_bank)")
        if bank.numel() == 0 or bank.numel() % sf:
            raise ValueError(f"bank: {bank.numel()} elements, a set has {sf}")
        k = int(k)
        if not 0 <= k < bank.numel() // sf:
            raise ValueError(f"bank slot {k} out of range for {bank.numel() // sf} sets")
        return bank.view(-1, sf)[k]

    def bank_snapshot(self, bank, k):
        """copy the handle's current actors into slot k of the bank (mdp_actor_set_snapshot)"""
        slot = self._bank_slot(bank, k)
        self.sync_in()
        self._c("mdp_actor_set_snapshot", self._ptr(slot))
        self.sync_out()

    def bank_write(self, bank, k, source, agents=None):
        """write actors into slot k of the bank: `source` is a state_dict()-style
        dict or a checkpoint path (npz or TF1 bundle, read as load_state reads
        it); agents: only these agents' actors (None: every agent).  The
        handle's own parameters are not touched (mdp_actor_set_write)."""
        slot = self._bank_slot(bank, k)
        sd = source
        if not isinstance(source, dict):
            sd = read_checkpoint(source, self.checkpoint_path(source), self.n, self.SETS)[0]
        todo = range(self.n) if agents is None else sorted({int(a) for a in agents})
        flats = []
        for i in todo:
            if not 0 <= i < self.n:
                raise ValueError(f"agent {i} out of range for {self.n} agents")
            flats.append((i, self._flat_params(i, "actor", {t: sd[f"agent_{i}/actor/{t}"] for t in TENSOR_NAMES})))
        self.sync_in()
        for i, flat in flats:
            self._c("mdp_actor_set_write", self._ptr(slot), i, _lib.fptr(flat), flat.size)
        self.sync_out()

    def evaluate_matchups(self, bank, table, episodes, first_episode=0, mode="sample", bench=False, u=None):
        """Score every row of a matchup table on evaluation episodes
        [first_episode, first_episode + episodes) in one launch
        (mdp_evaluate_matchups).  table [M, n] int32: table[m][j] is the set of
        `bank` that agent j's actor comes from.  Episodes are mdp_evaluate's:
        start state and noise depend on the id alone, so matchups on the same
        ids are paired on common random numbers.  The handle's parameters are
        neither read nor written.  u: [episodes, max_episode_len, n, 5]
        injected uniforms shared by every matchup (sample mode).  Returns a
        dict: `returns` [M, episodes, n] float32 device tensor, `bench`
        [M, episodes, n, BENCH_W] or None, `summary` per-matchup, per-agent
        mean / population std / standard error of the returns in fp64."""
        if mode not in _lib.EVAL_MODE:
            raise ValueError(f"unknown evaluation mode {mode!r} (sample, mean)")
        episodes, first_episode = int(episodes), int(first_episode)
        sf = self.actor_set_floats()
        if (not isinstance(bank, torch.Tensor) or bank.dtype != torch.float32 or bank.device != self.device
                or not bank.is_contiguous()):
            raise ValueError("bank: a contiguous float32 tensor on the engine's device (actor_bank)")
        n_sets = bank.numel() // sf
        self._sized("bank", bank, max(n_sets, 1) * sf)
        tab = table.cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
        if tab.dtype != np.int32:
            raise ValueError(f"table: dtype {tab.dtype}, the call reads int32")
        if tab.ndim != 2 or tab.shape[1] != self.n or tab.shape[0] < 1:
            raise ValueError(f"table: shape {tab.shape}, expected [matchups, {self.n}]")
        tab = np.ascontiguousarray(tab)
        M = tab.shape[0]
        uu = None if u is None else u.to(self.device, torch.float32).contiguous()
        self._sized("u", uu, episodes * self.max_episode_len * self.n * _lib.ACT_DIM)
        ne = max(episodes, 0)
        ret = torch.empty((M, ne, self.n), dtype=torch.float32, device=self.device)
        rec = None
        if bench:
            rec = torch.empty((M, ne, self.n, _lib.BENCH_W), dtype=torch.float32, device=self.device)
        self.sync_in()
        self._c("mdp_evaluate_matchups", self._ptr(bank), n_sets, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                M, first_episode, episodes, _lib.EVAL_MODE[mode], self._ptr(uu), self._ptr(ret), self._ptr(rec))
        self.sync_out()
        r64 = ret.double()
        std = r64.std(1, unbiased=False)
        summary = {"mean": r64.mean(1).tolist(), "std": std.tolist(), "sem": (std / ne ** 0.5).tolist()}
        return {"returns": ret, "bench": rec, "summary": summary}

    def cross_play(self, bank, team, episodes, first_episode=0, mode="sample", bench=False, u=None):
        """The K x K cross-play table of a bank of K sets: in cell (a, b) the agents
        in `team` play set a's actors and the others set b's.  One
        evaluate_matchups call (table construction only).  Returns a dict:
        `mean` / `sem` [K, K, n] float64 numpy arrays (per-agent mean return and
        its standard error), `table` [K * K, n], `returns` [K, K, episodes, n]
        and `bench` [K, K, episodes, n, BENCH_W] or None."""
        K = bank.numel() // self.actor_set_floats()
        team = sorted({int(a) for a in team})
        if any(not 0 <= a < self.n for a in team):
            raise ValueError(f"team {team}: agents out of range for {self.n} agents")
        table = np.empty((K, K, self.n), np.int32)
        for j in range(self.n):
            table[:, :, j] = np.arange(K)[:, None] if j in team else np.arange(K)[None, :]
        table = table.reshape(K * K, self.n)
        r = self.evaluate_matchups(bank, table, episodes, first_episode, mode, bench, u)
        shape = (K, K, self.n)
        return {"mean": np.asarray(r["summary"]["mean"], np.float64).reshape(shape),
                "sem": np.asarray(r["summary"]["sem"], np.float64).reshape(shape), "table": table,
                "returns": r["returns"].view(K, K, -1, self.n),
                "bench": None if r["bench"] is None else r["bench"].view(K, K, -1, self.n, _lib.BENCH_W)}

    def env_state(self):
        E, ne = self.num_envs, self.n_entities
        pos = np.empty((E, ne, 2), np.float32)
        vel = np.empty((E, ne, 2), np.float32)
        goal = np.empty(E, np.int32)
        step = np.empty(E, np.int32)
        self._c("mdp_env_get_state", _lib.fptr(pos), _lib.fptr(vel),
                goal.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                step.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        comm = np.empty((E, self.n, _lib.ACT_DIM), np.float32)
        self._c("mdp_env_get_comm", _lib.fptr(comm))
        return {"pos": pos, "vel": vel, "goal": goal, "ep_step": step, "comm": comm}

    def set_env_state(self, pos, vel, goal=None, ep_step=None, comm=None):
        E = self.num_envs
        pos = np.ascontiguousarray(pos, np.float32)
        vel = np.ascontiguousarray(vel, np.float32)
        goal = np.ascontiguousarray(np.zeros(E) if goal is None else goal, np.int32)
        ep_step = np.ascontiguousarray(np.zeros(E) if ep_step is None else ep_step, np.int32)
        self._c("mdp_env_set_state", _lib.fptr(pos), _lib.fptr(vel),
                goal.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                ep_step.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if comm is not None:    # [E, n, 5] state.c (scenarios with a speaking agent)
            comm = np.ascontiguousarray(comm, np.float32)
            assert comm.shape == (E, self.n, _lib.ACT_DIM)
            self._c("mdp_env_set_comm", _lib.fptr(comm))

    def env_obs(self):
        out = torch.empty((self.num_envs, sum(self.obs_dims)), dtype=torch.float32, device=self.device)
        self._c("mdp_env_obs", self._ptr(out))
        self.sync_out()
        return out

    def episode_count(self):
        n = self.lib.mdp_episode_count(self.h)
        if n < 0:
            raise _lib.MdpError("mdp_episode_count failed")
        return int(n)

    def episode_log(self, first, n):
        out = np.empty((n, 1 + self.n), np.float32)
        if n:
            self._c("mdp_episode_log", int(first), int(n), _lib.fptr(out))
        return out

    def replay_rows(self, start, count):
        """float32 view [count, row_stride] of the replay region (no copy)."""
        r = self.region("replay")
        return r[start * self.row_stride:(start + count) * self.row_stride].view(count, self.row_stride)

    # ---------------------------------------------------------- profiling
    @staticmethod
    def _kind(kind):
        for table in (_lib.KERNEL, _lib.KERNEL_PER, _lib.KERNEL_EVAL):
            if kind in table:
                return table[kind]
        raise KeyError(kind)

    def prof_enable(self, kind, on=True):
        self._c("mdp_prof_enable", self._kind(kind), 1 if on else 0)

    def prof_read(self, kind):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._c("mdp_prof_read", self._kind(kind), ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value
