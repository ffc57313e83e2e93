"""Helpers of the policy-evaluation tests: the cases, and the existing step chain
that an evaluation episode must reproduce.

The chain is engine B of tests/test_eval_gpu.py: a handle with one env copy per
evaluation id whose env state is set to the ids' start states and which then
takes max_episode_len vector steps (mdp_env_step, k_rollout).  Its episode log
holds what the evaluation kernel must return.
"""
import numpy as np

ACT = 5
T = 5             # max_episode_len of every evaluation test
PSEED = 11        # init_params seed: engines built with it hold the same parameters
RESET_STREAM = 0x60000
NOISE_STREAM = 0x70000

# name -> (scenario, agents, adversaries in the world, local_q, num_units)
CASES = {
    "simple": ("simple", 1, 0, None, 64),
    "spread3": ("simple_spread", 3, 0, None, 64),
    "adversary_ddpg": ("simple_adversary", 3, 1, [True, False, False], 64),   # a DDPG adversary
    "tag": ("simple_tag", 4, 3, None, 64),                    # contacts, max_speed
    "speaker_listener": ("simple_speaker_listener", 2, 0, None, 64),   # the message across steps, widths 3 / 5
    "spread5": ("simple_spread", 5, 0, None, 64),             # more than 4 agents: the per-agent tile forward
    "spread3_h128": ("simple_spread", 3, 0, None, 128),       # the general path
}
BENCH_CASES = ("spread3", "adversary_ddpg", "tag")


def case_spec(case):
    from maddpg_amd.envs import spec
    name, n, na, _lq, _h = CASES[case]
    if name in ("simple", "simple_speaker_listener"):
        return spec(name)
    return spec(name, n, na if na else None)


def make_engine(case, num_envs, seed, **kw):
    from maddpg_amd.engine import Engine
    name, _n, _na, local_q, H = CASES[case]
    sp = case_spec(case)
    kw.setdefault("batch_size", 16)
    kw.setdefault("capacity", 1024)
    eng = Engine(sp.obs_dims, local_q, num_units=H, num_envs=num_envs, scenario=name,
                 num_adversaries=sp.num_adversaries, max_episode_len=T, seed=seed, **kw)
    eng.init_params(PSEED)
    return eng


def noise(seed, n, ids):
    """[len(ids), T, n, 5]: the uniforms evaluation id g draws at step t for agent j"""
    from oracle import philox
    ids = np.asarray(ids)
    u = np.empty((len(ids), T, n, ACT), np.float32)
    for t in range(T):
        for j in range(n):
            u[:, t, j] = philox.uniforms5(seed, NOISE_STREAM | j, t, ids)
    return u


def chain(case, seed, start, step):
    """Engine B: one env copy per id from the start states `start`, T vector steps.
    step(eng, t) performs vector step t (and may collect what it needs).  Returns the
    per-agent returns [E, n] of the episode log."""
    E = len(start["goal"])
    eng = make_engine(case, E, seed)
    eng.set_env_state(start["pos"], start["vel"], start["goal"])
    for t in range(T):
        step(eng, t)
    eng.synchronize()
    assert eng.episode_count() == E
    return eng.episode_log(0, E)[:, 1:].copy()


def host_actions(eng, fn):
    """[E, n, 5] actions fn(j, logits_j) of every agent on the current observations,
    padded to the device's slot width"""
    import torch
    obs = eng.env_obs()
    out = np.zeros((eng.num_envs, eng.n, ACT), np.float32)
    off = 0
    for j, o in enumerate(eng.obs_dims):
        logits = eng.actor_logits(j, obs[:, off:off + o].contiguous()).cpu().numpy()
        a = fn(j, logits)
        out[:, j, :a.shape[1]] = a
        off += o
    return torch.from_numpy(out)


def slab_unwritten_lanes(eng):
    """Byte mask over the "slab" region of the lanes no run determines.  The strict
    round's critic launch leaves agent i's precomputed actor forward there, one
    144-float row per batch row: h1 [64] | h2 [64] | logits [8] | sample [8].  Of
    the two 8-float groups only 5 entries exist; lanes 5..7 are stored from
    whatever the workgroup's LDS held before and are never read.  Two identical
    training runs already differ in them, so a bit-for-bit comparison of the region
    leaves exactly these 6 floats per row out -- and nothing else.  The offset of
    the rows follows mdp_create's carve of the region."""
    import ctypes
    import torch
    from maddpg_amd import _lib
    off, nb = ctypes.c_int64(), ctypes.c_int64()
    eng._c("mdp_region", _lib.REGION["slab"], ctypes.byref(off), ctypes.byref(nb))
    n, nwg = eng.n, (eng.batch_size + 15) // 16
    slab_c = max(eng.grad_view(i, 1).numel() for i in range(n))
    slab_a = max(eng.grad_view(i, 0).numel() for i in range(n))
    base = eng.arena.data_ptr() + off.value
    p = base + 4 * n * nwg * (slab_c + slab_a)
    p = (p + 7) & ~7
    p += 2 * 8 * 8 * n * nwg                       # the critic's and the actor's per-workgroup stats
    p += 8 * n * eng.batch_size + 256              # TD targets
    p = (p + 255) & ~255
    p += 8 * 2 * 8 * 128 + 8 * 2 * 6 * 256 * 16    # the fused optimizer step's sync area (mdp_ra_sync_bytes)
    first = (p - base) // 4
    mask = torch.zeros(nb.value // 4, dtype=torch.bool)
    rows = mask[first:first + nwg * 16 * 144].view(nwg * 16, 144)
    rows[:, 133:136] = True
    rows[:, 141:144] = True
    return mask.numpy().repeat(4)


def softmax64(logits):
    z = logits.astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)
