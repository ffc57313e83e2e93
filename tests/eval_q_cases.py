"""Helpers of the critic-evaluation tests (mdp_evaluate_q): the configurations, the
engines, the ids' uniforms over any number of steps, the replay rows of the
existing step chain, and the fp64 references.

The chain is engine B of tests/test_eval_gpu.py: one env copy per evaluation id,
started from the ids' start states and stepped with the ids' uniforms; the rows
it appends to its replay ring hold the critic inputs of every step.  B is built
with max_episode_len = the steps played, so it does not reset on the way: the
evaluation call plays on past the handle's max_episode_len in the same manner.
"""
import numpy as np

from tests import eval_oracle as eo

ACT, T, PSEED = eo.ACT, eo.T, eo.PSEED
SEED = 0x0123456789ABCDEF
FIRST, COUNT = 7, 40          # two full 16-id tiles and a ragged tile of 8
IDS = np.arange(FIRST, FIRST + COUNT)
STEPS = 12                    # the longer run of the trajectory tests (max_episode_len = T = 5)

# eval_oracle's cases and the general path at 256 units
CASES = dict(eo.CASES, spread3_h256=("simple_spread", 3, 0, None, 256))


def case_spec(case):
    from maddpg_amd.envs import spec
    name, n, na, _lq, _h = CASES[case]
    if name in ("simple", "simple_speaker_listener"):
        return spec(name)
    return spec(name, n, na if na else None)


def make_engine(case, num_envs, seed=SEED, max_episode_len=T, **kw):
    from maddpg_amd.engine import Engine
    name, _n, _na, local_q, H = CASES[case]
    sp = case_spec(case)
    kw.setdefault("batch_size", 16)
    kw.setdefault("capacity", 1024)
    eng = Engine(sp.obs_dims, local_q, num_units=H, num_envs=num_envs, scenario=name,
                 num_adversaries=sp.num_adversaries, max_episode_len=max_episode_len, seed=seed, **kw)
    eng.init_params(PSEED)
    return eng


def noise(seed, n, ids, steps):
    """[len(ids), steps, n, 5]: the uniforms evaluation id g draws at step t for agent j"""
    from oracle import philox
    ids = np.asarray(ids)
    u = np.empty((len(ids), steps, n, ACT), np.float32)
    for t in range(steps):
        for j in range(n):
            u[:, t, j] = philox.uniforms5(seed, eo.NOISE_STREAM | j, t, ids)
    return u


def chain_rows(case, start, u):
    """[steps, E, row_stride] float32 (device): the replay rows engine B appends when it
    is stepped from `start` with the uniforms u [E, steps, n, 5]"""
    import torch
    E, steps = u.shape[0], u.shape[1]
    b = make_engine(case, E, max_episode_len=steps, capacity=max(1024, E * steps))
    b.set_env_state(start["pos"], start["vel"], start["goal"])
    for t in range(steps):
        b.env_step(u=torch.from_numpy(u[:, t]))
    b.synchronize()
    assert b.buffer_len() == E * steps
    rows = b.sample_rows(torch.arange(E * steps, dtype=torch.int32))
    return rows.view(steps, E, b.row_stride)


def critic_input(eng, j, rows):
    """agent j's critic input in the device's width from replay rows [R, row_stride]:
    the [obs_n | act_n] prefix, or [obs_j | act_j] for a DDPG critic"""
    import torch
    lay = eng.row_layout[j]
    if eng.local_q[j]:
        o = eng.obs_dims[j]
        return torch.cat([rows[:, lay[0]:lay[0] + o], rows[:, lay[1]:lay[1] + ACT]], 1).contiguous()
    return rows[:, :sum(eng.obs_dims) + ACT * eng.n].contiguous()


def critic64(params, x):
    """oracle/nets.py's forward (mlp_fwd) on the logical input x, every operation in fp64"""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    x = np.asarray(x, np.float64)
    h1 = np.maximum(x @ p["W1"] + p["b1"], 0.0)
    h2 = np.maximum(h1 @ p["W2"] + p["b2"], 0.0)
    return (h2 @ p["W3"].reshape(h2.shape[1], -1) + p["b3"])[:, 0]


def returns64(rew, gamma, scored, q):
    """the fp64 recursion on a returned rew trace [E, steps, n] and the gap of q
    [E, steps, n, C]: (G [E, steps, n] float64, gap [E, n, C] float64)"""
    gam = np.float64(np.float32(gamma))
    E, steps, n = rew.shape
    G = np.zeros((E, steps + 1, n), np.float64)
    for t in range(steps - 1, -1, -1):
        G[:, t] = rew[:, t].astype(np.float64) + gam * G[:, t + 1]
    s = np.zeros((E, n, q.shape[3]), np.float64)
    for t in range(scored):
        s = s + (q[:, t].astype(np.float64) - G[:, t, :, None])
    return G[:, :steps], s / scored
