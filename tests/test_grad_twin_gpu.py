"""Twin critic workgroups (k_critic_grad_r, CriticArgs::twin)
against one workgroup per row tile (MDP_GRAD_TWIN=0).

With twins every critic row tile runs on two workgroups that compute the same
d2, dh1 and activations from the same inputs and then each form half of the
tile's weight-gradient tiles: every slab word is still one MFMA chain in the
same k order with one writer, so nothing the update writes may change by a bit.
Every case below runs the same work on an engine created with the switch unset
and with MDP_GRAD_TWIN=0 and compares theta, targets, Adam m and v, the beta
powers, the reduced gradient and the stats with assert_array_equal.

Batch sizes 16 (one tile: the pair alone), 17 (a second tile with one valid
row), 40 (a ragged last tile) and 256 (16 tiles) on observations [18, 18, 18]
with the last agent a DDPG agent (the act-part tiles of its 23 x 64 W1), and a
single agent [4]; rounds through update_round (critic_post and actor_pre
beside the twins) and agent by agent through update, with and without the
extra workgroups; the prioritized-replay and the narrow-action instantiations;
a step graph; and the cases that must keep one workgroup per tile whatever the
switch says: a batch whose doubled grid has more workgroups than the GPU has
CUs, and throughput mode.
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd.engine import Engine  # noqa: E402
from tests import optimizer_edges as oe  # noqa: E402
from tests.helpers import joint_rows, synthetic_trainer_case  # noqa: E402

F32 = np.float32
DIMS, LOCAL_Q = [18, 18, 18], [False, False, True]
STATE = ("theta", "target", "adam_m", "adam_v", "beta")
SETS = ("actor", "tgt_actor", "m_actor", "v_actor", "critic", "tgt_critic", "m_critic", "v_critic")
TWIN = {"on": {}, "off": {"MDP_GRAD_TWIN": "0"}}
NO_EXTRA = {"MDP_ACTOR_PRE": "0", "MDP_CRITIC_PRE": "0"}
CTL_FAULT_OFFSET = 2572            # Ctl.fault (mdp_topo.h)


@contextlib.contextmanager
def _environ(env):
    """the switches are read at mdp_create: set around the engine's construction only"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check_twin(eng, env):
    """the handle's choice (mdp_grad_twin): two workgroups per row tile unless switched off or
    3 x row tiles + 1 workgroups (both twins, actor_pre, the draw) outnumber the CUs"""
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    fits = 3 * ((eng.batch_size + 15) // 16) + 1 <= cus
    assert eng.lib.mdp_grad_twin(eng.h) == (2 if fits and env.get("MDP_GRAD_TWIN") != "0" else 1)
    assert all(eng.lib.mdp_grad_variant(eng.h, i) == 1 for i in range(eng.n))     # the register kernels


_CASES = {}


def _case(B, dims=DIMS, local_q=LOCAL_Q):
    """tests/optimizer_edges.fused_case (loaded optimizer state), the local-q agents' critics cut
    to their own observation and action; made once per shape and left unchanged"""
    key = (B, tuple(dims), tuple(local_q))
    if key not in _CASES:
        c = oe.fused_case("active", B, seed=11, H=64, dims=dims)
        for i, lq in enumerate(local_q):
            if lq:
                cin = dims[i] + oe.ACT
                p = c["params"][i]
                for w in ("critic", "tgt_critic", "m_critic", "v_critic"):
                    p[w] = dict(p[w], W1=np.ascontiguousarray(p[w]["W1"][:cin]))
        _CASES[key] = c
    return _CASES[key]


def _engine(c, B, env, dims=DIMS, local_q=LOCAL_Q, prof=False, **kw):
    """prof: count the critic launches (a handle that times kernels runs every round eagerly)"""
    with _environ(env):
        eng = Engine(dims, local_q, num_units=64, batch_size=B, capacity=128, **kw)
    _check_twin(eng, env)
    eng.add_rows(torch.from_numpy(joint_rows(c["data"], dims)))
    for i, p in enumerate(c["params"]):
        for w in SETS:
            eng.set_params(i, w, p[w])
        for k in (0, 1):
            eng.set_beta_powers(i, k, np.array(oe.powers_at(50 + 20 * k + i), F32))
    if prof:
        eng.prof_enable("critic_grad")
    return eng


def _snapshot(eng, stats=None, prof=False):
    """everything an update writes, as bits; closes the engine"""
    eng.synchronize()
    torch.cuda.synchronize()
    assert eng.check_finite() == 0
    out = {r: eng.region(r).cpu().numpy().view(np.uint32).copy() for r in STATE}
    grad = eng.region("grad").cpu().numpy().view(np.uint32)
    spans = [(off, dr * dc) for i in range(eng.n) for net in (0, 1) for (off, _r, _c, dr, dc) in eng.net_tensors(i, net)]
    out["grad"] = np.concatenate([grad[o:o + n] for o, n in spans])
    if stats is None:
        stats = [np.array(eng.stats(i), np.float64) for i in range(eng.n)]
    out["stats"] = np.stack(stats).view(np.uint64)
    ctl = eng.region("ctl", torch.uint8).cpu().numpy()
    assert int(ctl[CTL_FAULT_OFFSET:CTL_FAULT_OFFSET + 4].view(np.uint32)[0]) == 0
    if prof:
        out["critic_launches"] = np.array([eng.prof_read("critic_grad")[1]])
    eng.close()
    return out


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _by_agent(c, B, env, dims=DIMS, local_q=LOCAL_Q):
    """one strict round, agent by agent through update (injected indices and noise)"""
    eng = _engine(c, B, env, dims, local_q, prof=True)
    stats = []
    for i in range(eng.n):
        eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                   u_act=torch.from_numpy(c["u_act"][i]))
        stats.append(np.array(eng.stats(i), np.float64))
    return _snapshot(eng, stats, prof=True)


def _rounds(c, B, env, rounds=3):
    """`rounds` strict rounds through update_round (device index draw and noise)"""
    eng = _engine(c, B, env)
    eng.seed_py_random(77)
    for _ in range(rounds):
        eng.update_round()
    return _snapshot(eng)


@pytest.mark.parametrize("B", [16, 17, 40, 256])
def test_update_agent_by_agent(B):
    """1, 2 (the second with one valid row), 3 (ragged) and 16 row tiles; MADDPG and DDPG critics"""
    c = _case(B)
    on, off = _by_agent(c, B, TWIN["on"]), _by_agent(c, B, TWIN["off"])
    assert on["critic_launches"][0] == 3
    _equal(on, off)
    assert np.count_nonzero(on["grad"]) > on["grad"].size // 2


def test_single_agent():
    """one agent with 4 observations: no target-actor split, a 9 x 64 critic W1"""
    B, dims, lq = 40, [4], [False]
    c = _case(B, dims, lq)
    _equal(_by_agent(c, B, TWIN["on"], dims, lq), _by_agent(c, B, TWIN["off"], dims, lq))


@pytest.mark.parametrize("B", [17, 40])
def test_three_update_rounds(B):
    """critic_post and actor_pre beside the twins, the first round eager and the next replayed"""
    c = _case(B)
    _equal(_rounds(c, B, TWIN["on"]), _rounds(c, B, TWIN["off"]))


def test_three_update_rounds_without_extra_workgroups():
    """MDP_ACTOR_PRE=0 MDP_CRITIC_PRE=0: a twin grid with nothing behind the critic workgroups
    but the draw; and equal to the rounds with the extra workgroups"""
    B = 40
    c = _case(B)
    on, off = _rounds(c, B, dict(NO_EXTRA)), _rounds(c, B, dict(NO_EXTRA, **TWIN["off"]))
    _equal(on, off)
    _equal(on, _rounds(c, B, TWIN["on"]))


def test_prioritized_instantiation():
    """the PER kernel on the smallest PER configuration of tests/test_per_gpu.py: |TD errors|,
    weights and the priorities written back from them equal as well"""
    dims, B, L = [8, 10, 10], 40, 300
    c = synthetic_trainer_case(dims, B, L, 21, None, 64)
    res = []
    for env in TWIN.values():
        with _environ(env):
            eng = Engine(dims, c["local_q"], num_units=64, batch_size=B, capacity=L + 7, prioritized=True)
        _check_twin(eng, env)
        eng.add_rows(torch.from_numpy(joint_rows(c["data"], dims)))
        for i, p in enumerate(c["params"]):
            for w in ("actor", "critic", "tgt_actor", "tgt_critic"):
                eng.set_params(i, w, p[w])
        rng = np.random.default_rng(8)
        per = {}
        for i in range(3):
            prio = rng.uniform(0.05, 1.0, L).astype(F32)
            eng.per_set_priorities(i, torch.from_numpy(np.arange(L, dtype=np.int32)), torch.from_numpy(prio))
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                       u_act=torch.from_numpy(c["u_act"][i]))
            s_idx, s_w, s_td = (x.cpu().numpy().copy() for x in eng.per_slots(i))
            per[f"idx{i}"], per[f"w{i}"], per[f"td{i}"] = s_idx, s_w.view(np.uint32), s_td.view(np.uint32)
            per[f"tree{i}"] = np.asarray(eng.per_tree(i), F32).view(np.uint32).copy()
        assert np.count_nonzero(per["td0"]) > B // 2
        out = _snapshot(eng)
        out.update(per)
        res.append(out)
    _equal(*res)


def _runner(name, env, B, graphs=True, steps=4):
    from maddpg_amd.runner import VecRunner
    with _environ(env):
        r = VecRunner(name, 64, batch_size=B, capacity=20000, seed=3, train_every=16, max_episode_len=5)
    _check_twin(r.eng, env)
    r.eng.set_graphs(graphs)
    r.prefill()
    for _ in range(steps):
        assert r.step() == 4
    return _snapshot(r.eng)


def test_narrow_instantiation():
    """simple_speaker_listener (action widths 3 and 5): the NARROW kernels, trained steps"""
    _equal(_runner("simple_speaker_listener", TWIN["on"], 128, steps=2),
           _runner("simple_speaker_listener", TWIN["off"], 128, steps=2))


def test_step_graph_replay():
    """mdp_train_step at E = 64, B = 64: four steps with rounds due (the first runs eagerly,
    the rest replay the captured graph), twin on and off and the eager twin run"""
    on = _runner("simple_spread", TWIN["on"], 64)
    _equal(on, _runner("simple_spread", TWIN["off"], 64))
    _equal(on, _runner("simple_spread", TWIN["on"], 64, graphs=False))


def test_batch_too_large_for_twins_keeps_one_workgroup_per_tile():
    """B = 2048 at n = 3: 2 x 128 + 128 + 1 workgroups are more than the GPU's CUs, so the
    handle launches one workgroup per tile with the switch in either state"""
    B = 2048
    assert 3 * ((B + 15) // 16) + 1 > torch.cuda.get_device_properties(0).multi_processor_count
    c = _case(B)
    on, off = _by_agent(c, B, TWIN["on"]), _by_agent(c, B, TWIN["off"])
    assert on["critic_launches"][0] == off["critic_launches"][0] == 3      # (_check_twin: 1 in both)
    _equal(on, off)


def test_throughput_mode_keeps_one_workgroup_per_tile():
    """throughput mode (every agent's critic step in one launch) never twins"""
    B = 64
    c = _case(B, DIMS, [False] * 3)
    res = []
    for env in TWIN.values():
        eng = _engine(c, B, env, DIMS, [False] * 3, prof=True)
        eng.set_update_mode("throughput")
        eng.update_all(idx=torch.from_numpy(c["idx"]), u_tgt=torch.from_numpy(c["u_tgt"]),
                       u_act=torch.from_numpy(c["u_act"]))
        res.append(_snapshot(eng, prof=True))
    assert res[0]["critic_launches"][0] == res[1]["critic_launches"][0] == 1
    _equal(*res)
