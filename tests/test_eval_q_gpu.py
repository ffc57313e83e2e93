"""GPU: critic evaluation (mdp_evaluate_q, k_eval_episodes<H, EvalQArgs> + k_eval_returns).

The trajectory is mdp_evaluate's (bit for bit, and a longer run reproduces a
shorter one); Q is the value mdp_q_values gives on the rows the existing step
chain appends (bit for bit) and is measured against oracle/nets.py's forward in
fp64; the return-to-go and the gap are the fp64 recursion on the returned
reward trace.  max_episode_len = 5 everywhere, 12 steps in the longer run.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd import _lib  # noqa: E402
from maddpg_amd.engine import Engine  # noqa: E402
from tests import eval_oracle as eo  # noqa: E402
from tests import eval_q_cases as qc  # noqa: E402

T, ACT, SEED, FIRST, COUNT, IDS, STEPS = qc.T, qc.ACT, qc.SEED, qc.FIRST, qc.COUNT, qc.IDS, qc.STEPS
KEYS = ("q", "rew", "g", "gap")


def _np(res):
    out = {k: res[k].cpu().numpy() for k in KEYS}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _long(case):
    """engine A and its 12-step evaluation of IDS on its own noise, shared by the tests (never modified)"""
    a = qc.make_engine(case, 4)
    return a, _np(a.evaluate_q(COUNT, steps=STEPS, scored=T, first_episode=FIRST))


def _step_order_sum(rew):
    s = np.zeros(rew[:, 0].shape, np.float32)
    for t in range(rew.shape[1]):
        s = s + rew[:, t]                       # fp32 + fp32
    return s


# ------------------------------------------------------------------ trajectory
@pytest.mark.parametrize("case", list(qc.CASES))
def test_trajectory_is_evaluates(case):
    """steps = 5: the fp32 step-order sum of rew == evaluate's returns, bit for bit;
    steps = 12: the first 5 steps of q and rew == the steps = 5 call.  With the
    device's noise, with the same uniforms injected, and in mean mode."""
    a, long = _long(case)
    u = qc.noise(SEED, a.n, IDS, STEPS)
    runs = {
        "device noise": ({}, {}, {}, long),
        "injected": ({"u": torch.from_numpy(u[:, :T].copy())}, {"u": torch.from_numpy(u[:, :T].copy())},
                     {"u": torch.from_numpy(u)}, None),
        "mean": ({"mode": "mean"}, {"mode": "mean"}, {"mode": "mean"}, None),
    }
    for name, (kw_ret, kw5, kw12, have12) in runs.items():
        ret = a.evaluate(COUNT, FIRST, **kw_ret)["returns"].cpu().numpy()
        r5 = _np(a.evaluate_q(COUNT, steps=T, scored=T, first_episode=FIRST, **kw5))
        r12 = have12 or _np(a.evaluate_q(COUNT, steps=STEPS, scored=T, first_episode=FIRST, **kw12))
        assert r5["q"].shape == (COUNT, T, a.n, 1) and r12["rew"].shape == (COUNT, STEPS, a.n), name
        assert all(np.all(np.isfinite(v)) for v in (*r5.values(), *r12.values())), name
        np.testing.assert_array_equal(_step_order_sum(r5["rew"]), ret, err_msg=name)
        np.testing.assert_array_equal(r12["q"][:, :T], r5["q"], err_msg=name)
        np.testing.assert_array_equal(r12["rew"][:, :T], r5["rew"], err_msg=name)
        assert np.any(r12["rew"][:, T:] != 0) and np.any(r12["q"][:, T:] != r12["q"][:, :1]), name
        if name == "injected":                   # the injected uniforms are the device's own
            for k in KEYS:
                np.testing.assert_array_equal(r12[k], long[k], err_msg=k)
        if name == "mean":
            assert np.any(r12["rew"] != long["rew"])
    with pytest.raises(_lib.MdpError, match="MDP_EVAL_MEAN"):
        a.evaluate_q(COUNT, steps=T, first_episode=FIRST, mode="mean", u=torch.zeros(COUNT, T, a.n, ACT))


@pytest.mark.parametrize("mode", ["sample", "mean"])
@pytest.mark.parametrize("case", ["spread3", "adversary_ddpg"])
def test_split_invariance(case, mode):
    """ids [0, 48) in one call == three calls of 16 == the same ids on handles with
    1 and 64 env copies (whose training env was also reset and stepped): exact"""
    def run(eng, pieces):
        out = [eng.evaluate_q(c, steps=STEPS, scored=T, first_episode=f, mode=mode) for f, c in pieces]
        return {k: torch.cat([o[k] for o in out]).cpu().numpy() for k in KEYS}

    a = qc.make_engine(case, 4)
    one = run(a, [(0, 48)])
    assert len({r.tobytes() for r in one["q"]}) == 48           # every id its own episode
    for eng, pieces in ((a, [(0, 16), (16, 16), (32, 16)]),
                        (qc.make_engine(case, 1), [(0, 48)]),
                        (qc.make_engine(case, 64), [(0, 48)])):
        if eng is not a:
            eng.env_reset()
            eng.env_step()
        got = run(eng, pieces)
        for k in KEYS:
            np.testing.assert_array_equal(got[k], one[k], err_msg=k)


# ------------------------------------------------------------------ Q
def _rows(case, a):
    start = a.eval_initial_state(COUNT, FIRST)
    return qc.chain_rows(case, start, qc.noise(SEED, a.n, IDS, STEPS))      # [STEPS, COUNT, row_stride]


def _oracle_q(eng, j, which, x_dev):
    cols = eng.cin_columns(j)
    return qc.critic64(eng.get_params(j, which), x_dev.cpu().numpy()[:, cols])


@pytest.mark.parametrize("case", list(qc.CASES))
def test_q_is_the_critics(case):
    """q[:, t, j, 0] == q_values(j, x_t) bit for bit on the rows the step chain appends
    (all 12 steps: the chain is built not to reset before).  Independently against the
    fp64 forward: within 4 x the deviation of mdp_q_values from it on the same rows."""
    a, long = _long(case)
    rows = _rows(case, a)
    flat = rows.reshape(STEPS * COUNT, -1)
    for j in range(a.n):
        x = qc.critic_input(a, j, flat)
        want = a.q_values(j, x).cpu().numpy().reshape(STEPS, COUNT).T
        got = long["q"][:, :, j, 0]
        np.testing.assert_array_equal(got, want, err_msg=f"agent {j}")
        ref = _oracle_q(a, j, "critic", x).reshape(STEPS, COUNT).T
        yard = float(np.max(np.abs(want.astype(np.float64) - ref)))
        dev = float(np.max(np.abs(got.astype(np.float64) - ref)))
        print(f"{case} agent {j}: mdp_q_values vs fp64 {yard:.3e}, evaluate_q vs fp64 {dev:.3e}, "
              f"largest |Q| {np.abs(ref).max():.3e}")
        assert yard > 0 and np.abs(ref).max() > 1e-3
        assert dev <= 4 * yard
    # the step rewards are the rows' too
    for j in range(a.n):
        np.testing.assert_array_equal(long["rew"][:, :, j], rows[:, :, a.row_layout[j][3]].cpu().numpy().T)


@pytest.mark.parametrize("case", ["spread3", "adversary_ddpg", "spread3_h128"])
def test_td3_twin_columns(case):
    """C = 2 on a td3 engine.  critic2 := critic: both columns bit-equal, and column 0
    is the MADDPG handle's.  A distinct twin: column 1 against the fp64 forward on the
    MDP_CRITIC2 parameters, within 4 x mdp_q_values' deviation (critic 1, same rows)."""
    a, long = _long(case)
    t3 = qc.make_engine(case, 4, td3=True)
    other = qc.make_engine(case, 4)
    other.init_params(qc.PSEED + 1)
    for j in range(a.n):
        for which in ("actor", "critic"):
            t3.set_params(j, which, a.get_params(j, which))
        t3.set_params(j, "critic2", a.get_params(j, "critic"))
    same =_np(t3.evaluate_q(COUNT, steps=STEPS, scored=T, first_episode=FIRST))
    assert same["q"].shape == (COUNT, STEPS, a.n, 2) and same["gap"].shape == (COUNT, a.n, 2)
    np.testing.assert_array_equal(same["q"][..., 1], same["q"][..., 0])
    np.testing.assert_array_equal(same["gap"][..., 1], same["gap"][..., 0])
    np.testing.assert_array_equal(same["q"][..., 0], long["q"][..., 0])
    for k in ("rew", "g"):
        np.testing.assert_array_equal(same[k], long[k])
    for j in range(a.n):
        t3.set_params(j, "critic2", other.get_params(j, "critic"))
    twin = _np(t3.evaluate_q(COUNT, steps=STEPS, scored=T, first_episode=FIRST))
    np.testing.assert_array_equal(twin["q"][..., 0], long["q"][..., 0])
    flat = _rows(case, a).reshape(STEPS * COUNT, -1)
    for j in range(a.n):
        x = qc.critic_input(a, j, flat)
        q1 = a.q_values(j, x).cpu().numpy().astype(np.float64)
        yard = float(np.max(np.abs(q1 - _oracle_q(t3, j, "critic", x))))
        ref2 = _oracle_q(t3, j, "critic2", x).reshape(STEPS, COUNT).T
        dev = float(np.max(np.abs(twin["q"][:, :, j, 1].astype(np.float64) - ref2)))
        print(f"{case} agent {j}: yardstick {yard:.3e}, twin vs fp64 {dev:.3e}, largest |Q2| {np.abs(ref2).max():.3e}")
        assert yard > 0 and dev <= 4 * yard
        assert np.any(twin["q"][:, :, j, 1] != twin["q"][:, :, j, 0])
        # the twin's value is the critic kernel's on those parameters: bit for bit
        np.testing.assert_array_equal(twin["q"][:, :, j, 1].T.reshape(-1), other.q_values(j, x).cpu().numpy())


# ------------------------------------------------------------------ returns
@pytest.mark.parametrize("td3", [False, True])
@pytest.mark.parametrize("steps,scored", [(STEPS, T), (STEPS, 1), (STEPS, STEPS), (1, 1), (33, 33), (70, 40), (None, None)])
def test_returns_are_the_fp64_recursion(steps, scored, td3):
    """g within one fp32 ulp of float32(G) of the fp64 recursion on the returned rew
    trace; gap within 1e-6 * max|g| of the numpy value (fp32 rounding of a sum whose
    terms are formed in fp64).  scored = 1, scored = steps, steps = 1; 33 and 70
    steps cross the return kernel's 32-step blocks; None: the default window."""
    a = qc.make_engine("tag", 4, td3=td3)
    res = a.evaluate_q(COUNT, steps=steps, scored=scored, first_episode=FIRST)
    if steps is None:
        assert (res["steps"], res["scored"]) == (T + 90, T) == a.eval_q_window()
        steps, scored = res["steps"], res["scored"]
        assert abs(res["summary"]["truncation"] - 0.95 ** 91) < 1e-6
    r = _np(res)
    G, gap = qc.returns64(r["rew"], 0.95, scored, r["q"])
    g32 = G.astype(np.float32)
    assert np.all(np.abs(r["g"].astype(np.float64) - g32) <= np.spacing(np.abs(g32)))
    scale = float(np.abs(r["g"]).max())
    assert scale > 0
    err = float(np.max(np.abs(r["gap"].astype(np.float64) - gap)))
    print(f"steps {steps} scored {scored}: gap error {err:.3e}, bound {1e-6 * scale:.3e}")
    assert err <= 1e-6 * scale
    s = res["summary"]
    np.testing.assert_allclose(s["gap_mean"], gap.mean(0), rtol=0, atol=2e-6 * scale)
    np.testing.assert_allclose(s["gap_rms"], np.sqrt((gap ** 2).mean(0)), rtol=0, atol=2e-6 * scale)
    np.testing.assert_allclose(s["q_mean"], r["q"][:, :scored].astype(np.float64).mean((0, 1)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.array(s["g_mean"])[:, 0], r["g"][:, :scored].astype(np.float64).mean((0, 1)),
                               rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ side effects
REGIONS = ("theta", "target", "adam_m", "adam_v", "grad", "replay", "index", "stats", "env", "eplog", "beta",
           "slab", "ctl")


@pytest.mark.parametrize("td3", [False, True])
@pytest.mark.parametrize("graphs", [True, False])
def test_evaluate_q_has_no_side_effects(graphs, td3):
    """train_step(1), evaluate_q, train_step(1) == two train_step(1): every arena region
    (the slab's never-read pad lanes apart, as in tests/test_eval_gpu.py), the second
    critic's five parameter regions of the TD3 buffer and its counters, the index RNG"""
    from maddpg_amd.runner import VecRunner

    def run(with_eval):
        r = VecRunner("simple_spread", 16, batch_size=64, capacity=4096, seed=5, train_every=16, max_episode_len=T,
                      td3=td3)
        r.eng.set_graphs(graphs)
        r.prefill()
        r.eng.train_step(1)
        if with_eval:
            for mode in ("sample", "mean"):
                out = r.eng.evaluate_q(40, steps=STEPS, scored=T, first_episode=3, mode=mode)
                assert np.all(np.isfinite(out["gap"].cpu().numpy())) and out["q"].shape[3] == (2 if td3 else 1)
        r.eng.train_step(1)
        r.eng.synchronize()
        regions = {k: r.eng.region(k, torch.uint8).cpu().numpy() for k in REGIONS}
        regions["slab"][eo.slab_unwritten_lanes(r.eng)] = 0
        twin = {}
        if td3:
            twin = {k: r.eng.td3_region(k).cpu().numpy() for k in Engine.TD3_REGIONS}
            twin["info"] = [r.eng.td3_info(i) for i in range(r.eng.n)]
        return regions, r.eng.get_rng_state(), r.eng.buffer_len(), r.eng.episode_count(), twin

    plain, mixed = run(False), run(True)
    for k in REGIONS:
        assert np.array_equal(plain[0][k], mixed[0][k]), f"region {k} differs after evaluate_q"
    np.testing.assert_array_equal(plain[1], mixed[1])
    assert plain[2:4] == mixed[2:4]
    for k in plain[4]:
        assert np.array_equal(plain[4][k], mixed[4][k]) if k != "info" else plain[4][k] == mixed[4][k], k


# ------------------------------------------------------------------ refusals
def _refused(eng, fn, *args):
    rc = getattr(eng.lib, fn)(eng.h, *args)
    assert rc < 0, fn
    return eng.lib.mdp_last_error(eng.h).decode()


def test_refusals_launch_nothing():
    """every refusal of mdp_evaluate_q: host, pinned and one-float-short buffers on each
    of the five pointers, NULL outputs, bad counts, id ranges, modes, steps and scored,
    uniforms in mean mode, a capturing stream, a handle without a device scenario, a NULL
    handle -- each message names the entry point, nothing is launched or written, and a
    good call follows each group"""
    fn = "mdp_evaluate_q"
    a, long = _long("spread3")
    n, E, S, K = a.n, 16, STEPS, T
    a.prof_enable("eval")
    timed = a.prof_read("eval")[1]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda k: torch.full((k,), 7.0, dtype=torch.float32, device=a.device)  # noqa: E731
    sizes = {"u": E * S * n * ACT, "q": E * S * n, "rew": E * S * n, "g": E * S * n, "gap": E * n}
    good = {k: dev(v) for k, v in sizes.items()}
    good["u"].fill_(0.5)

    def call(first=0, episodes=E, mode=0, steps=S, scored=K, **over):
        ptr = {k: p(v) for k, v in good.items()}
        ptr.update(over)
        return _refused(a, fn, first, episodes, mode, steps, scored, ptr["u"], ptr["q"], ptr["rew"], ptr["g"], ptr["gap"])

    def works():
        got = _np(a.evaluate_q(COUNT, steps=STEPS, scored=T, first_episode=FIRST))
        for k in KEYS:
            np.testing.assert_array_equal(got[k], long[k], err_msg=k)

    host = {k: np.zeros(v, np.float32) for k, v in sizes.items()}
    pinned = {k: torch.zeros(v, dtype=torch.float32).pin_memory() for k, v in sizes.items()}
    nbytes, base = 4 << 20, ctypes.c_void_p()
    assert a.lib.hipMalloc(ctypes.byref(base), ctypes.c_size_t(nbytes)) == 0
    try:
        rb, ext = ctypes.c_void_p(), ctypes.c_size_t()
        assert a.lib.hipMemGetAddressRange(ctypes.byref(rb), ctypes.byref(ext), base) == 0
        assert rb.value == base.value and ext.value == nbytes     # the extent the library checks against
        for k, v in sizes.items():
            assert f"{fn}: {k}_dev is not device memory" in call(**{k: ctypes.c_void_p(host[k].ctypes.data)}), k
            assert f"{fn}: {k}_dev is not device memory" in call(**{k: p(pinned[k])}), k
            short = ctypes.c_void_p(base.value + nbytes - 4 * (v - 1))
            assert f"{fn}: {k}_dev ends before" in call(**{k: short}), k
    finally:
        torch.cuda.synchronize()
        assert a.lib.hipFree(base) == 0
    works()
    for k in ("q", "rew", "g", "gap"):
        assert f"{fn}: {k}_dev is null" in call(**{k: None})
    for count in (0, -1, (1 << 20) + 1):
        assert f"{fn}: 1 <= episodes <= 2^20" in call(episodes=count)
    for first in (-1, (1 << 32) - E + 1, 1 << 40):
        msg = call(first=first)
        assert fn in msg and "uint32" in msg
    for mode in (-1, 2):
        assert f"{fn}: mode" in call(mode=mode)
    for steps in (0, -1, 4097):
        assert f"{fn}: 1 <= steps <= 4096" in call(steps=steps, scored=1)
    for scored in (0, -1, S + 1):
        assert f"{fn}: 1 <= scored <= steps" in call(scored=scored)
    assert f"{fn}: u_dev is given but MDP_EVAL_MEAN" in call(mode=1)
    works()
    # a capturing stream
    stream, graph = ctypes.c_void_p(a.lib.mdp_stream(a.h)), ctypes.c_void_p()
    a.synchronize()
    torch.cuda.synchronize()
    assert a.lib.hipStreamBeginCapture(stream, 2) == 0        # hipStreamCaptureModeRelaxed
    try:
        msg = call(u=None)
    finally:
        assert a.lib.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
        if graph.value:
            assert a.lib.hipGraphDestroy(graph) == 0
    assert fn in msg and "capturing" in msg
    # nothing was launched or written by any of them
    a.synchronize()
    assert a.prof_read("eval")[1] == timed + 2 * 2            # works() twice: two launches each, both timed
    assert all(bool(torch.all(v == (0.5 if k == "u" else 7.0))) for k, v in good.items())
    # a handle without a device scenario, a NULL handle
    plain = Engine([6], batch_size=16, capacity=64)
    assert "no device env" in _refused(plain, fn, 0, E, 0, S, K, None, p(good["q"]), p(good["rew"]), p(good["g"]),
                                       p(good["gap"]))
    assert a.lib.mdp_evaluate_q(None, 0, E, 0, S, K, None, p(good["q"]), p(good["rew"]), p(good["g"]), p(good["gap"])) < 0
    # Python's own checks
    with pytest.raises(ValueError, match="mode"):
        a.evaluate_q(E, mode="greedy")
    with pytest.raises(ValueError, match="u: "):
        a.evaluate_q(E, steps=S, u=torch.zeros(E, S - 1, n, ACT))
    # the last ids of the range are accepted; the handle still evaluates and trains
    top = a.evaluate_q(E, steps=S, scored=K, first_episode=(1 << 32) - E)
    assert np.all(np.isfinite(top["gap"].cpu().numpy()))
    works()
    assert np.all(np.isfinite(a.evaluate(E)["returns"].cpu().numpy()))
    a.prof_enable("eval", False)
    from maddpg_amd.runner import VecRunner
    r = VecRunner("simple_spread", 16, batch_size=64, capacity=4096, seed=5, train_every=16, max_episode_len=T)
    r.prefill()
    assert "1 <= scored <= steps" in _refused(r.eng, fn, 0, E, 0, S, S + 1, None, p(good["q"]), p(good["rew"]),
                                              p(good["g"]), p(good["gap"]))
    r.eng.train_step(1)
    r.eng.synchronize()
    assert r.eng.check_finite() == 0
