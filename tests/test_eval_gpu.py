"""GPU: device-side policy evaluation (mdp_evaluate, k_eval_episodes).

An evaluation episode is k_rollout's step chain without its side effects, so the
reference of every test here is the existing chain itself (tests/eval_oracle.py):
sample mode bit for bit, the record sums bit for bit, mean mode within a bound
measured in the same test on parent code paths.  max_episode_len = 5 everywhere.
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
from oracle import mpe, nets, philox  # noqa: E402
from tests import eval_oracle as eo  # noqa: E402

T, ACT = eo.T, eo.ACT
SEED = 0x0123456789ABCDEF
FIRST, COUNT = 7, 40          # two full 16-id tiles and a ragged tile of 8
IDS = np.arange(FIRST, FIRST + COUNT)


@functools.lru_cache(maxsize=None)
def _sample(case):
    """engine A's evaluation of IDS with its own noise, shared by the tests (never modified)"""
    a = eo.make_engine(case, 4, SEED)
    start = a.eval_initial_state(COUNT, FIRST)
    res = a.evaluate(COUNT, FIRST, bench=case in eo.BENCH_CASES)
    ret = res["returns"].cpu().numpy()
    rec = None if res["bench"] is None else res["bench"].cpu().numpy()
    for arr in (ret, rec, *start.values()):
        if arr is not None:
            arr.setflags(write=False)
    return a, start, ret, rec


def _oracle_scn(case):
    name, n, na, _lq, _h = eo.CASES[case]
    if name == "simple_tag":
        return mpe.SimpleTag(n_adv=na, n_good=n - na)
    if name == "simple_adversary":
        return mpe.SimpleAdversary(n_good=n - na, n_adv=na)
    if name == "simple_spread":
        return mpe.SimpleSpread(n)
    if name == "simple_speaker_listener":
        from tests.speaker_listener import SimpleSpeakerListener
        return SimpleSpeakerListener()
    return mpe.Simple()


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", list(eo.CASES))
def test_sample_mode_is_the_step_chain_bit_for_bit(case):
    """40 ids from 7 on engine A == engine B (num_envs = 40, the same parameters)
    started from A's start states and stepped 5 times with the ids' uniforms
    (stream 0x70000 | agent, counter = step, row = id): B's episode log, exactly.
    Once with A's own device noise, once with the same uniforms injected into A."""
    a, start, ret, _rec = _sample(case)
    u = eo.noise(SEED, a.n, IDS)
    want = eo.chain(case, SEED, start, lambda b, t: b.env_step(u=torch.from_numpy(u[:, t])))
    assert np.all(np.isfinite(want)) and np.any(want != 0)
    np.testing.assert_array_equal(ret, want)
    inj = a.evaluate(COUNT, FIRST, u=torch.from_numpy(u))["returns"].cpu().numpy()
    np.testing.assert_array_equal(inj, want)
    if case not in ("adversary_ddpg", "tag"):     # collaborative (or one agent): the shared sum
        assert np.all(ret == ret[:, :1])


@pytest.mark.parametrize("case", list(eo.CASES))
def test_start_states_are_the_scenario_reset_on_pinned_philox(case):
    """eval_initial_state = reset_world on slot_uniforms(seed, 0x60000, 0, ids, 2 ne + 1),
    within the 1e-6 of the existing reset test; velocities zero, goals exact"""
    _a, start, _ret, _rec = _sample(case)
    sc = _oracle_scn(case)
    ne = start["pos"].shape[1]
    want = sc.reset(philox.ResetStream(philox.slot_uniforms(SEED, eo.RESET_STREAM, 0, IDS, 2 * ne + 1), ne), COUNT)
    np.testing.assert_allclose(start["pos"], want["pos"], rtol=0, atol=1e-6)
    assert np.all(start["vel"] == 0)
    if case in ("adversary_ddpg", "speaker_listener"):
        np.testing.assert_array_equal(start["goal"], want["goal"])
        assert len(set(start["goal"].tolist())) > 1
    else:
        assert np.all(start["goal"] == 0)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("mode", ["sample", "mean"])
@pytest.mark.parametrize("case", ["spread3", "speaker_listener"])
def test_result_is_a_pure_function_of_the_ids(case, mode):
    """ids [0, 48) in one call == the calls [0, 16) + [16, 21) + [21, 48) == the same
    ids on handles with num_envs = 1 and 64 (whose training env state was also
    reset and stepped): exact, returns and record sums"""
    bench = case in eo.BENCH_CASES

    def run(eng, pieces):
        out = [eng.evaluate(c, f, mode=mode, bench=bench) for f, c in pieces]
        ret = torch.cat([o["returns"] for o in out]).cpu().numpy()
        rec = torch.cat([o["bench"] for o in out]).cpu().numpy() if bench else None
        return ret, rec

    a = eo.make_engine(case, 4, SEED)
    ret, rec = run(a, [(0, 48)])
    assert ret.shape == (48, a.n) and np.all(np.isfinite(ret))
    assert len({r.tobytes() for r in ret}) == 48          # every id its own episode
    for eng, pieces in ((a, [(0, 16), (16, 5), (21, 27)]),
                        (eo.make_engine(case, 1, SEED), [(0, 48)]),
                        (eo.make_engine(case, 64, SEED), [(0, 48)])):
        if eng is not a:
            eng.env_reset()
            eng.env_step()
        r2, b2 = run(eng, pieces)
        np.testing.assert_array_equal(r2, ret)
        if bench:
            np.testing.assert_array_equal(b2, rec)


# ------------------------------------------------------------------ 3
REGIONS = ("theta", "target", "adam_m", "adam_v", "grad", "replay", "index", "stats", "env", "eplog", "beta",
           "slab", "ctl")


@pytest.mark.parametrize("graphs", [True, False])
def test_evaluation_has_no_side_effects(graphs):
    """two train_step(1) on a prefilled ring == train_step(1), evaluate, train_step(1):
    every arena region and the index RNG state, bit for bit"""
    from maddpg_amd.runner import VecRunner

    def run(with_eval):
        r = VecRunner("simple_spread", 16, batch_size=64, capacity=4096, seed=5, train_every=16, max_episode_len=T)
        r.eng.set_graphs(graphs)
        r.prefill()
        r.eng.train_step(1)
        if with_eval:
            for mode in ("sample", "mean"):
                out = r.eng.evaluate(40, 3, mode=mode, bench=True)
                assert np.all(np.isfinite(out["returns"].cpu().numpy()))
        r.eng.train_step(1)
        r.eng.synchronize()
        regions = {k: r.eng.region(k, torch.uint8).cpu().numpy() for k in REGIONS}
        # (the slab's never-read pad lanes hold stale LDS: two plain runs differ there)
        regions["slab"][eo.slab_unwritten_lanes(r.eng)] = 0
        return regions, r.eng.get_rng_state(), r.eng.buffer_len(), r.eng.episode_count()

    plain, mixed = run(False), run(True)
    for k in REGIONS:
        assert np.array_equal(plain[0][k], mixed[0][k]), f"region {k} differs after an evaluation"
    np.testing.assert_array_equal(plain[1], mixed[1])
    assert plain[2:] == mixed[2:]


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("case", eo.BENCH_CASES)
def test_record_sums_are_the_step_records_summed_in_step_order(case):
    """bench == the fp32 sum, in step order, of the records engine B's
    env_step_bench writes on the same chain (the ids' uniforms injected), exactly"""
    a, start, ret, rec = _sample(case)
    u = eo.noise(SEED, a.n, IDS)
    total = np.zeros((COUNT, a.n, _lib.BENCH_W), np.float32)

    def step(b, t):
        nonlocal total
        total = total + b.env_step_bench(u=torch.from_numpy(u[:, t])).cpu().numpy()    # fp32 + fp32

    want_ret = eo.chain(case, SEED, start, step)
    np.testing.assert_array_equal(ret, want_ret)
    assert total.dtype == np.float32 and np.any(total != 0)
    np.testing.assert_array_equal(rec, total)


@pytest.mark.parametrize("case,why", [("simple", "no benchmark_data"), ("speaker_listener", "benchmark_data raises")])
def test_records_refused_where_the_scenario_has_none(case, why):
    a = eo.make_engine(case, 4, SEED)
    with pytest.raises(_lib.MdpError, match=why):
        a.evaluate(16, bench=True)
    assert a.evaluate(16)["bench"] is None


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("case", ["spread3", "speaker_listener", "tag"])
def test_mean_mode(case):
    """Mean mode: deterministic, noise-free (it differs from sample mode and takes no
    uniforms), and equal to chain B stepped with act_in = fp32(softmax in fp64 of
    mdp_actor_logits).  B's forward and softmax are not the rollout's (another
    kernel, libm's exp), so parity is not exact; the yardstick is measured here on
    parent code paths: the same B chain with act_in = nets.gumbel_softmax(logits, u)
    against the exact sample-mode returns of test 1 -- what a host-side softmax
    costs on these episodes.  Mean mode is the same mechanism on other inputs, so
    it may deviate by 4 x that yardstick (its largest element), and never less
    than one fp32 ulp of the return."""
    a, start, ret, _rec = _sample(case)
    mean = a.evaluate(COUNT, FIRST, mode="mean")["returns"].cpu().numpy()
    np.testing.assert_array_equal(a.evaluate(COUNT, FIRST, mode="mean")["returns"].cpu().numpy(), mean)
    assert np.any(mean != ret)
    with pytest.raises(_lib.MdpError, match="MDP_EVAL_MEAN"):
        a.evaluate(COUNT, FIRST, mode="mean", u=torch.zeros(COUNT, T, a.n, ACT))

    u = eo.noise(SEED, a.n, IDS)
    w = a.act_dims

    def host_sample(b, t):
        b.env_step(act_in=eo.host_actions(b, lambda j, lg: nets.gumbel_softmax(lg, u[:, t, j, :w[j]])))

    yard = float(np.max(np.abs(eo.chain(case, SEED, start, host_sample).astype(np.float64) - ret)))
    want = eo.chain(case, SEED, start, lambda b, t: b.env_step(act_in=eo.host_actions(b, lambda j, lg: eo.softmax64(lg))))
    dev = np.abs(mean.astype(np.float64) - want)
    bound = np.maximum(4 * yard, np.spacing(np.abs(want)).astype(np.float64))
    print(f"{case}: yardstick {yard:.3e}, mean-mode deviation {dev.max():.3e}, largest |return| {np.abs(want).max():.3e}")
    assert np.all(dev <= bound), (yard, float(dev.max()))


# ------------------------------------------------------------------ 6
def _refused(eng, fn, *args):
    rc = getattr(eng.lib, fn)(eng.h, *args)
    assert rc < 0, fn
    return eng.lib.mdp_last_error(eng.h).decode()


def test_refusals_launch_nothing():
    """host, pinned and one-float-short buffers on every device pointer; bad counts,
    id ranges and modes on both calls; a handle without a device scenario"""
    case = "spread3"
    a = eo.make_engine(case, 4, SEED)
    n, E = a.n, 16
    a.prof_enable("eval")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda k: torch.full((k,), 7.0, dtype=torch.float32, device=a.device)  # noqa: E731
    sizes = {"u": E * T * n * ACT, "ret": E * n, "bench": E * n * _lib.BENCH_W}
    good = {k: dev(v) for k, v in sizes.items()}

    def call(**over):
        ptr = {k: p(v) for k, v in good.items()}
        ptr.update(over)
        return _refused(a, "mdp_evaluate", 0, E, 0, ptr["u"], ptr["ret"], ptr["bench"])

    host = {k: np.zeros(v, np.float32) for k, v in sizes.items()}
    pinned = {k: torch.zeros(v, dtype=torch.float32).pin_memory() for k, v in sizes.items()}
    nbytes, base = 4 << 20, ctypes.c_void_p()
    assert a.lib.hipMalloc(ctypes.byref(base), ctypes.c_size_t(nbytes)) == 0
    try:
        rb, ext = ctypes.c_void_p(), ctypes.c_size_t()
        assert a.lib.hipMemGetAddressRange(ctypes.byref(rb), ctypes.byref(ext), base) == 0
        assert rb.value == base.value and ext.value == nbytes     # the extent the library checks against
        for k, v in sizes.items():
            assert "not device memory" in call(**{k: ctypes.c_void_p(host[k].ctypes.data)}), k
            assert "not device memory" in call(**{k: p(pinned[k])}), k
            short = ctypes.c_void_p(base.value + nbytes - 4 * (v - 1))
            assert "allocation too small" in call(**{k: short}), k
    finally:
        torch.cuda.synchronize()
        assert a.lib.hipFree(base) == 0
    assert "ret_dev is null" in call(ret=None)
    ne = a.n_entities
    hpos, hvel = np.full((E, ne, 2), 7, np.float32), np.full((E, ne, 2), 7, np.float32)
    hgoal = np.full(E, 7, np.int32)
    f32, i32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    st = (hpos.ctypes.data_as(f32), hvel.ctypes.data_as(f32), hgoal.ctypes.data_as(i32))
    ok = (p(good["u"]), p(good["ret"]), p(good["bench"]))
    for count in (0, -1, (1 << 20) + 1):
        assert "2^20" in _refused(a, "mdp_evaluate", 0, count, 0, *ok)
        assert "2^20" in _refused(a, "mdp_eval_initial_state", 0, count, *st)
    for first in (-1, (1 << 32) - E + 1, 1 << 40):
        assert "uint32" in _refused(a, "mdp_evaluate", first, E, 0, *ok)
        assert "uint32" in _refused(a, "mdp_eval_initial_state", first, E, *st)
    for mode in (-1, 2):
        assert "mode" in _refused(a, "mdp_evaluate", 0, E, mode, *ok)
    assert "MDP_EVAL_MEAN" in _refused(a, "mdp_evaluate", 0, E, 1, *ok)
    assert "null" in _refused(a, "mdp_eval_initial_state", 0, E, None, st[1], st[2])
    # nothing was launched or written
    a.synchronize()
    assert a.prof_read("eval") == (0.0, 0)
    assert all(bool(torch.all(v == 7.0)) for v in good.values())
    assert np.all(hpos == 7) and np.all(hvel == 7) and np.all(hgoal == 7)
    # the last ids of the range are accepted, and the handle still works; the launch is timed
    top = a.evaluate(E, (1 << 32) - E)["returns"].cpu().numpy()
    assert np.all(np.isfinite(top))
    assert a.prof_read("eval")[1] == 1
    # a handle without a device scenario
    plain = Engine([6], batch_size=16, capacity=64)
    assert "no device env" in _refused(plain, "mdp_evaluate", 0, E, 0, None, p(good["ret"]), None)
    assert "no device env" in _refused(plain, "mdp_eval_initial_state", 0, E, *st)
    with pytest.raises(ValueError, match="mode"):
        a.evaluate(E, mode="greedy")


def test_load_state_of_selected_agents(tmp_path):
    """Engine.load_state(fname, agents=[...]) restores those agents only"""
    a = eo.make_engine("adversary_ddpg", 4, SEED)
    b = eo.make_engine("adversary_ddpg", 4, SEED)
    b.init_params(eo.PSEED + 1)
    path = b.save_state(str(tmp_path / "b"))
    before = [a.get_params(i, "actor") for i in range(a.n)]
    a.load_state(path, agents=[0])
    for i in range(a.n):
        src = b.get_params(i, "actor") if i == 0 else before[i]
        for k, v in a.get_params(i, "actor").items():
            np.testing.assert_array_equal(v, src[k])
    with pytest.raises(ValueError, match="out of range"):
        a.load_state(path, agents=[3])
