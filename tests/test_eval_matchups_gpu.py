"""GPU: matchup evaluation (mdp_evaluate_matchups, k_eval_episodes<H, EvalMuArgs>).

A matchup is mdp_evaluate's episode with agent j's actor read from a bank set, so
the reference of every test is the existing Engine.evaluate (pinned to the step
chain by tests/test_eval_gpu.py) on an engine that holds that mix of actors.
Every comparison is exact.  max_episode_len = 5 everywhere.
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

T, ACT = eo.T, eo.ACT
SEED = 0x0123456789ABCDEF
FIRST, COUNT = 7, 40          # two full 16-id tiles and a ragged tile of 8
IDS = np.arange(FIRST, FIRST + COUNT)
SET_SEEDS = (11, 12, 13)      # init_params seeds of the bank's three sets
CASES = ("tag", "spread5", "spread3_h128", "speaker_listener")
MODES = ("sample", "mean")


def _team(case):
    na = eo.CASES[case][2]
    return list(range(na)) if na else [0]


def _table(case):
    """the three diagonals, a row that mixes the sets over the agents (every agent
    of up to three from a different set), and the team split"""
    n = eo.CASES[case][1]
    team = _team(case)
    rows = [[k] * n for k in range(3)]
    rows.append([(j + 2) % 3 for j in range(n)])
    rows.append([1 if j in team else 2 for j in range(n)])
    return np.asarray(rows, np.int32)


def _as_state(params):
    """per-agent actor dicts -> the state_dict() keys bank_write reads"""
    return {f"agent_{j}/actor/{t}": v for j, p in enumerate(params) for t, v in p.items()}


@functools.lru_cache(maxsize=None)
def _bank(case):
    """engine A (its own parameters: seed 11, never played below), the actor
    parameters of the three sets on the host, and A's bank holding them, written
    with bank_write.  Shared by the tests, never modified."""
    a = eo.make_engine(case, 4, SEED)
    donor = eo.make_engine(case, 4, SEED)
    sets = []
    bank = a.actor_bank(len(SET_SEEDS))
    assert bank.shape == (3, a.actor_set_floats()) and a.actor_set_floats() % 4 == 0 and not bool(bank.any())
    for k, s in enumerate(SET_SEEDS):
        donor.init_params(s)
        sets.append([donor.get_params(j, "actor") for j in range(a.n)])
        a.bank_write(bank, k, _as_state(sets[k]))
    return a, sets, bank


@functools.lru_cache(maxsize=None)
def _reference(case):
    """{(row, mode): (returns, bench)}: Engine.evaluate of a fresh engine whose agent
    j got set_params(j, "actor", set table[row][j]'s)"""
    _a, sets, _bank_t = _bank(case)
    bench = case in eo.BENCH_CASES
    out = {}
    for m, row in enumerate(_table(case)):
        b = eo.make_engine(case, 4, SEED)
        for j, k in enumerate(row):
            b.set_params(j, "actor", sets[k][j])
        for mode in MODES:
            r = b.evaluate(COUNT, FIRST, mode=mode, bench=bench)
            ret = r["returns"].cpu().numpy()
            rec = r["bench"].cpu().numpy() if bench else None
            for arr in (ret, rec):
                if arr is not None:
                    arr.setflags(write=False)
            out[(m, mode)] = (ret, rec)
    return out


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_every_matchup_is_evaluate_on_that_mix(case, mode):
    """returns[m] / bench[m] == evaluate(COUNT, FIRST, mode, bench) of an engine that
    holds row m's mix of actors, bit for bit; the rows differ from each other, so
    a kernel that ignores the table fails"""
    a, _sets, bank = _bank(case)
    table, want = _table(case), _reference(case)
    bench = case in eo.BENCH_CASES
    res = a.evaluate_matchups(bank, table, COUNT, FIRST, mode=mode, bench=bench)
    ret = res["returns"].cpu().numpy()
    assert ret.shape == (len(table), COUNT, a.n) and np.all(np.isfinite(ret))
    assert (res["bench"] is not None) == bench
    for m in range(len(table)):
        np.testing.assert_array_equal(ret[m], want[(m, mode)][0], err_msg=f"matchup {m} {table[m]}")
        if bench:
            np.testing.assert_array_equal(res["bench"][m].cpu().numpy(), want[(m, mode)][1])
    assert len({ret[m].tobytes() for m in range(len(table))}) == len(table)
    s = res["summary"]
    r64 = ret.astype(np.float64)
    np.testing.assert_allclose(s["mean"], r64.mean(1), rtol=1e-12)
    np.testing.assert_allclose(s["std"], r64.std(1), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(s["sem"], r64.std(1) / np.sqrt(COUNT), rtol=1e-9, atol=1e-12)


def test_injected_uniforms_are_shared_by_every_matchup():
    """the ids' own uniforms (eo.noise) injected == the device noise, for every row"""
    case = "tag"
    a, _sets, bank = _bank(case)
    table, want = _table(case), _reference(case)
    u = torch.from_numpy(eo.noise(SEED, a.n, IDS))
    res = a.evaluate_matchups(bank, table, COUNT, FIRST, bench=True, u=u)
    for m in range(len(table)):
        np.testing.assert_array_equal(res["returns"][m].cpu().numpy(), want[(m, "sample")][0])
        np.testing.assert_array_equal(res["bench"][m].cpu().numpy(), want[(m, "sample")][1])


def test_cross_play_is_table_construction():
    case = "tag"
    a, _sets, bank = _bank(case)
    team = _team(case)
    cp = a.cross_play(bank, team, COUNT, FIRST)
    K, n = 3, a.n
    assert cp["mean"].shape == cp["sem"].shape == (K, K, n) and cp["returns"].shape == (K, K, COUNT, n)
    for r in range(K):
        for c in range(K):
            assert cp["table"][r * K + c].tolist() == [r if j in team else c for j in range(n)]
    want = _reference(case)
    for k in range(K):                                       # the diagonal: one set plays itself
        np.testing.assert_array_equal(cp["returns"][k, k].cpu().numpy(), want[(k, "sample")][0])
    np.testing.assert_array_equal(cp["returns"][1, 2].cpu().numpy(), want[(4, "sample")][0])   # the team split


# ------------------------------------------------------------------ 2
def _spans(eng, bank, k):
    """the floats of slot k that mdp_tensor names (agent j's actor tensors)"""
    row = bank.view(-1, eng.actor_set_floats())[k].cpu().numpy()
    return [row[off:off + dr * dc].copy() for j in range(eng.n) for (off, _r, _c, dr, dc) in eng.net_tensors(j, 0)]


def test_the_bank_is_independent_of_the_handle(tmp_path):
    from maddpg_amd.runner import VecRunner
    r = VecRunner("simple_spread", 16, batch_size=64, capacity=4096, seed=5, train_every=16, max_episode_len=T)
    eng, n = r.eng, r.n
    r.prefill()
    bank = eng.actor_bank(2)
    eng.bank_snapshot(bank, 0)
    before = eng.evaluate(COUNT, FIRST, bench=True)
    ret0, rec0 = before["returns"].cpu().numpy(), before["bench"].cpu().numpy()
    actors0 = [eng.get_params(j, "actor") for j in range(n)]
    for _ in range(8):
        eng.train_step(1)
        now = [eng.get_params(j, "actor") for j in range(n)]
        if all(np.any(now[j]["W1"] != actors0[j]["W1"]) for j in range(n)):
            break
    assert all(np.any(now[j]["W1"] != actors0[j]["W1"]) for j in range(n)), "training did not move the actors"
    diag = lambda k: np.full((1, n), k, np.int32)  # noqa: E731
    res = eng.evaluate_matchups(bank, diag(0), COUNT, FIRST, bench=True)
    np.testing.assert_array_equal(res["returns"][0].cpu().numpy(), ret0)
    np.testing.assert_array_equal(res["bench"][0].cpu().numpy(), rec0)
    eng.bank_snapshot(bank, 1)
    after = eng.evaluate(COUNT, FIRST, bench=True)
    assert np.any(after["returns"].cpu().numpy() != ret0)
    res = eng.evaluate_matchups(bank, diag(1), COUNT, FIRST, bench=True)
    np.testing.assert_array_equal(res["returns"][0].cpu().numpy(), after["returns"].cpu().numpy())
    np.testing.assert_array_equal(res["bench"][0].cpu().numpy(), after["bench"].cpu().numpy())
    # bank_write from the engine's own state, an npz and a TF1 bundle == bank_snapshot, span by span
    theta = eng.region("theta").clone()
    snap = _spans(eng, bank, 1)
    assert any(np.any(s != 0) for s in snap)
    npz = eng.save_state(str(tmp_path / "npz" / "ck"))
    (tmp_path / "tf1").mkdir()
    tf1 = eng.save_state(str(tmp_path / "tf1" / "ck"), fmt="tf1")
    other = eng.actor_bank(3)
    for k, src in enumerate((eng.state_dict(), npz, tf1)):
        eng.bank_write(other, k, src)
        got = _spans(eng, other, k)
        assert len(got) == len(snap) == 6 * n
        for g, s in zip(got, snap):
            np.testing.assert_array_equal(g, s)
    assert torch.equal(eng.region("theta"), theta)          # the handle's parameters were not touched
    # only the chosen agents are written
    part = eng.actor_bank(1)
    eng.bank_write(part, 0, npz, agents=[1])
    got = _spans(eng, part, 0)
    for q, (g, s) in enumerate(zip(got, snap)):
        np.testing.assert_array_equal(g, s if q // 6 == 1 else np.zeros_like(s))
    bad = eng.state_dict()
    bad["agent_0/actor/W1"] = bad["agent_0/actor/W1"][:, :-1]
    with pytest.raises(ValueError):
        eng.bank_write(part, 0, bad)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("case", ["tag", "speaker_listener"])
def test_result_is_a_pure_function_of_table_row_and_id(case):
    """M matchups x ids [0, 48) in one call == the calls split by matchup and by id
    range; permuting the rows permutes the result; a set duplicated at another
    bank index gives the same rows; handles with num_envs 1 and 64 agree"""
    a, _sets, bank = _bank(case)
    table = _table(case)
    M = len(table)
    bench = case in eo.BENCH_CASES

    def run(eng, bk, tab, first, count):
        r = eng.evaluate_matchups(bk, tab, count, first, bench=bench)
        return r["returns"].cpu().numpy(), (r["bench"].cpu().numpy() if bench else np.zeros(0))

    ret, rec = run(a, bank, table, 0, 48)
    assert ret.shape == (M, 48, a.n) and len({ret[m].tobytes() for m in range(M)}) == M
    for m in range(M):
        parts = [run(a, bank, table[m:m + 1], f, c) for f, c in ((0, 16), (16, 5), (21, 27))]
        np.testing.assert_array_equal(np.concatenate([p[0][0] for p in parts]), ret[m])
        if bench:
            np.testing.assert_array_equal(np.concatenate([p[1][0] for p in parts]), rec[m])
    perm = np.asarray([3, 0, 4, 2, 1])
    r2, b2 = run(a, bank, table[perm], 0, 48)
    np.testing.assert_array_equal(r2, ret[perm])
    if bench:
        np.testing.assert_array_equal(b2, rec[perm])
    dup = torch.cat([bank, bank[0:1]]).contiguous()          # set 0 again at index 3
    moved = np.where(table == 0, 3, table).astype(np.int32)
    assert np.any(moved != table)
    r3, b3 = run(a, dup, moved, 0, 48)
    np.testing.assert_array_equal(r3, ret)
    for num_envs in (1, 64):
        e = eo.make_engine(case, num_envs, SEED)
        e.env_reset()
        e.env_step()
        r4, b4 = run(e, bank, table, 0, 48)
        np.testing.assert_array_equal(r4, ret)
        if bench:
            np.testing.assert_array_equal(b4, rec)


# ------------------------------------------------------------------ 4
REGIONS = ("theta", "target", "adam_m", "adam_v", "grad", "replay", "index", "stats", "env", "eplog", "beta",
           "slab", "ctl")


@pytest.mark.parametrize("graphs", [True, False])
def test_matchup_evaluation_has_no_side_effects(graphs):
    """two train_step(1) on a prefilled ring == train_step(1), bank_snapshot +
    evaluate_matchups, train_step(1): every arena region and the index RNG state,
    bit for bit; the call leaves the bank's bytes as they were"""
    from maddpg_amd.runner import VecRunner

    def run(with_eval):
        r = VecRunner("simple_spread", 16, batch_size=64, capacity=4096, seed=5, train_every=16, max_episode_len=T)
        r.eng.set_graphs(graphs)
        r.prefill()
        bank = r.eng.actor_bank(2)
        if with_eval:
            r.eng.bank_snapshot(bank, 0)
        r.eng.train_step(1)
        if with_eval:
            r.eng.bank_snapshot(bank, 1)
            kept = bank.clone()
            assert not torch.equal(kept[0], kept[1])
            table = np.asarray([[0, 0, 0], [1, 1, 1], [0, 1, 0]], np.int32)
            for mode in MODES:
                out = r.eng.evaluate_matchups(bank, table, 40, 3, mode=mode, bench=True)
                ret = out["returns"].cpu().numpy()
                assert np.all(np.isfinite(ret)) and np.any(ret[0] != ret[1]) and np.any(ret[2] != ret[1])
            assert torch.equal(bank, kept)
        r.eng.train_step(1)
        r.eng.synchronize()
        regions = {k: r.eng.region(k, torch.uint8).cpu().numpy() for k in REGIONS}
        # (the slab's never-read pad lanes hold stale LDS: two plain runs differ there)
        regions["slab"][eo.slab_unwritten_lanes(r.eng)] = 0
        return regions, r.eng.get_rng_state(), r.eng.buffer_len(), r.eng.episode_count()

    plain, mixed = run(False), run(True)
    for k in REGIONS:
        assert np.array_equal(plain[0][k], mixed[0][k]), f"region {k} differs after a matchup evaluation"
    np.testing.assert_array_equal(plain[1], mixed[1])
    assert plain[2:] == mixed[2:]


# ------------------------------------------------------------------ 5
def _refused(eng, fn, *args):
    rc = getattr(eng.lib, fn)(eng.h, *args)
    assert rc < 0, fn
    msg = eng.lib.mdp_last_error(eng.h).decode()
    assert fn in msg, msg
    return msg


def test_refusals_launch_nothing():
    """every refusal of the four entry points: host, pinned and one-float-short
    buffers on every device pointer, the bounds, the table's entries, a capturing
    stream, a handle without a device scenario -- each with a message that names
    the entry point; nothing is launched or written, and the handle still works"""
    case = "tag"
    a, _sets, bank = _bank(case)
    table = _table(case)
    n, E, M, K = a.n, 16, len(table), 3
    sf = a.actor_set_floats()
    a.prof_enable("eval")
    timed = a.prof_read("eval")[1]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda k: torch.full((k,), 7.0, dtype=torch.float32, device=a.device)  # noqa: E731
    i32 = ctypes.POINTER(ctypes.c_int32)
    tptr = lambda t: np.ascontiguousarray(t, np.int32).ctypes.data_as(i32)  # noqa: E731
    sizes = {"bank": K * sf, "u": E * T * n * ACT, "ret": M * E * n, "bench": M * E * n * _lib.BENCH_W}
    good = {k: dev(v) for k, v in sizes.items() if k != "bank"}
    good["bank"] = bank
    kept = bank.clone()
    fn = "mdp_evaluate_matchups"

    def call(n_sets=K, tab=table, matchups=None, first=0, episodes=E, mode=0, **over):
        ptr = {k: p(v) for k, v in good.items()}
        ptr.update(over)
        tab_arg = None if tab is None else tptr(tab)
        return _refused(a, fn, ptr["bank"], n_sets, tab_arg, M if matchups is None else matchups, first, episodes,
                        mode, ptr["u"], ptr["ret"], ptr["bench"])

    host = {k: np.zeros(v, np.float32) for k, v in sizes.items()}
    pinned = {k: torch.zeros(v, dtype=torch.float32).pin_memory() for k, v in sizes.items()}
    one_set = dev(sf)
    nbytes, base = 4 << 20, ctypes.c_void_p()
    assert a.lib.hipMalloc(ctypes.byref(base), ctypes.c_size_t(nbytes)) == 0
    try:
        rb, ext = ctypes.c_void_p(), ctypes.c_size_t()
        assert a.lib.hipMemGetAddressRange(ctypes.byref(rb), ctypes.byref(ext), base) == 0
        assert rb.value == base.value and ext.value == nbytes     # the extent the library checks against
        assert 4 * max(sizes.values()) < nbytes
        for k, v in sizes.items():
            assert f"{k}_dev is not device memory" in call(**{k: ctypes.c_void_p(host[k].ctypes.data)}), k
            assert f"{k}_dev is not device memory" in call(**{k: p(pinned[k])}), k
            short = ctypes.c_void_p(base.value + nbytes - 4 * (v - (4 if k == "bank" else 1)))   # (the bank stays 16-byte aligned)
            assert f"{k}_dev ends before" in call(**{k: short}), k
        flat = a._flat_params(0, "actor", _sets[0][0])
        for bad, why in ((ctypes.c_void_p(host["bank"].ctypes.data), "set_dev is not device memory"),
                         (p(pinned["bank"]), "set_dev is not device memory"),
                         (ctypes.c_void_p(base.value + nbytes - 4 * (sf - 1)), "set_dev ends before"),
                         (None, "set_dev is null")):
            assert why in _refused(a, "mdp_actor_set_snapshot", bad)
            assert why in _refused(a, "mdp_actor_set_write", bad, 0, _lib.fptr(flat), flat.size)
        assert "agent" in _refused(a, "mdp_actor_set_write", p(one_set), n, _lib.fptr(flat), flat.size)
        assert "agent" in _refused(a, "mdp_actor_set_write", p(one_set), -1, _lib.fptr(flat), flat.size)
        assert "count" in _refused(a, "mdp_actor_set_write", p(one_set), 0, _lib.fptr(flat), flat.size - 1)
        assert "src_host" in _refused(a, "mdp_actor_set_write", p(one_set), 0, None, flat.size)
    finally:
        torch.cuda.synchronize()
        assert a.lib.hipFree(base) == 0
    assert bool(torch.all(one_set == 7.0))
    assert "bank_dev is null" in call(bank=None)
    assert "ret_dev is null" in call(ret=None)
    assert "table_host is null" in call(tab=None)
    assert "16-byte aligned" in call(bank=ctypes.c_void_p(bank.data_ptr() + 4), n_sets=K - 1)
    for bad in (0, -1, 4097):
        assert "n_sets" in call(n_sets=bad)
        assert "matchups" in call(matchups=bad)
    for count in (0, -1, (1 << 20) + 1):
        assert "2^20" in call(episodes=count)
    assert "2^22" in call(matchups=4096, episodes=1025)
    for first in (-1, (1 << 32) - E + 1, 1 << 40):
        assert "uint32" in call(first=first)
    for mode in (-1, 2):
        assert "mode" in call(mode=mode)
    assert "MDP_EVAL_MEAN" in call(mode=1)
    for (m, j), v in (((0, 0), -1), ((M - 1, n - 1), K), ((2, 1), 1 << 30)):
        tab = table.copy()
        tab[m, j] = v
        msg = call(tab=tab)
        assert f"matchup {m}" in msg and f"agent {j}" in msg and "table_host" in msg, msg
    msg = call(n_sets=2)                                      # the bank's third set is out of the table's reach
    assert "table_host" in msg and "matchup 2" in msg and "agent 0" in msg
    # records where the scenario has none
    sl, _s, sl_bank = _bank("speaker_listener")
    sl_ret, sl_rec = dev(E * sl.n), dev(E * sl.n * _lib.BENCH_W)
    msg = _refused(sl, fn, p(sl_bank), K, tptr(np.zeros((1, sl.n))), 1, 0, E, 0, None, p(sl_ret), p(sl_rec))
    assert "bench_dev" in msg and "benchmark_data raises" in msg
    # a capturing stream
    stream, graph = ctypes.c_void_p(a.lib.mdp_stream(a.h)), ctypes.c_void_p()
    a.synchronize()
    torch.cuda.synchronize()
    assert a.lib.hipStreamBeginCapture(stream, 2) == 0        # hipStreamCaptureModeRelaxed
    try:
        msgs = [call(u=None, bench=None), _refused(a, "mdp_actor_set_snapshot", p(one_set))]
    finally:
        assert a.lib.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
        if graph.value:
            assert a.lib.hipGraphDestroy(graph) == 0
    assert all("capturing" in m for m in msgs), msgs
    # nothing was launched or written
    a.synchronize()
    assert a.prof_read("eval")[1] == timed
    assert all(bool(torch.all(v == 7.0)) for k, v in good.items() if k != "bank")
    assert bool(torch.all(sl_ret == 7.0)) and bool(torch.all(sl_rec == 7.0)) and torch.equal(bank, kept)
    # a handle without a device scenario
    plain = Engine([6], batch_size=16, capacity=64)
    pb = torch.zeros(plain.actor_set_floats(), dtype=torch.float32, device=plain.device)
    msg = _refused(plain, fn, p(pb), 1, tptr(np.zeros((1, 1))), 1, 0, E, 0, None, p(good["ret"]), None)
    assert "no device env" in msg
    # Python's own checks
    with pytest.raises(ValueError, match="mode"):
        a.evaluate_matchups(bank, table, E, mode="greedy")
    with pytest.raises(ValueError, match="table"):
        a.evaluate_matchups(bank, table.astype(np.int64), E)
    with pytest.raises(ValueError, match="table"):
        a.evaluate_matchups(bank, table[:, :-1], E)
    with pytest.raises(ValueError, match="bank"):
        a.evaluate_matchups(bank.view(-1)[:-4], table, E)
    with pytest.raises(ValueError, match="u: "):
        a.evaluate_matchups(bank, table, E, u=torch.zeros(E, T, n, ACT - 1))
    with pytest.raises(ValueError, match="slot"):
        a.bank_snapshot(bank.clone(), K)
    # after all of them a good call on the same handle returns the result of test 1, and is timed
    res = a.evaluate_matchups(bank, table, COUNT, FIRST, bench=True)
    want = _reference(case)
    for m in range(M):
        np.testing.assert_array_equal(res["returns"][m].cpu().numpy(), want[(m, "sample")][0])
        np.testing.assert_array_equal(res["bench"][m].cpu().numpy(), want[(m, "sample")][1])
    assert a.prof_read("eval")[1] == timed + 1
    a.prof_enable("eval", False)
