"""GPU: the MPE step (env_physics_tile, env_reward, env_bench, env_obs through
k_rollout) on the edge states of tests/mpe_edges.py, and the episode ends of
envs that are not in lockstep.

The bound of every quantity is ``mpe_edges.bound``: FACTOR (4) times what the
numpy fp32 restatement of the same step differs from the fp64 oracle by on that
family and case group (``mpe_edges.YARD``, measured on the CPU), or one
fp32 spacing of the oracle's value where that is larger -- a different but
equally valid rounding order passes, a wrong branch, a fast-math transcendental
at a deep contact or a force with the wrong sign does not.  Rewards and records
are judged against the oracle on the *device's* post-physics state, so the
physics' rounding cannot move an indicator; on cases whose indicator distances
are all more than 1e-6 from their thresholds (``decided``) the counts are exact.

Measured on MI355X (worst |device - oracle| per family, group and quantity beside
the yardstick; the tests print them as FIG lines): see DESIGN.md 15.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd.engine import Engine  # noqa: E402
from maddpg_amd.envs import bench_record, spec  # noqa: E402
from oracle import philox  # noqa: E402
from tests import mpe_edges as me  # noqa: E402
from tests.helpers import row_layout  # noqa: E402

ACT = 5
F64 = np.float64


def _spec(scn):
    name, n, na = scn
    return spec(name) if name in ("simple", "simple_speaker_listener") else spec(name, n, na if na else None)


def _engine(scn, E, H=64, **kw):
    sp = _spec(scn)
    kw.setdefault("max_episode_len", 25)
    kw.setdefault("seed", 3)
    return sp, Engine(sp.obs_dims, num_units=H, batch_size=16, capacity=1000, num_envs=E, scenario=scn[0],
                      num_adversaries=sp.num_adversaries, **kw)


def _obs(sc, pos, vel, goal, comm0=None):
    """the oracle's observations of a state (speaker-listener: comm0 is the speaker's state.c)"""
    comm = None
    if sc.name == "simple_speaker_listener":
        comm = np.zeros((len(pos), 2, 3))
        if comm0 is not None:
            comm[:, 0] = comm0
    return sc.observation(me.oracle_state(pos, vel, goal, comm))


def _check_obs(got, want, copied, what):
    """a difference is one fp32 subtraction: within one spacing of the fp64 difference of
    the same fp32 state; a copied entry is exact"""
    want32 = want.astype(np.float32)
    err = np.abs(got.astype(F64) - want)
    assert np.all(err <= np.spacing(np.abs(want32)).astype(F64)), (what, float(err.max()))
    assert np.array_equal(got[:, copied], want32[:, copied]), what


def _ties(f, pos):
    """the family's tie cases: on the device's post-state too, every one of them has the
    pair's fp32 distance (dy = 0: |dx|, one fp32 subtraction) equal to the fp32 threshold.
    MPE's `<` says no there, whatever the fp64 distance of those fp32 positions is"""
    a, b = f["pair"]
    tie = f["meta"]["tie"]
    exact = (pos[:, a, 1] == pos[:, b, 1]) & (np.abs(pos[:, a, 0] - pos[:, b, 0]) == f["tie_thr"])
    assert np.all(exact[tie]), "a tie case is off the threshold on the device"
    return tie


def _report(fid, H, q, err, group, ok=None):
    """one line per case group: the device's worst error beside the family's yardstick"""
    for g in np.unique(group):
        m = (group == g) if ok is None else (group == g) & ok
        worst = float(err[m].max()) if m.any() else 0.0
        print(f"FIG {fid} {H} {q} {g} {worst:.3e} {me.YARD[fid][g][q]:.3e}")


def _cases():
    out = []
    for fid in me.FAMILY_IDS:
        out.append((fid, 64))
        if "spread" in fid or "tag" in fid:
            out.append((fid, 128))              # the two k_rollout instantiations carve LDS differently
    return out


@pytest.mark.parametrize("fid,H", _cases())
def test_step_on_edge_states(fid, H):
    """one env_step(act_in) from the family's state: positions, velocities, the replay
    row's obs / act / obs' / reward / done, everything finite"""
    f = me.family(fid)
    sc = me.scenario(*f["scn"])
    E, n = len(f["pos"]), sc.n_agents
    sp, eng = _engine(f["scn"], E, H)
    eng.env_reset()
    eng.set_env_state(f["pos"], f["vel"], f["goal"])
    eng.env_step(act_in=torch.from_numpy(f["act"]))
    got = eng.env_state()
    rows = eng.replay_rows(0, E).cpu().numpy()
    assert np.all(np.isfinite(got["pos"])) and np.all(np.isfinite(got["vel"])) and np.all(np.isfinite(rows))
    assert np.all(got["ep_step"] == 1) and np.array_equal(got["goal"], f["goal"]) and eng.buffer_len() == E

    nst, _obs1, _rew = me.oracle_step(sc, f["pos"], f["vel"], f["act"], f["goal"])
    for q in ("pos", "vel"):
        err = np.abs(got[q].astype(F64) - nst[q])
        b = me.bound(f, q, nst[q])
        _report(fid, H, q, err.reshape(E, -1).max(1), f["group"])
        assert np.all(err <= b), (q, float((err / b).max()), int(np.argmax((err / b).reshape(E, -1).max(1))))

    # the row: obs of the set state, the injected actions, obs' of the device's own post-state
    lay, _ = row_layout(sp.obs_dims)
    copied = me.copied_entries(sc)
    said = f["act"][:, 0, :3].astype(F64)
    obs0 = _obs(sc, f["pos"], f["vel"], f["goal"])
    obs1 = _obs(sc, got["pos"], got["vel"], f["goal"], said)
    for j in range(n):
        lj, o = lay[j], sp.obs_dims[j]
        _check_obs(rows[:, lj["obs"]:lj["obs"] + o], obs0[j], copied[j], f"obs {j}")
        _check_obs(rows[:, lj["nobs"]:lj["nobs"] + o], obs1[j], copied[j], f"obs' {j}")
        assert np.array_equal(rows[:, lj["act"]:lj["act"] + ACT], f["act"][:, j])
        assert np.all(rows[:, lj["done"]] == 0)

    # rewards against the oracle on the device's post-state
    ok = me.decided(sc, got["pos"])
    assert (~ok).mean() <= 0.05
    if fid.startswith("sweep"):                                 # both sides of the threshold, decided, within 2e-3
        a, b = f["pair"]
        gap = me._dist(got["pos"].astype(F64), a, b) - (sc.size[a] + sc.size[b])
        far = np.abs(gap) > me.DECIDE
        assert np.sum(far & (gap > 0) & (gap < 2e-3)) >= 8 and np.sum(far & (gap < 0) & (gap > -2e-3)) >= 8
    if fid.startswith("occupied"):                              # all six off-threshold placements of every set
        off = f["meta"]["offset"]
        for s in set(f["meta"]["set"]) - {-1}:
            m = (f["meta"]["set"] == s) & ~np.isnan(off)
            assert set(off[m]) == set(me.OCC_OFFSETS) and np.all(ok[m])
    want = me.oracle_reward(sc, got["pos"], f["goal"])
    rew = np.stack([rows[:, lay[j]["rew"]] for j in range(n)], 1)
    b = me.bound(f, "rew", want)
    err = np.abs(rew.astype(F64) - want)
    _report(fid, H, "rew", err.max(1), f["group"], ok)
    print(f"UNDECIDED {fid} {H} step {int((~ok).sum())} of {E}")
    assert np.all(err[ok] <= b[ok]), float((err[ok] / b[ok]).max())
    if sc.name in ("simple_spread", "simple_tag"):
        assert b.max() < 0.25                                   # so a count that is off by one fails above
    if sc.name == "simple_tag":                                 # the +-10 multiples, exactly
        parts = me.integer_parts(sc, got["pos"])
        for i in range(n):
            if sc.adversary[i]:
                assert np.array_equal(rew[ok, i], 10.0 * parts["caught"][ok])
    if "tie" in f["meta"] and f["meta"]["tie"].any():           # on the threshold itself: the strict inequality
        tie = _ties(f, got["pos"])
        want32 = me.reward_t(sc, got["pos"], f["goal"], np.float32).astype(F64)
        assert np.all(np.abs(rew.astype(F64) - want32)[tie] <= b[tie]) and b[tie].max() < 0.25
        print(f"TIES {fid} {H} {int(tie.sum())}")


def _record_cases():
    out = [(fid, 64) for fid in me.FAMILY_IDS if me.has_records(me.scenario(*me.family(fid)["scn"]))]
    return out + [("sweep-simple_spread3-01", 128), ("sweep-simple_tag4-03", 128)]


@pytest.mark.parametrize("fid,H", _record_cases())
def test_records_on_edge_states(fid, H):
    """env_step_bench from the family's state with all-zero actors and u = 0.5 (every
    action entry the same: no action force): the benchmark_data records against the
    oracle on the device's post-state; the counts exact on decided cases"""
    f = me.family(fid)
    sc = me.scenario(*f["scn"])
    E, n = len(f["pos"]), sc.n_agents
    sp, eng = _engine(f["scn"], E, H)
    for i in range(n):
        eng.set_params(i, "actor", {k: np.zeros_like(v) for k, v in eng.get_params(i, "actor").items()})
    eng.env_reset()
    eng.set_env_state(f["pos"], f["vel"], f["goal"])
    info = eng.env_step_bench(u=torch.full((E, n, ACT), 0.5)).cpu().numpy()
    got = eng.env_state()
    rows = eng.replay_rows(0, E).cpu().numpy()
    lay, _ = row_layout(sp.obs_dims)
    for j in range(n):      # five equal entries (1 x rcp(5): 0.2 to the hardware reciprocal's ulp): no action force
        a = rows[:, lay[j]["act"]:lay[j]["act"] + ACT]
        assert np.all(a == a[:, :1]) and np.all(np.abs(a - np.float32(0.2)) <= 2 * np.spacing(np.float32(0.2)))
    assert np.all(np.isfinite(info)) and np.all(np.isfinite(got["pos"]))
    ok = me.decided(sc, got["pos"])
    assert (~ok).mean() <= 0.05
    want = me.oracle_records(sc, got["pos"], f["goal"])
    parts = me.integer_parts(sc, got["pos"])
    tie = _ties(f, got["pos"]) if "tie" in f["meta"] and f["meta"]["tie"].any() else None
    rec32 = me.bench_t(sc, got["pos"], f["goal"], np.float32)
    worst = np.zeros(E)
    for i in range(n):
        w = want[i]
        width = w.shape[1]
        assert np.all(info[:, i, width:] == 0)
        err = np.abs(info[:, i, :width].astype(F64) - w)
        b = me.bound(f, "rec", w)
        worst = np.maximum(worst, err.max(1))
        assert np.all(err[ok] <= b[ok]), (i, float((err[ok] / b[ok]).max()))
        if sc.name == "simple_spread":
            assert b.max() < 0.25
            assert np.array_equal(info[ok, i, 1], parts["coll"][ok, i]) and np.array_equal(info[ok, i, 3],
                                                                                            parts["occupied"][ok])
            assert np.all(err[:, 2] <= b[:, 2])             # min_dists has no indicator in it: every case
        if sc.name == "simple_tag":
            assert np.array_equal(info[ok, i, 0], parts["tags"][ok, i])
        if tie is not None:       # on the threshold itself: the counts of the strict inequality (the fp32 form's)
            for col in ((1, 3) if sc.name == "simple_spread" else (0,)):
                assert np.array_equal(info[tie, i, col], rec32[i][tie, col])
        for e in range(0, E, 7):
            assert type(bench_record(sp, info[e, i], i)) is type(sc.record(w[e], i))
    _report(fid, H, "rec", worst, f["group"], ok)
    print(f"UNDECIDED {fid} {H} records {int((~ok).sum())} of {E}")


# ------------------------------------------------------- episode ends
def _match_rows(got, want, rtol, atol):
    """got and want hold the same rows in some order (each want row takes the nearest unused got row)"""
    assert got.shape == want.shape
    free = list(range(len(got)))
    for w in want:
        tol = atol + rtol * np.abs(w)
        d = [np.max(np.abs(got[k] - w) / tol) for k in free]
        k = int(np.argmin(d))
        assert d[k] <= 1.0, (w, got[free[k]])
        free.pop(k)


@pytest.mark.parametrize("name,n,na", [("simple_spread", 3, 0), ("simple_tag", 4, 3)])
def test_staggered_episode_ends(name, n, na):
    """envs at unequal episode steps (mdp_env_set_state clears the lockstep flag, the
    log goes in arrival order): every step the envs at the last episode step log
    their summed rewards, store a terminal row (done 0, obs' of the post-physics
    state) and restart from the scenario's reset on Philox stream 0x20000 at the
    step's counter; a fresh env_reset() logs in env order again"""
    sc = me.scenario(name, n, na)
    E, T, seed, ne = 37, 4, 0x5EED0123456789AB, sc.n_entities
    sp, eng = _engine((name, n, na), E, max_episode_len=T, seed=seed)
    lay, _ = row_layout(sp.obs_dims)
    rng = np.random.default_rng(17)
    # the bound of test_env_episode_reset_and_log for the logged sums
    rtol, atol = 1e-5, 1e-4
    # obs' against the oracle's step from the device's pre-state: two entities, each within
    # FACTOR x the contact families' yardstick
    y = max(max(g["pos"], g["vel"]) for fid, fy in me.YARD.items() if fid.startswith("contact") for g in fy.values())
    tol_nobs = 2 * me.FACTOR * y

    eng.env_reset()
    st = eng.env_state()
    eng.set_env_state(st["pos"], st["vel"], st["goal"], ep_step=np.arange(E) % T)
    acc = np.zeros((E, n))
    count, c, logged = 0, 0, np.zeros((0, 1 + n), np.float32)
    reset_obs = None                       # (envs, observations) of the last step's restarted envs
    for step in range(T):
        pre = eng.env_state()
        assert np.array_equal(pre["ep_step"], (np.arange(E) + step) % T)
        act = me._softmax_actions(rng, E, n)
        nst, obs1, _rew = me.oracle_step(sc, pre["pos"], pre["vel"], act, pre["goal"])
        eng.env_step(act_in=torch.from_numpy(act))
        term = np.flatnonzero(pre["ep_step"] + 1 >= T)
        assert len(term) in (9, 10)
        rows = eng.replay_rows(step * E, E).cpu().numpy()
        post = eng.env_state()
        for j in range(n):
            lj, o = lay[j], sp.obs_dims[j]
            assert np.all(rows[:, lj["done"]] == 0)
            # every row's obs', the terminal rows' too, is of the post-physics state
            assert np.max(np.abs(rows[:, lj["nobs"]:lj["nobs"] + o] - obs1[j])) <= tol_nobs
            if reset_obs is not None:       # the restarted envs' next obs: of the reset state
                envs, want = reset_obs
                got_o = rows[envs, lj["obs"]:lj["obs"] + o]
                assert np.max(np.abs(got_o - want[j])) <= 2e-6
                assert np.all(got_o[:, :2] == 0)            # spread and tag: the agent's own velocity
            acc[:, j] += rows[:, lj["rew"]]
        # the restart: reset_world on stream 0x20000 at this step's counter
        u = philox.slot_uniforms(seed, 0x20000, c, term, 2 * ne + 1)
        want = sc.reset(philox.ResetStream(u, ne), len(term))
        np.testing.assert_allclose(post["pos"][term], want["pos"], rtol=0, atol=1e-6)
        assert np.all(post["vel"][term] == 0)
        keep = np.setdiff1d(np.arange(E), term)
        assert np.max(np.abs(post["pos"][keep] - nst["pos"][keep])) <= tol_nobs / 2
        reset_obs = (term, sc.observation(me.oracle_state(want["pos"], want["vel"])))
        assert np.array_equal(post["ep_step"], (np.arange(E) + step + 1) % T)
        # the log: the count, the new rows behind all earlier ones, as a set the terminated envs' sums
        assert eng.episode_count() == count + len(term)
        assert np.array_equal(eng.episode_log(0, count), logged)
        new = eng.episode_log(count, len(term))
        _match_rows(new.astype(F64), np.concatenate([acc[term].sum(1, keepdims=True), acc[term]], 1), rtol, atol)
        np.testing.assert_allclose(new[:, 0], new[:, 1:].astype(F64).sum(1), rtol=rtol, atol=atol)
        if name == "simple_spread":
            assert len({float(x) for x in new[:, 0]}) == len(term)   # distinct sums: the matching is one to one
        logged = np.concatenate([logged, new])
        count += len(term)
        acc[term] = 0
        c += 1
    assert count == E                                            # every env ended once

    # in lockstep again: one whole episode logs in env order
    eng.env_reset()
    acc = np.zeros((E, n))
    for step in range(T):
        eng.env_step(act_in=torch.from_numpy(me._softmax_actions(rng, E, n)))
        rows = eng.replay_rows((T + step) * E, E).cpu().numpy()
        acc += np.stack([rows[:, lay[j]["rew"]] for j in range(n)], 1)
        assert eng.episode_count() == (count if step < T - 1 else count + E)
    log = eng.episode_log(count, E)
    np.testing.assert_allclose(log[:, 1:], acc, rtol=rtol, atol=atol)
    np.testing.assert_allclose(log[:, 0], acc.sum(1), rtol=rtol, atol=atol)
    assert np.array_equal(eng.episode_log(0, count), logged)
    post = eng.env_state()
    u = philox.slot_uniforms(seed, 0x20000, 2 * T - 1, np.arange(E), 2 * ne + 1)
    np.testing.assert_allclose(post["pos"], sc.reset(philox.ResetStream(u, ne), E)["pos"], rtol=0, atol=1e-6)
    assert np.all(post["ep_step"] == 0)
