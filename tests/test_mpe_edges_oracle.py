"""CPU: the MPE oracle against values worked out by hand, and the edge states of
tests/mpe_edges.py against what they claim to be.

* ``oracle/mpe.py`` at a contact, the clamp, the boundary penalty and an occupied
  landmark gives the values derived in the comments below (none of them is
  computed by the code under test);
* the restatement of tests/mpe_edges.py in float64 is the oracle bit for bit on
  every family (spread's shared reward of eight agents: numpy adds eight terms
  pairwise, the device and the restatement one after another, so the per-agent
  rewards are compared bit for bit and the sum to 1e-13);
* the recorded yardsticks ``YARD`` are what ``measure()`` measures, family by family;
* the families meet their conditions: fp32 arrays, colliding pairs at least 1e-3
  apart, the sharpest cases on tile rows 0, 15, 16 and the last row of a ragged
  E, undecided cases at most 5 % of an indicator family, at least 8 decided
  cases on each side of every collision threshold within 2e-3 of it, all six
  off-threshold placements of every ``occupied`` set decided.
"""
import math

import numpy as np
import pytest

from tests import mpe_edges as me

F64 = np.float64
LN2 = 0.6931471805599453


def _one(sc, pos, vel, act=None):
    """one oracle step of a single env from fp64 inputs"""
    pos, vel = np.asarray(pos, F64)[None], np.asarray(vel, F64)[None]
    act = np.full((1, sc.n_agents, 5), 0.2) if act is None else np.asarray(act, F64)[None]
    with np.errstate(all="ignore"):
        nst, _obs, rew = sc.step({"pos": pos, "vel": vel, "goal": np.zeros(1, int)}, act)
    return nst["pos"][0], nst["vel"][0], rew[0]


def _spread_pair(dist):
    """spread N=3: agents 0 and 1 `dist` apart on the x axis about the origin, agent 2
    and the landmarks far away, everyone at rest"""
    pos = np.array([[dist / 2, 0], [-dist / 2, 0], [50, 50], [20, 0], [0, 20], [-20, 0]], F64)
    return pos, np.zeros((6, 2))


def test_contact_force_at_dist_equal_dmin():
    # dist = dmin = 0.15 + 0.15: x = -(dist - dmin) / k = 0, pen = k ln(1 + e^0) = k ln 2,
    # force = 100 (delta / dist) pen = 100 k ln 2 = 0.0693147... along +x on agent 0 (delta
    # = pos_0 - pos_1 points from 1 to 0) and -x on agent 1; a uniform action gives no
    # action force; at rest v' = 0.75 * 0 + F * 0.1
    sc = me.scenario("simple_spread", 3)
    pos, vel = _spread_pair(0.3)
    assert pos[0, 0] - pos[1, 0] == 0.15 + 0.15
    _p, v, _r = _one(sc, pos, vel)
    f = 100 * 1e-3 * LN2
    assert abs(v[0, 0] - f * 0.1) <= 1e-15 and v[0, 1] == 0
    assert v[1, 0] == -v[0, 0] and v[1, 1] == 0
    assert np.all(v[2:] == 0)


def test_contact_penetration_deep_and_apart():
    sc = me.scenario("simple_spread", 3)
    # depth dmin - dist = 0.25: pen = k ln(1 + e^250) = 0.25 + k ln(1 + e^-250) = 0.25 (the
    # second term is 1e-3 * 2.7e-109); force 100 * 0.25 = 25, v' = 2.5
    _p, v, _r = _one(sc, *_spread_pair(0.3 - 0.25))
    assert abs(v[0, 0] / 0.1 / 100 - 0.25) <= 0.25e-12
    assert v[1, 0] == -v[0, 0]
    # dist = dmin + 0.1: pen = k ln(1 + e^-100) = 1e-3 * 3.72e-44, force 3.72e-45 < 1e-40
    _p, v, _r = _one(sc, *_spread_pair(0.3 + 0.1))
    assert 0 < v[0, 0] / 0.1 < 1e-40 and abs(v[0, 0] / 0.1 / 3.720076e-45 - 1) < 1e-6    # e^-100 = 3.720076e-44


def test_landmark_in_contact_does_not_move():
    # tag: the good agent 3 (size 0.05) at dist = dmin = 0.25 above landmark 4 (size 0.2),
    # both collide, the landmark is not movable: the agent gets the whole 100 k ln 2 along
    # +y, the landmark nothing; 0.0069 is far below max_speed 1.3: no clamp
    sc = me.scenario("simple_tag", 4, 3)
    pos = np.array([[30, 0], [0, 30], [-30, 0], [0.25, 0.5], [0.25, 0.25], [0, -30]], F64)
    p, v, _r = _one(sc, pos, np.zeros((6, 2)))
    assert abs(v[3, 1] - 100 * 1e-3 * LN2 * 0.1) <= 1e-15 and v[3, 0] == 0
    assert np.all(p[4] == pos[4]) and np.all(v[4] == 0)
    assert np.all(v[:3] == 0) and np.all(p[5] == pos[5])


def test_momentum_change_of_a_movable_pair_sums_to_zero():
    # the pair's forces are f and -f (one value, negated), so from rest the two velocity
    # changes cancel exactly, at every depth and along a generic direction
    sc = me.scenario("simple_tag", 4, 3)
    for depth in (0.1, 1e-3, 0.0, -2e-3):
        d = 0.075 + 0.075 - depth
        u = np.array([math.cos(1.0), math.sin(1.0)])
        pos = np.array([d / 2 * u, -d / 2 * u, [-30, 0], [30, 0], [0, 30], [0, -30]], F64)
        _p, v, _r = _one(sc, pos, np.zeros((6, 2)))
        assert np.all(v[0] + v[1] == 0) and np.any(v[0] != 0)


def test_clamp():
    # tag adversary, max_speed 1, no force: v = (2, 0) damps to 1.5 > 1 and is scaled to
    # (1.5 / 1.5) * 1 = 1; v = (1.2, 0) damps to 0.9 < 1 and stays; the good agent's 1.3
    sc = me.scenario("simple_tag", 4, 3)
    pos = np.array([[30, 0], [0, 30], [-30, 0], [30, 30], [-30, -30], [0, -30]], F64)
    vel = np.zeros((6, 2))
    vel[0], vel[1], vel[3] = [2, 0], [1.2, 0], [3 * 0.6, 3 * 0.8]
    _p, v, _r = _one(sc, pos, vel)
    assert v[0, 0] == 1.0 and v[0, 1] == 0
    assert v[1, 0] == 1.2 * 0.75 and v[1, 1] == 0
    assert abs(math.hypot(*v[3]) - 1.3) <= 1e-15 and abs(v[3, 1] / v[3, 0] - 0.8 / 0.6) <= 1e-15


def test_boundary_penalty_values():
    # bound(x) of simple_tag: 0 below 0.9; (x - 0.9) * 10 up to 1; min(exp(2 x - 2), 10) from
    # 1 on, which reaches 10 at x = 1 + ln(10) / 2.  At 0.95: 0.5; at 1: e^0 = 1; at 1.5: e^1;
    # 1e-4 below the cap point: 10 e^(-2e-4) = 10 (1 - 2e-4 + 2e-8 - ...) = 9.9980002; above: 10
    sc = me.scenario("simple_tag", 4, 3)
    xs = [0.5, 0.9, 0.95, 1.0, 1.5, me.CAP_X - 1e-4, me.CAP_X + 1e-4, 3.0, 50.0]
    want = [0.0, 0.0, 0.5, 1.0, math.e, 9.9980002, 10.0, 10.0, 10.0]
    tol = [0, 0, 1e-14, 0, 1e-14, 2e-10, 0, 0, 0]
    for ax in (0, 1):
        for sg in (1, -1):
            pos = np.zeros((len(xs), 6, 2))
            pos[:, :, 0], pos[:, :, 1] = [-20, -25, -30, 0, -35, -40], [20, 25, 30, 0, 35, 40]
            pos[:, 3, ax], pos[:, 3, 1 - ax] = sg * np.array(xs), 0.3
            got = -me.oracle_reward(sc, pos)[:, 3]
            for g, w, t in zip(got, want, tol):
                assert abs(g - w) <= t, (g, w)
    assert abs(9.9980002 - 9.998) < 1e-6


def test_spread_agent_on_a_landmark_is_occupied():
    # agent 0 on landmark 0: min distance 0 (< 0.1: occupied); landmark 1 is (3, 4) from
    # agent 1: 5; landmark 2 is (6, 8) from agent 2: 10; nothing else is nearer.  min_dists
    # = 15, one landmark occupied, every agent collides with itself alone: reward -15 - 1
    sc = me.scenario("simple_spread", 3)
    pos = np.array([[0.25, -0.5], [40, 0], [0, 40], [0.25, -0.5], [43, 4], [6, 48]], F64)[None]
    rec = me.oracle_records(sc, pos)
    for i in range(3):
        assert list(rec[i][0]) == [-16.0, 1.0, 15.0, 1.0]
    assert np.all(me.oracle_reward(sc, pos) == 3 * -16.0)
    parts = me.integer_parts(sc, pos)
    assert parts["occupied"][0] == 1 and np.all(parts["coll"] == 1)


# ------------------------------------------------------------ restatements
@pytest.mark.parametrize("fid", me.FAMILY_IDS)
def test_fp64_restatement_is_the_oracle(fid):
    f = me.family(fid)
    sc = me.scenario(*f["scn"])
    p64, v64 = me.step_t(sc, f["pos"], f["vel"], f["act"], F64)
    nst, _obs, rew = me.oracle_step(sc, f["pos"], f["vel"], f["act"], f["goal"])
    assert np.array_equal(p64, nst["pos"]) and np.array_equal(v64, nst["vel"])
    if f["scn"][:2] == ("simple_spread", 8):
        with np.errstate(all="ignore"):
            assert np.array_equal(me.reward_t(sc, p64, f["goal"], F64, shared=False), sc.reward(nst))
        assert np.max(np.abs(me.reward_t(sc, p64, f["goal"], F64) - rew)) <= 1e-13
    else:
        assert np.array_equal(me.reward_t(sc, p64, f["goal"], F64), rew)
    assert np.array_equal(me.oracle_reward(sc, p64, f["goal"]), rew)
    if me.has_records(sc):
        for got, want in zip(me.bench_t(sc, p64, f["goal"], F64), sc.benchmark_data(nst)):
            assert np.array_equal(got, want)
    # the fp32 form: fp32 throughout, finite
    p32, v32 = me.step_t(sc, f["pos"], f["vel"], f["act"], np.float32)
    assert np.all(np.isfinite(p32)) and np.all(np.isfinite(v32))
    assert np.all(np.isfinite(me.reward_t(sc, p32, f["goal"], np.float32)))


@pytest.mark.parametrize("fid", me.FAMILY_IDS)
def test_yardsticks_reproduce(fid):
    got = me.measure(me.family(fid))
    print(fid, got)
    assert set(got) == set(me.YARD[fid])
    for g, qs in got.items():
        assert set(qs) == set(me.YARD[fid][g])
        for q, e in qs.items():
            y = me.YARD[fid][g][q]
            # A quarter either way: numpy's fp32 exp / log1p differ by an ulp between its SIMD
            # builds -- a property of the numpy build, not of the project.  A recorded 0 has to
            # reproduce as exactly 0: those are quantities no rounding enters (an agent at
            # rest that stays, integer counts, a penalty at its cap)
            assert 0.75 * y <= e <= 1.25 * y, (fid, g, q, e, y)


def test_yardsticks_are_far_below_the_flat_bound():
    """the table the bounds were planned on: contact grid velocities within 4e-7 at |v| <= 2.9,
    the cluster's within 2.8e-6 at |v| <= 12.5 -- 50 and 7 times below the 2e-5 of
    tests/test_gpu_parity.py::test_env_step_parity"""
    contact = [g["vel"] for fid, y in me.YARD.items() if fid.startswith("contact") for g in y.values()]
    assert len(contact) == 3 * len(me.CONTACT_PAIRS) and max(contact) < 5e-7
    assert me.YARD["cluster-simple_spread8"]["all"]["vel"] < 3e-6


# ---------------------------------------------------------------- families
@pytest.mark.parametrize("fid", me.FAMILY_IDS)
def test_family_layout(fid):
    f = me.family(fid)
    E = len(f["pos"])
    assert 18 <= E <= 208 and E % 16 != 0
    for r in (0, 15, 16, E - 1):
        assert f["order"][r] in f["sharp"]
    assert set(f["order"]) == set(range(f["order"].max() + 1))        # every case is there
    me.check_family(f)
    assert set(f["group"]) == set(me.YARD[fid])


@pytest.mark.parametrize("idx", range(len(me.CONTACT_PAIRS)))
def test_contact_grid_is_on_its_depths(idx):
    f = me.contact_family(idx)
    sc = me.scenario(*f["scn"])
    a, b = f["pair"]
    p = f["pos"].astype(F64)
    t_real = (me._dist(p, a, b) - (sc.size[a] + sc.size[b])) / me.K
    # fp32 positions in the unit box and 1.3 around it: the distance is within 3e-7 = 3e-4 k
    assert np.max(np.abs(t_real - f["meta"]["t"])) < 1e-3
    ts = set(f["meta"]["t"])
    assert {-5.0, -1.0, -0.1, 0.0, 0.1, 1.0, 5.0, 20.0, 87.0, 104.0, 1000.0} <= ts
    assert set(me.T_GRID) - ts == {t for t in me.T_GRID if sc.size[a] + sc.size[b] + me.K * t < me.MIN_SEP + 1e-6}
    d = p[:, a] - p[:, b]
    for k in range(4):                                                    # dx or dy exactly 0
        assert np.all(d[f["meta"]["dir"] == k][:, 1 - k % 2] == 0)
    assert np.all(np.all(d[f["meta"]["dir"] >= 4] != 0, axis=1))
    assert {float(f["meta"]["t"][r]) for r in (0, 15, 16, len(p) - 1)} <= {-1.0, 0.0, 1.0}


def test_cluster_contacts():
    f = me.family("cluster-simple_spread8")
    p = f["pos"].astype(F64)
    touching = sum((me._dist(p, a, b) < 0.3).astype(int) for a in range(8) for b in range(a + 1, 8))
    assert np.median(touching) == 28 and touching.min() >= 24
    assert 0.05 == f["meta"]["r"].min() and f["meta"]["r"].max() == 0.149


def test_clamp_and_boundary_inputs():
    f = me.family("clamp-simple_tag4")
    sc = me.scenario(*f["scn"])
    sp = np.sqrt((f["vel"].astype(F64) ** 2).sum(-1))[:, :4] * 0.75 / np.array(sc.max_speed[:4]) - 1
    assert np.max(np.abs(sp - f["meta"]["delta"][:, None])) < 2e-7 * (1 + np.abs(f["meta"]["delta"]).max())
    assert set(me.CLAMP_DELTAS) == set(f["meta"]["delta"])
    nst, _o, _r = me.oracle_step(sc, f["pos"], f["vel"], f["act"])
    assert np.array_equal(nst["vel"][:, 4:], f["vel"][:, 4:])
    speed = np.sqrt((nst["vel"] ** 2).sum(-1))[:, :4]
    assert np.all(speed <= np.array(sc.max_speed[:4]) * (1 + 1e-15))
    b = me.family("boundary-simple_tag4")
    x = np.abs(b["pos"][np.arange(len(b["pos"])), 3, b["meta"]["axis"]])
    assert np.array_equal(x, b["meta"]["x"].astype(np.float32)) and x.max() == 1e4
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(2) * x.max() - np.float32(2)))   # expf overflows before the min
    nst, _o, _r = me.oracle_step(sc, b["pos"], b["vel"], b["act"])
    assert np.array_equal(nst["pos"], b["pos"]) and np.all(nst["vel"] == 0)       # at rest: it stays


def test_occupied_sets_are_decided():
    f = me.family("occupied-simple_spread3")
    sc = me.scenario(*f["scn"])
    nst, _o, _r = me.oracle_step(sc, f["pos"], f["vel"], f["act"])
    assert np.array_equal(nst["pos"], f["pos"])                                   # nothing moves
    ok = me.decided(sc, nst["pos"])
    off, occ = f["meta"]["offset"], me.integer_parts(sc, nst["pos"])["occupied"]
    for s in set(f["meta"]["set"]) - {-1}:
        m = (f["meta"]["set"] == s) & ~np.isnan(off)
        assert set(off[m]) == set(me.OCC_OFFSETS) and np.all(ok[m])
        assert np.array_equal(occ[m], (off[m] < 0).astype(int))
    tie = f["meta"]["tie"]                                       # on the fp32 threshold: not occupied under `<`
    assert tie.sum() == 1 and not ok[tie].any() and f["tie_thr"] == np.float32(0.1)
    assert np.all(me._dist(f["pos"], 0, 3)[tie] == f["tie_thr"])
    assert np.all(me.bench_t(sc, f["pos"], f["goal"], np.float32)[0][tie, 3] == 0)
    assert not any(tie[r] for r in (0, 15, 16, len(tie) - 1))
    on = np.isnan(off)
    assert np.all(me._dist(f["pos"].astype(F64), 0, 3)[on] == 0) and np.all(occ[on] == 1) and np.all(ok[on])
    assert (~ok).mean() <= 0.05


@pytest.mark.parametrize("idx", range(len(me.SWEEP_PAIRS)))
def test_collision_sweeps_cover_both_sides(idx):
    f = me.sweep_family(idx)
    sc = me.scenario(*f["scn"])
    a, b = f["pair"]
    nst, _o, _r = me.oracle_step(sc, f["pos"], f["vel"], f["act"])
    gap = me._dist(nst["pos"], a, b) - (sc.size[a] + sc.size[b])
    assert gap.min() < -0.08 and 4e-3 < gap.max() <= me.SWEEP_GAP0 + 1e-4
    ok = np.abs(gap) > me.DECIDE
    assert np.sum(ok & (gap > 0) & (gap < 2e-3)) >= 8 and np.sum(ok & (gap < 0) & (gap > -2e-3)) >= 8
    assert (~ok).mean() <= 0.05 and (~me.decided(sc, nst["pos"])).mean() <= 0.05
    assert np.sum(ok & (np.abs(gap) < 5e-5)) >= 4                 # and decided cases within 5e-5 of it
    tie = f["meta"]["tie"]
    indicator = sc.name == "simple_spread" or sc.adversary[a] != sc.adversary[b]
    assert tie.sum() == (me.TIES if indicator else 0)
    if tie.any():                                                 # on the fp32 threshold: no collision under `<`
        p32, _ = me.step_t(sc, f["pos"], f["vel"], f["act"], np.float32)
        thr = np.float32(sc.size[a]) + np.float32(sc.size[b])
        assert thr == f["tie_thr"] == np.float32(sc.size[a] + sc.size[b])
        assert np.all(me._dist(p32, a, b)[tie] == thr) and np.all(np.abs(gap[tie]) < me.DECIDE)
        rec = me.bench_t(sc, p32, f["goal"], np.float32)[a]
        assert np.all(rec[tie, 1] == 1) if sc.name == "simple_spread" else np.all(rec[tie, 0] == 0)
        assert not any(tie[r] for r in (0, 15, 16, len(tie) - 1))
    ind = me.indicator_margins(sc, nst["pos"])
    if sc.adversary[a] == sc.adversary[b] and sc.name == "simple_tag":
        assert np.all(ind > 1)                                    # two adversaries: no indicator of tag's
    else:
        assert np.any(np.all(ind == gap[:, None], axis=0))        # the pair's own margin is one of them


@pytest.mark.parametrize("idx", range(len(me.PLAIN)))
def test_plain_family_cases(idx):
    f = me.plain_family(idx)
    name, n, na = f["scn"]
    sc = me.scenario(name, n, na)
    src = f["order"]
    p, L = f["pos"].astype(F64), sc.n_landmarks
    assert np.abs(p[np.isin(src, [0, 1, 2, 3])]).max() > 900
    assert {int(g) for g in f["goal"]} >= {0, L - 1}
    mover = 1 if name == "simple_speaker_listener" else 0
    for c in (10, 11):
        r = int(np.argmax(src == c))
        assert np.all(p[r, mover] == p[r, n + f["goal"][r]])
    if name == "simple_adversary":
        for c in (12, 13):
            r = int(np.argmax(src == c))
            d = [me._dist(p[r:r + 1], i, n + int(f["goal"][r]))[0] for i in range(na, n)]
            assert d[0] == d[-1] == min(d) and sorted(d)[2 if n > 3 else 1] >= d[0]
            one = slice(r, r + 1)
            nst, _o, _r = me.oracle_step(sc, f["pos"][one], f["vel"][one], f["act"][one], f["goal"][one])
            assert np.array_equal(nst["pos"][0], p[r])                        # at rest: the tie stays


def test_copied_entries():
    sp = me.copied_entries(me.scenario("simple_spread", 3))
    assert all(list(m) == [True] * 4 + [False] * 10 + [True] * 4 for m in sp)
    tag = me.copied_entries(me.scenario("simple_tag", 4, 3))
    assert [int(m.sum()) for m in tag] == [6, 6, 6, 4]
    assert not any(m.any() for m in me.copied_entries(me.scenario("simple_adversary", 3, 1)))
    sl = me.copied_entries(me.scenario("simple_speaker_listener"))
    assert sl[0].all() and list(sl[1]) == [True] * 2 + [False] * 6 + [True] * 3
