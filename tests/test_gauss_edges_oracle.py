"""CPU: the edge inputs of tests/gauss_edges.py are what they claim to be, and the
float32 restatement they are measured with is exact where the device is.

* box_actions.box_muller reduces 2 u1 as sincospi does: u1 in {0, 1/4, 1/2, 3/4}
  gives exact 0 and +-r in float32 and in float64 (before the fix cos(pi / 2) was
  6.1e-17, and a sample under logstd = 80 held 3.99e18 where the truth is the
  mean); NaN in u[2:5] changes no bit; the moments of a million draws stand;
* the grids meet their conditions (check_inputs);
* the yardstick: the float32 restatement against the float64 reference on
  grid(2).  Measured: plain 1.43e-7 relative over the entries of scale >= FLT_MIN
  and 2.10 units of 2^-149 over the denormal ones (mean 0 at logstd -100),
  squashed 2.34e-7 absolute, 1 - a^2 1.28e-7 absolute; the recorded E32_* are
  those figures and the GPU tests bound the device by 2 x them;
* the factor S_UPDATE = 16 of the saturated update case is the one its three
  conditions select (figures beside it in tests/gauss_edges.py);
* what the restatement does at logstd = 89, where expf gives inf -- written down
  for the device tests to agree with: plain sample +-inf, eps 0 NaN (inf * 0),
  squashed sample +-1 and squashed dlogstd NaN (0 * inf).
"""
import numpy as np
import pytest

from oracle import nets
from tests import box_actions as ba
from tests import box_squash as bs
from tests import gauss_edges as gs
from tests import gumbel_edges as ge

F32 = np.float32


@pytest.mark.parametrize("d", [1, 2])
def test_grid_conditions(d):
    head, u = gs.grid(d)
    assert head.dtype == u.dtype == F32 and head.shape == (7 * 7 * 9 + 6, 2 * d) and u.shape == (len(head), 5)
    gs.check_inputs(head, u, d, pairs=True)          # (grid() asserts them too)
    assert np.array_equal(head * F32(128), np.round(head * F32(128)))       # multiples of 1 / 128
    zero = gs.eps_is_zero(u, d)
    assert zero.any() and not zero.all()
    # the ends of the device's grid: u01 of the smallest and the largest 23-bit mantissa
    from oracle import philox
    ends = philox.u01(np.array([0, 1 << 9, 0xFFFFFFFF], np.uint32))
    assert list(ends) == [gs.U0[0], gs.U0[1], gs.U0[6]] and gs.U1[6] == gs.U0[6]
    # the head table through the exact actor, as the kernels will see it
    p = gs.head_actor(18, 64, d)
    assert np.array_equal(nets.mlp_fwd(p, ge.obs_for(head, 18))[0], head)
    bad = head.copy()
    bad[3, d] = 89.0
    with pytest.raises(AssertionError):
        gs.check_inputs(bad, u, d)


@pytest.mark.parametrize("agent", range(6))
def test_rollout_rows_conditions(agent):
    head, u = gs.rollout_rows(17, agent)
    gs.check_inputs(head, u, 2)
    a, se, _t = gs.reference(head, u, 2, False)
    assert np.isfinite(a).all() and abs(se[-1, 0]) > 3e35
    p = gs.head_actor(18, 64, 2, drive=[0, 1, 2, 3])
    assert np.array_equal(nets.mlp_fwd(p, ge.obs_for(head, 18, drive=[0, 1, 2, 3]))[0], head)


def test_rollout_positions_differ_between_agents():
    pos = np.stack([gs.rollout_rows(17, j)[0][:, 2:4] for j in range(6)], 1)     # [E, n, 2]
    for a in range(6):
        for b in range(a + 1, 6):
            assert np.all(np.abs(pos[:, a] - pos[:, b]).max(-1) > 0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_box_muller_is_exact_at_the_quarter_turns(dt):
    u0 = np.repeat(gs.U0, 4)
    u1 = np.tile(np.array([0.0, 0.25, 0.5, 0.75], F32), len(gs.U0))
    with np.errstate(under="ignore"):
        eps = ba.box_muller(np.stack([u0, u1], -1), dt)
    r = np.sqrt(dt(-2) * np.log(dt(1) - u0.astype(dt)))
    assert eps.dtype == dt
    want_c = np.tile(np.array([1.0, 0.0, -1.0, 0.0], dt), len(gs.U0)) * r
    want_s = np.tile(np.array([0.0, 1.0, 0.0, -1.0], dt), len(gs.U0)) * r
    assert np.array_equal(eps[:, 0], want_c) and np.array_equal(eps[:, 1], want_s)
    # the issue's example: mean 0.5, u0 = 0.5, u1 = 0.25 -- the sample is the mean at any std
    for logstd in (20.0, 80.0):
        flat = np.array([[0.5, logstd]], dt)
        assert ba.gaussian_sample(flat, np.array([[0.5, 0.25]], F32), 1, dt)[0][0, 0] == 0.5
    # on the 7 x 7 grid of edge uniforms: the exact zeros of the float64 form, in both types
    g0, g1 = np.meshgrid(gs.U0, gs.U1, indexing="ij")
    grid_eps = ba.box_muller(np.stack([g0.ravel(), g1.ravel()], -1), dt)
    assert np.count_nonzero(grid_eps == 0) == 38
    assert np.array_equal(grid_eps == 0, gs.eps_is_zero(np.stack([g0.ravel(), g1.ravel()], -1), 2))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_box_muller_reads_two_uniforms_and_keeps_its_moments(dt):
    _head, u = gs.grid(2)
    filled = u.copy()
    filled[:, 2:] = 0.25
    a, b = ba.box_muller(u, dt), ba.box_muller(filled, dt)
    assert np.array_equal(a.view(np.uint32 if dt is np.float32 else np.uint64),
                          b.view(np.uint32 if dt is np.float32 else np.uint64))
    # away from the quarter turns the change is rounding: against the plain float64 form
    rng = np.random.default_rng(7)
    top = np.nextafter(F32(1), F32(0))
    uu = np.minimum(rng.uniform(size=(1_000_000, 2)).astype(F32), top)
    eps = ba.box_muller(uu, dt).astype(np.float64)
    r = np.sqrt(dt(-2) * np.log(dt(1) - uu[:, 0].astype(dt)))
    t = np.pi * (2.0 * uu[:, 1].astype(np.float64))        # the form before the fix
    plain = np.stack([r * np.cos(t).astype(dt), r * np.sin(t).astype(dt)], -1).astype(np.float64)
    # sin / cos moved by ~1e-16 (the old argument, up to 2 pi, carried half an ulp of 2 pi = 4.4e-16 of
    # its own): in float32 at most one rounding of the factor and one of the product, in float64 a few ulp
    k = 2 if dt is np.float32 else 8
    assert np.all(np.abs(eps - plain) <= k * np.finfo(dt).eps * r[:, None].astype(np.float64))
    # a million uniforms: mean 0, variance 1, no correlation, the normal's fourth moment
    se = 1e-3
    assert np.all(np.abs(eps.mean(0)) < 5 * se) and np.all(np.abs(eps.var(0) - 1) < 5 * 1.5 * se)
    assert abs(np.mean(eps[:, 0] * eps[:, 1])) < 5 * se and np.all(np.abs((eps ** 4).mean(0) - 3) < 5 * 10 * se)


def test_baseline_e32():
    rel, den, ab, tt = gs.baseline_e32(2)
    print(f"e32 on grid(2): plain rel {rel:.3e}, denormal rows {den:.3f} x 2^-149, squashed abs {ab:.3e}, "
          f"1 - a^2 abs {tt:.3e}")
    for got, rec in ((rel, gs.E32_PLAIN_REL), (den, gs.E32_DENORM), (ab, gs.E32_SQ_ABS), (tt, gs.E32_T_ABS)):
        assert 0.9 * rec <= got <= 1.1 * rec, (got, rec)
    r1, d1, a1, t1 = gs.baseline_e32(1)               # the narrower form is no worse
    assert r1 <= rel and d1 <= den and a1 <= ab and t1 <= tt
    # the entries judged in the absolute are the zero means at logstd -100, and only those
    head, u = gs.grid(2)
    _a, se, _t = gs.reference(head, u, 2, False)
    small = np.abs(head[:, :2].astype(np.float64)) + np.abs(se) < gs.FLT_MIN
    assert small.sum() == 52 and np.all(head[:, :2][small] == 0)
    live = small & (se != 0)                              # the rest: eps exactly 0, the sample an exact 0
    assert live.sum() == 9 and np.all(head[:, 2:][live] == -100)
    # the restatement on the grid: finite, the mean itself where eps is 0, inside the bounds
    head, u = gs.grid(2)
    zero = gs.eps_is_zero(u, 2)
    plain, sq = gs.restatement(head, u, 2, False), gs.restatement(head, u, 2, True)
    assert np.isfinite(plain).all() and np.isfinite(sq).all() and np.abs(sq).max() == 1.0
    assert np.array_equal(plain[zero], head[:, :2][zero])
    assert np.array_equal(sq[zero], np.tanh(head[:, :2])[zero])
    # 1 - a^2 relative to t is unbounded by construction near |z| = 9
    _a, _se, t = gs.reference(head, u, 2, True)
    t32 = (F32(1) - sq * sq).astype(np.float64)
    near = (t > 0) & (t < 1e-6)
    assert near.any() and (np.abs(t32 - t)[near] / t[near]).max() >= 1.0


@pytest.mark.parametrize("name", list(gs.UPDATE_CASES))
def test_update_factor_conditions(name):
    s = gs.S_UPDATE
    c = gs.saturated_case(name)
    gap, ones, hmax = gs.oracle_gap(c)
    ulp = ge.largest_weight_ulp(c)
    print(f"{name} s={s}: fp32/fp64 restatement gradient gap {gap:.3e}, {ones} squashed entries at +-1.0f, "
          f"max |head| {hmax:.2f}, weight ulp {ulp:.2e}, edge rows {[int(r) for r in c['edge_rows']]}")
    assert ones >= 1
    assert gap <= gs.GRAD_BOUND / 4
    assert 0.5 * gs.S_UPDATE_GAPS[name] <= gap <= 2 * gs.S_UPDATE_GAPS[name]      # the recorded figure
    assert ulp <= gs.WEIGHT_BOUND / 2
    assert hmax <= gs.LOGSTD_MAX                          # within the range the forward tests cover
    B = c["B"]
    assert {int(r) // 16 for r in c["edge_rows"]} == set(range((B + 15) // 16))
    for i in range(2):
        for blk in list(c["u_tgt"][i]) + [c["u_act"][i]]:
            e = blk[c["edge_rows"]]
            assert set(map(tuple, e[:, :2])) <= set(map(tuple, gs.EDGE_U)) and np.isnan(e[:, 2:]).all()
            others = np.delete(blk, c["edge_rows"], 0)
            assert others.min() >= 1e-6 and others.max() < 1
    # the next power of two fails a condition on one of the cases
    fails = []
    for other in gs.UPDATE_CASES:
        c2 = gs.saturated_case(other, 2 * s)
        gap2, _ones2, _h = gs.oracle_gap(c2)
        fails.append(not gap2 <= gs.GRAD_BOUND / 4 or ge.largest_weight_ulp(c2) > gs.WEIGHT_BOUND / 2)
    assert any(fails)


def test_what_the_restatement_does_at_an_infinite_std():
    """logstd = 89: expf overflows (88.73 is the last finite one).  The reference has
    no clamp on logstd (distributions.py:343-371) and no squash; these are the
    restatement's values, which the device is held to (test_gauss_edges_gpu.py)."""
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.isfinite(np.exp(F32(88.7))) and np.isinf(np.exp(F32(88.73))) and np.isinf(np.exp(F32(89)))
        flat = np.array([[0.5, -0.5, 89.0, 89.0]] * 3, F32)
        u = np.array([[0.5, 0.125], [0.5, 0.25], [0.0, 0.125]], F32)
        a, se = ba.gaussian_sample(flat, u, 2, F32)
        assert a[0, 0] == np.inf and a[0, 1] == np.inf and np.all(np.isinf(se[0]))      # eps != 0: +-inf
        assert np.isnan(a[1, 0]) and a[1, 1] == np.inf                              # cos = 0: inf * 0
        assert np.isnan(a[2]).all()                                                 # r = 0: both
        a64, _se, _t = gs.reference(flat, u, 2, False)                              # float64: e^89 is finite
        assert np.isfinite(a64).all() and a64[1, 0] == 0.5 and np.all(a64[2] == [0.5, -0.5])
        sq, se = bs.squashed_sample(flat, u, 2, F32)
        assert np.all(sq[0] == 1.0) and np.isnan(sq[1, 0]) and sq[1, 1] == 1.0
        # the squashed backward: dz = da (1 - a^2) = 0 exactly, dlogstd = 0 * inf = NaN
        da = np.full((3, 2), 0.25, F32)
        g = bs.squashed_bwd(flat, da, se, sq, 2, 0.0, F32)
        assert np.all(g[0, :2] == 0) and np.isnan(g[0, 2:]).all()
        # ... while at a finite std the saturated row passes exactly the regulariser
        flat80 = np.array([[0.5, -0.5, 80.0, 80.0]], F32)
        sq, se = bs.squashed_sample(flat80, u[:1], 2, F32)
        g = bs.squashed_bwd(flat80, da[:1], se, sq, 2, 0.125, F32)
        assert np.all(np.abs(sq) == 1.0) and np.array_equal(g, flat80 * F32(0.125))
        # mode() never reads the std
        assert np.array_equal(bs.mode(bs.BOX2T, flat), np.tanh(flat[:, :2])) and np.array_equal(
            bs.mode(("box", 2), flat), flat[:, :2])


def test_zero_draw_seed():
    """the constants of tests/test_gauss_edges_gpu.py::test_device_draws_a_zero_radius"""
    from oracle import philox
    u = philox.uniforms5(gs.ZERO_SEED, 0x40000 | (gs.ZERO_AGENT << 1), 0, np.arange(16))
    assert u[gs.ZERO_ROW, 0] == 0 and np.count_nonzero(u[:, 0] == 0) == 1
