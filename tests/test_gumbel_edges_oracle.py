"""CPU: the edge inputs of tests/gumbel_edges.py are what they claim to be.

* the exact-logit actor reproduces a logit table bit for bit through
  oracle.nets.mlp_fwd, in fp32 and with the hidden units summed in any order;
* the grids meet their conditions (no all-zero row, every edge value, every
  (uniform, logit) pair, a tie at the maximum, a saturated entry);
* the baseline e32: oracle.nets.gumbel_softmax (numpy fp32) against the float64
  reference on grid(5).  Measured: 1.08e-7 absolute, 5.50e-6 relative (over
  entries with reference probability > 1e-30); the recorded E32_ABS / E32_REL
  are those figures and the GPU tests bound the device by 4 x them;
* the factor S_UPDATE of the saturated update case is the one the three
  conditions stated beside it select.  Measured at S_UPDATE = 16 on the
  [18, 18, 18] case: largest sampled probability 1 - 2.1e-10 (1.0f), fp32 /
  fp64 oracle gradient gap 8.2e-7 of the tensor's largest entry (bound / 4 =
  2.5e-6), largest |logit| 19.5, largest weight 4.7 (ulp 4.8e-7); at 32 the
  largest weight is 9.4 (ulp 9.5e-7 > 5e-7).  The other cases the GPU tests run
  at the same factor: [3, 11] widths [3, 5] gap 4.6e-7, |logit| <= 14.9; tag
  N=6 at H = 128 (round-start gradients) gap 8.4e-7, |logit| <= 13.6.
"""
import numpy as np
import pytest

from oracle import nets
from tests import gumbel_edges as ge


@pytest.mark.parametrize("obs_dim,H,width", [(18, 64, 5), (18, 128, 5), (22, 256, 5), (3, 64, 3), (5, 64, 1)])
def test_exact_logit_actor_is_exact(obs_dim, H, width):
    lg, _ = ge.grid(width)
    p = ge.exact_logit_actor(obs_dim, H, width)
    obs = ge.obs_for(lg, obs_dim)
    got = nets.mlp_fwd(p, obs)[0]
    assert got.dtype == np.float32 and np.array_equal(got, lg)
    # any summation order: the hidden units permuted (rows and columns of the layers alike)
    perm = np.random.default_rng(0).permutation(H)
    q = {"W1": p["W1"][:, perm], "b1": p["b1"][perm], "W2": p["W2"][perm][:, perm], "b2": p["b2"][perm],
         "W3": p["W3"][perm], "b3": p["b3"]}
    assert np.array_equal(nets.mlp_fwd(q, obs)[0], lg)
    # every product but the driven ones is an exact zero: one non-zero term per sum
    assert (np.count_nonzero(p["W1"], 0) <= 1).all() and (np.count_nonzero(p["W2"], 0) <= 1).all()
    assert (np.count_nonzero(p["W3"], 0) == 2).all() and (np.count_nonzero(p["W3"], 1) <= 1).all()


def test_exact_logit_actor_with_driven_observation_entries():
    lg, _ = ge.rollout_rows(17, 2)
    drive = [0, 1, 2, 3, None]
    p = ge.exact_logit_actor(18, 64, 5, drive=drive)
    obs = ge.obs_for(lg, 18, drive=drive)
    assert np.array_equal(nets.mlp_fwd(p, obs)[0], lg) and np.all(lg[:, 4] == 0)
    assert np.abs(obs).max() == 0.625


@pytest.mark.parametrize("width", [5, 3, 1])
def test_grid_conditions(width):
    lg, u = ge.grid(width)
    assert lg.shape == u.shape and lg.shape[1] == width and lg.dtype == u.dtype == np.float32
    ge.check_inputs(lg, u, pairs=True)          # (grid() asserts them too)
    ref = ge.reference(lg, u)
    assert np.all(ref[u == 0] == 0) and np.allclose(ref.sum(1), 1, rtol=0, atol=1e-15)
    if width == 1:
        assert not (u == 0).any() and np.all(ref == 1)
    else:
        assert (u == 0).any() and ((ref > 0) & (ref < 1e-25)).any() and (ref > 1 - 2e-7).any()
    # the ends of the device's grid: u01 of the smallest and the largest 23-bit mantissa
    from oracle import philox
    ends = philox.u01(np.array([0, 1 << 9, 0xFFFFFFFF], np.uint32))
    assert list(ends) == [ge.UNIFORMS[0], ge.UNIFORMS[1], ge.UNIFORMS[6]]


@pytest.mark.parametrize("agent,width", [(j, 5) for j in range(6)] + [(0, 3)])
def test_rollout_rows_conditions(agent, width):
    lg, u = ge.rollout_rows(17, agent, width)
    ge.check_inputs(lg[:, :min(width, 4)], u)
    assert np.all(lg[:, 4:] == 0)
    ge.reference(lg, u)


def test_rollout_positions_differ_between_agents():
    pos = np.stack([ge.rollout_rows(17, j)[0][:, 2:4] for j in range(6)], 1)     # [E, n, 2]
    for a in range(6):
        for b in range(a + 1, 6):
            assert np.all(np.abs(pos[:, a] - pos[:, b]).max(-1) > 0)


def test_baseline_e32():
    a, r = ge.baseline_e32(5)
    print(f"e32 on grid(5): abs {a:.3e} rel {r:.3e}")
    # the recorded yardstick is this measurement (numpy's fp32 log / exp differ by
    # an ulp between SIMD builds: a quarter either way)
    assert 0.75 * ge.E32_ABS <= a <= 1.25 * ge.E32_ABS
    assert 0.75 * ge.E32_REL <= r <= 1.25 * ge.E32_REL
    # the narrower forms are no worse
    for w in (3, 1):
        aw, rw = ge.baseline_e32(w)
        assert aw <= a and rw <= r
    # zeros and NaN: the restatement gives the exact 0 and a finite rest
    lg, u = ge.grid(5)
    got = nets.gumbel_softmax(lg, u)
    assert np.all(np.isfinite(got)) and np.all(got[u == 0] == 0)


def test_edge_noise_rows():
    c = ge.saturated_case([18, 18, 18], 40, 300, ge.SEED_UPDATE, ge.S_UPDATE)
    rows = c["edge_rows"]
    assert {int(r) // 16 for r in rows} == {0, 1, 2}          # both full tiles and the ragged one
    for i in range(3):
        for blk in list(c["u_tgt"][i]) + [c["u_act"][i]]:
            assert (blk[rows] == 0).any() and (blk[rows] == ge.UNIFORMS[6]).any()
            assert set(np.unique(blk[rows])) <= set(ge.UNIFORMS)
            others = np.delete(blk, rows, 0)
            assert others.min() >= 1e-6 and others.max() < 1
    assert c["replaced"] <= 0.1 * 3 * 40


@pytest.mark.parametrize("name,kw,throughput", [
    ("spread", dict(dims=[18, 18, 18], seed=ge.SEED_UPDATE), False),
    ("narrow", dict(dims=[3, 11], widths=[3, 5], seed=ge.SEED_UPDATE + 1), False),
    ("tag6_h128", dict(dims=[22, 22, 22, 22, 20, 20], seed=61, H=128), True)])
def test_update_factor_conditions(name, kw, throughput):
    s = ge.S_UPDATE
    c = ge.saturated_case(B=40, L=300, s=s, **kw)
    gap, top, lmax = ge.oracle_gap(c, kw.get("widths"), throughput)
    print(f"{name} s={s}: fp32/fp64 oracle gradient gap {gap:.3e}, 1 - top probability {1 - top:.3e}, "
          f"max |logit| {lmax:.2f}, weight ulp {ge.largest_weight_ulp(c):.2e}, {c['replaced']} positions replaced, "
          f"edge rows {[int(r) for r in c['edge_rows']]}")
    assert top > 1 - 1e-6
    assert gap <= ge.GRAD_BOUND / 4
    assert ge.largest_weight_ulp(c) <= ge.WEIGHT_BOUND / 2
    assert lmax <= ge.LOGITS.max()            # within the range the forward tests cover
    if name == "spread":                      # the case the factor is chosen on: the next one fails
        c2 = ge.saturated_case(B=40, L=300, s=2 * s, **kw)
        gap2, top2, _ = ge.oracle_gap(c2)
        assert top2 > 1 - 1e-6 and gap2 <= ge.GRAD_BOUND / 4
        assert ge.largest_weight_ulp(c2) > ge.WEIGHT_BOUND / 2


def test_zero_draw_seed():
    """the constants of tests/test_gumbel_edges_gpu.py::test_device_draws_a_zero"""
    from oracle import philox
    u = philox.uniforms5(ge.ZERO_SEED, 0x40000 | (ge.ZERO_AGENT << 1), 0, np.arange(16))
    assert u[ge.ZERO_ROW, ge.ZERO_ENTRY] == 0 and np.count_nonzero(u == 0) == 1
