"""GPU tests of M3DDPG's perturbation where the action gradient vanishes or is tiny
(mm_perturb in mdp_grads.hip), on the constructed states of
tests/minimax_edges.py.

Handles, updates and the update-parity tolerances are tests/test_minimax_gpu.py's.
a^ (adv_out of both steps) is held on EVERY row to minimax_edges.adv_bound, which is that
file's bound above the clamp and its gradient tolerance times the constant 1e6 below it;
where the gradient is exactly zero, or eps is, a^ equals the slot of a handle with
eps = 0 on the same inputs bit for bit.  Case H checks the sign and the size of the step
against a product of the critic's weights, not against the restatement.  What each
case would catch is shown on the CPU in tests/test_minimax_edges_oracle.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from tests import minimax_cases as mc  # noqa: E402
from tests import minimax_edges as me  # noqa: E402
from tests import minimax_oracle as mo  # noqa: E402
from tests.test_minimax_gpu import _assert_equal, _engine, _state, _update, _update_parity  # noqa: E402


def _same_critic(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def _run(c, tag):
    """one update of every agent on a handle with the case's eps and on one with eps = 0
    (same inputs).  Held here for every case: minimax_info, update parity against the fp32
    restatement, the critic bit-identical after its step (lr = 0), exact-zero pad entries
    and a^ within adv_bound on every row of both sites.  Returns per agent
    {site: (a^, a^ of the eps = 0 handle, oracle ss)} and both handles' stats; prints the
    worst error / bound ratio per site."""
    n = len(c["params"])
    zero = np.zeros((n, n), np.float32)
    eng, eng0 = _engine(c, tag), _engine(c, tag, eps=zero)
    assert np.array_equal(eng.minimax_info(), c["eps"] * (1 - np.eye(n, dtype=np.float32)))
    adv, adv0 = eng.minimax_debug_adv(), eng0.minimax_debug_adv()
    ags = mc.oracle_agents(c)
    out, worst, moved = [], {"critic": 0.0, "actor": 0.0}, {"critic": 0.0, "actor": 0.0}
    for i in range(n):
        for t in adv + adv0:
            t.zero_()
        before = eng.get_params(i, "critic")
        got, _, ex = _update_parity(eng, ags, c, i, tag)
        _update(eng0, c, i)
        eng0.synchronize()
        if c["lr"] == 0:    # the actor site saw the constructed critic, not one an Adam step moved
            assert _same_critic(before, eng.get_params(i, "critic")), i
        rec = {"stats": got, "stats0": eng0.stats(i)}
        for s, site in enumerate(("critic", "actor")):
            dev, dev0 = adv[s].cpu().numpy(), adv0[s].cpu().numpy()
            want, ss = mo.pad5(ex["adv_" + site]), ex["ss_" + site]
            assert np.isfinite(dev).all(), (tag, i, site)
            for j, w in enumerate(c["widths"]):
                assert not dev[:, j, w:].any(), (tag, i, site, j, "pad entries")
            assert np.array_equal(dev[:, i], dev0[:, i]), (tag, i, site, "own slot")
            ratio = np.abs(dev - want).max(-1) / me.adv_bound(ss, c["eps"][i], i)
            worst[site] = max(worst[site], float(ratio.max()))
            moved[site] = max(moved[site], float(np.delete(ratio, i, 1).max()))
            assert np.all(ratio <= 1), (tag, i, site, float(ratio.max()), np.argwhere(ratio > 1)[:4].tolist())
            rec[site] = (dev, dev0, ss)
        out.append(rec)
    print(f"{tag}: a^ worst error / bound critic {worst['critic']:.3f} actor {worst['actor']:.3f}; over the "
          f"perturbed slots alone {moved['critic']:.3f} / {moved['actor']:.3f}")
    return out


# ---- A. dead and live rows in one tile
@pytest.mark.parametrize("shape", me.THREE)
def test_zero_gradient_rows_are_the_unperturbed_rows_bit_for_bit(shape):
    c = me.case("A", shape)
    for i, rec in enumerate(_run(c, f"A {shape}")):
        dead = c["gate"][c["idx"][i]] == 1
        for site in ("critic", "actor"):
            dev, dev0, ss = rec[site]
            assert np.array_equal(dev[dead], dev0[dead]), (i, site)
            others = [j for j in range(len(c["widths"])) if j != i]
            assert np.all(np.abs(dev[~dead] - dev0[~dead]).max(-1)[:, others] > 0.01), (i, site)   # live rows moved


# ---- B. a wholly dead critic: eps changes nothing, ever
@pytest.mark.parametrize("shape", me.THREE)
def test_a_dead_critic_trains_as_with_eps_zero_bit_for_bit(shape):
    c = me.case("B", shape)
    n = len(c["params"])
    eng, eng0 = _engine(c, shape), _engine(c, shape, eps=np.zeros((n, n), np.float32))
    for r in range(3):
        for i in range(n):
            _update(eng, c, i)
            _update(eng0, c, i)
            if r in (0, 2):
                assert eng.stats(i) == eng0.stats(i), (r, i)
                _assert_equal(_state(eng, i), _state(eng0, i), (r, i))
    assert eng.check_finite() == 0


# ---- C, D. under and across the clamp (E's bound, held in _run)
@pytest.mark.parametrize("kind", ["C", "D"])
@pytest.mark.parametrize("shape", me.THREE)
def test_clamped_rows_step_by_eps_g_1e6(shape, kind):
    c = me.case(kind, shape)
    for i, rec in enumerate(_run(c, f"{kind} {shape}")):
        for site in ("critic", "actor"):
            dev, dev0, ss = rec[site]
            below = np.delete(ss, i, 0) < me.CLAMP       # (the restatement's fp32 ss)
            assert below.all() if kind == "C" else below.any(), (i, site)
            assert not np.array_equal(dev, dev0)


# ---- F. an asymmetric matrix: row i, column j
@pytest.mark.parametrize("shape", ["spread", "tag"])
def test_asymmetric_eps_is_read_by_row_and_a_zero_entry_moves_nothing(shape):
    c = me.case("F", shape)
    n = len(c["params"])
    for i, rec in enumerate(_run(c, f"F {shape}")):
        for site in ("critic", "actor"):
            dev, dev0, _ = rec[site]
            for j in range(n):
                if c["eps"][i][j] == 0:
                    assert np.array_equal(dev[:, j], dev0[:, j]), (i, site, j)
                else:
                    assert not np.array_equal(dev[:, j], dev0[:, j]), (i, site, j)


# ---- G. widths 1 and 2
@pytest.mark.parametrize("scale", [0, -20])
def test_narrow_widths(scale):
    c = me.case("G", "narrow", scale)
    ags = mc.oracle_agents(c)
    for i, rec in enumerate(_run(c, f"G 2^{scale}")):
        if scale or i == 0:
            continue
        s64 = me.sites(c, ags, i, np.float64)   # (lr = 0: ags' weights are the critic's after its step too)
        for site in ("critic", "actor"):
            dev, dev0, _ = rec[site]
            sign = np.sign(dev0[:, 0, 0].astype(np.float64) - s64[site][0][:, 0, 0])   # a - a^ = eps sign(g)
            assert np.all(np.abs(sign) == 1)
            want = dev0[:, 0, 0].astype(np.float64) - float(c["eps"][i][0]) * sign
            assert np.all(np.abs(dev[:, 0, 0] - want) <= 2e-6), (i, site, float(np.abs(dev[:, 0, 0] - want).max()))


# ---- H. sign and size from the weights alone
def test_linear_critic_q_drops_by_eps_times_the_gradient_norms():
    c = me.case("H", "spread")
    ags = mc.oracle_agents(c)
    for i, rec in enumerate(_run(c, "H spread")):
        got, got0 = rec["stats"], rec["stats0"]
        # stats[4]: mean q' (target critic); stats[1]: p_loss = -mean Q + regulariser (critic).
        # Tolerance: the stats tolerance once (2e-5 |stat| + 2e-6), though two device values are subtracted
        for k, name, p, sgn in ((4, "mean q'", ags[i].tgt_critic, -1.0), (1, "p_loss", ags[i].critic, 1.0)):
            want = me.linear_drop(p, c, i)
            drop = sgn * (got[k] - got0[k])
            tol = 2e-5 * max(abs(got[k]), abs(got0[k])) + 2e-6
            print(f"H agent {i} {name}: expected {want:.6f} measured {drop:.6f} tolerance {tol:.2e}")
            assert abs(drop - want) <= tol, (i, name, drop, want, tol)
