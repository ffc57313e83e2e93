"""CPU tests of the constructed M3DDPG states (tests/minimax_edges.py):
each case has the property the GPU test relies on, the float64 restatement still agrees
with torch.autograd under the clamp, and five subtly wrong perturbations -- variants of
minimax_oracle.perturb, kept here -- land far outside the bounds of
tests/test_minimax_edges_gpu.py on at least one case each (CATCHES).
"""
import numpy as np
import pytest

from oracle import nets
from tests import minimax_cases as mc
from tests import minimax_edges as me
from tests import minimax_oracle as mo
from tests import mixed_width

F32, F64 = np.float32, np.float64


def _others(n, i):
    return [j for j in range(n) if j != i]


def _all_sites(c, dt=F32):
    ags = mc.oracle_agents(c)
    return [me.sites(c, ags, i, dt) for i in range(len(ags))]


# ---- A
@pytest.mark.parametrize("shape", me.THREE)
def test_gate_gives_exact_zero_gradients_beside_live_rows_in_every_tile(shape):
    c = me.case("A", shape)
    n = len(c["params"])
    assert all(dead >= 2 and live >= 2 for dead, live in me.gate_tiles(c)), me.gate_tiles(c)
    zero = _all_sites(me.with_eps(c, np.zeros((n, n))))
    for i, s in enumerate(_all_sites(c)):
        dead = c["gate"][c["idx"][i]] == 1
        for site in ("critic", "actor"):
            adv, ss = s[site]
            assert np.isfinite(adv).all()
            for j in _others(n, i):
                assert not ss[j][dead].any() and np.all(ss[j][~dead] > 1e-6), (i, site, j)   # 0.0 / far above the clamp
            assert np.array_equal(adv[dead], zero[i][site][0][dead])
            assert np.all(np.abs(adv[~dead] - zero[i][site][0][~dead]).max(-1)[:, _others(n, i)] > 0.01)


# ---- B
@pytest.mark.parametrize("shape", me.THREE)
def test_a_dead_critic_has_no_gradient_anywhere(shape):
    c = me.case("B", shape)
    n = len(c["params"])
    for i, s in enumerate(_all_sites(c)):
        assert not s["critic"][1][_others(n, i)].any() and not s["actor"][1][_others(n, i)].any()
    a, b = mc.oracle_agents(c), mc.oracle_agents(c)
    c0 = me.with_eps(c, np.zeros((n, n)))
    for i in range(n):
        assert mc.oracle_update(a, c, i)[0] == mc.oracle_update(b, c0, i)[0]


# ---- C, D
def _ss_pairs(c, dt):
    n = len(c["params"])
    return np.concatenate([s[site][1][_others(n, i)].ravel() for i, s in enumerate(_all_sites(c, dt))
                           for site in ("critic", "actor")])


@pytest.mark.parametrize("kind,shape,scale", [("C", s, 0) for s in me.THREE] + [("G", "narrow", -20)])
def test_clamp_regime_every_ss_is_below_the_clamp_and_the_step_is_large(kind, shape, scale):
    c = me.case(kind, shape, scale)
    n = len(c["params"])
    for dt in (F32, F64):
        ss = _ss_pairs(c, dt)
        assert np.all(ss < me.CLAMP) and np.all(ss >= 0), (dt, float(ss.max()))
    zero = _all_sites(me.with_eps(c, np.zeros((n, n))))
    for i, s in enumerate(_all_sites(c)):
        for site in ("critic", "actor"):
            adv, ss = s[site]
            step = np.abs(adv - zero[i][site][0]).max(-1)
            big = step > 100 * me.adv_bound(ss, c["eps"][i], i)
            for j in _others(n, i):       # not a case that passes because nothing moves
                assert big[:, j].mean() >= 0.5, (i, site, j, float(big[:, j].mean()))


@pytest.mark.parametrize("shape", me.THREE)
def test_straddle_has_a_tenth_of_its_pairs_on_each_side_of_the_clamp(shape):
    c = me.case("D", shape)
    for dt in (F32, F64):
        below = float((_ss_pairs(c, dt) < me.CLAMP).mean())
        print(f"D {shape} {dt.__name__}: {below:.3f} of the (row, agent) pairs below the clamp")
        assert 0.1 <= below <= 0.9, below


def _rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("kind", ["C", "D"])
@pytest.mark.parametrize("shape", me.THREE)
def test_float64_restatement_matches_autograd_under_the_clamp(shape, kind):
    """tests/test_minimax_oracle.py's comparison (1e-10 of each tensor's largest entry) where
    torch.clamp(ss, min=1e-12) binds on all (C) or some (D) rows"""
    pytest.importorskip("torch")
    c = me.case(kind, shape)
    ags = mc.oracle_agents(c)
    S = sum(c["spec"]["dims"])
    for i in range(len(ags)):
        bn = mc.batches(c, i)
        u_t = mixed_width.narrow(c["u_tgt"][i], c["widths"])
        gq, st = mo.critic_grads(ags, i, bn, u_t, c["eps"][i], dt=F64)
        gp, p_loss, ex = mo.actor_grads(ags, i, bn, c["u_act"][i], c["eps"][i], dt=F64)
        t = mo.torch_step(ags, i, bn, u_t, c["u_act"][i], c["eps"][i])
        assert abs(st["q_loss"] - t["q_loss"]) <= 1e-10 * abs(t["q_loss"])
        assert abs(p_loss - t["p_loss"]) <= 1e-10 * abs(t["p_loss"])
        assert _rel(st["target_q_next"], t["target_q_next"]) < 1e-10
        for k in nets.NAMES:
            assert _rel(gq[k].reshape(t["grad_critic"][k].shape), t["grad_critic"][k]) < 1e-10, (i, k)
            assert _rel(gp[k].reshape(t["grad_actor"][k].shape), t["grad_actor"][k]) < 1e-10, (i, k)
        assert _rel(np.concatenate(st["adv"], 1), t["adv_critic"][:, S:]) < 1e-10
        assert _rel(np.concatenate(ex["adv"], 1), t["adv_actor"][:, S:]) < 1e-10


# ---- F
@pytest.mark.parametrize("n", [3, 6])
def test_asymmetric_matrix_has_no_two_equal_entries_and_one_zero_per_row(n):
    e = me.asym_eps(n)
    off = ~np.eye(n, dtype=bool)
    assert e.dtype == F32 and not e.diagonal().any()
    assert all((e[i][off[i]] == 0).sum() == 1 for i in range(n))
    pos = e[off & (e > 0)]
    assert len(set(pos.tolist())) == len(pos)
    assert not np.array_equal(e, e.T) and np.all(np.abs(e - e.T)[off] > 0.04)


# ---- G
def test_narrow_widths_the_width_one_step_is_eps_times_a_determined_sign():
    c = me.case("G", "narrow")
    assert c["widths"] == [1, 2, 5]
    for i, s in enumerate(_all_sites(c)):
        for site in ("critic", "actor"):
            adv, ss = s[site]
            for j, w in enumerate(c["widths"]):
                assert not adv[:, j, w:].any()
            if i != 0:    # ss = g^2: |g| stands 100 gradient tolerances clear of 0, so sign(g) is not in doubt
                norm = np.sqrt(ss[0])
                assert np.all(norm > 100 * 1e-5 * norm.max()), (i, site, float(norm.min() / norm.max()))
                assert np.all(np.abs(np.abs(adv[:, 0, 0] - 1) - c["eps"][i][0]) <= 2e-6)   # a_0 is 1.0: a^ = 1 -+ eps


# ---- H
def test_linear_regime_margins_formula_and_the_five_percent_rule():
    c = me.case("H", "spread")
    n = len(c["params"])
    ags = mc.oracle_agents(c)
    c0 = me.with_eps(c, np.zeros((n, n)))
    for i in range(n):
        margin = me.linear_margins(c, ags, i)
        assert margin >= 1e-3, (i, margin)
        drops = me.linear_drop(ags[i].tgt_critic, c, i), me.linear_drop(ags[i].critic, c, i)
        s64, z64 = me.sites(c, ags, i, F64), me.sites(c0, ags, i, F64)
        assert abs((z64["q_next"] - s64["q_next"]) - drops[0]) <= 1e-9 * drops[0]
        assert abs((s64["p_loss"] - z64["p_loss"]) - drops[1]) <= 1e-9 * drops[1]
        s32, z32 = me.sites(c, ags, i), me.sites(c0, ags, i)
        for key, drop in (("q_next", drops[0]), ("p_loss", drops[1])):
            tol = 2e-5 * max(abs(s32[key]), abs(z32[key])) + 2e-6
            print(f"H agent {i} {key}: expected drop {drop:.6f}, tolerance {tol:.2e} = {tol / drop:.4f} of it, "
                  f"margin {margin:.3f}")
            assert tol < 0.05 * drop, (i, key, tol, drop)


# ---- the wrong kernels
def _variant(kind, eps):
    """minimax_oracle.perturb with one mistake: clamp_sqrt (a) clamps sqrt(ss) instead of ss;
    no_clamp (b); transposed (c) takes eps[j][i]; shifted (d) indexes the row as if the
    updating agent's slot were left out; pad_ss (e) sums ss over all five slot entries, the
    pad ones carrying the gradient of the slot's last logical entry"""
    def perturb(p, x, offs, widths, i, eps_row, dt=F32, sign=1):
        B = x.shape[0]
        _, cache = mo.fwd(p, x, dt)
        dx = mo.in_grad(p, cache, np.ones((B, 1), dt), dt)
        xh = np.array(cache[0], dt, copy=True)
        ss_n = np.full((len(widths), B), np.nan)
        for j, (o, k) in enumerate(zip(offs, widths)):
            if j == i:
                continue
            g = dx[:, o:o + k]
            ss = np.zeros(B, dt)
            for col in range(k):
                ss = ss + g[:, col] * g[:, col]
            e = eps_row[j]
            if kind == "transposed":
                e = eps[j][i]
            elif kind == "shifted":
                e = eps[i][j - 1] if j > i else eps[i][j]
            elif kind == "pad_ss":
                ss = ss + dt(5 - k) * g[:, k - 1] * g[:, k - 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                if kind == "clamp_sqrt":
                    inv = dt(1) / np.maximum(np.sqrt(ss), dt(1e-12))
                elif kind == "no_clamp":
                    inv = dt(1) / np.sqrt(ss)
                else:
                    inv = dt(1) / np.sqrt(np.maximum(ss, dt(1e-12)))
                xh[:, o:o + k] = xh[:, o:o + k] - dt(sign * float(e)) * (g * inv[:, None])
            ss_n[j] = ss
        return xh, ss_n
    return perturb


# which constructed case catches which variant (case letter, shape, W3 scale as 2^k)
CATCHES = {
    "clamp_sqrt": [("C", "spread", 0), ("C", "tag", 0), ("C", "spread_wide", 0), ("D", "spread", 0), ("G", "narrow", -20)],
    "no_clamp": [("C", "spread", 0), ("D", "tag", 0), ("D", "spread_wide", 0), ("G", "narrow", -20)],
    "transposed": [("F", "spread", 0), ("F", "tag", 0), ("H", "spread", 0)],
    "shifted": [("F", "spread", 0), ("F", "tag", 0), ("H", "spread", 0)],
    "pad_ss": [("G", "narrow", 0)],      # (not at 2^-20: under the clamp ss does not enter a^)
}


def _worst_move(c, good, bad):
    """largest |a^_variant - a^| over rows, sites and agents in units of the GPU test's bound"""
    worst = 0.0
    for i in range(len(good)):
        for site in ("critic", "actor"):
            move = np.abs(bad[i][site][0] - good[i][site][0]).max(-1)
            worst = max(worst, float((move / me.adv_bound(good[i][site][1], c["eps"][i], i)).max()))
    return worst


@pytest.mark.parametrize("variant", list(CATCHES))
def test_a_subtly_wrong_perturbation_is_far_outside_the_gpu_bounds(monkeypatch, variant):
    for kind, shape, scale in CATCHES[variant]:
        c = me.case(kind, shape, scale)
        good = _all_sites(c)
        with monkeypatch.context() as m:
            m.setattr(mo, "perturb", _variant(variant, c["eps"]))
            bad = _all_sites(c)
        worst = _worst_move(c, good, bad)
        print(f"{variant} on {kind} {shape} 2^{scale}: a^ moves {worst:.0f} x its bound")
        if kind == "H":     # ... and some agent's mean q' by more than 100 x H's tolerance
            assert max(abs(b["q_next"] - g["q_next"]) / (2e-5 * abs(g["q_next"]) + 2e-6)
                       for g, b in zip(good, bad)) > 100
        assert worst > 100, (variant, kind, shape, worst)


def test_no_clamp_is_not_finite_on_the_gate_rows(monkeypatch):
    c = me.case("A", "spread")
    monkeypatch.setattr(mo, "perturb", _variant("no_clamp", c["eps"]))
    for i, s in enumerate(_all_sites(c)):
        dead = c["gate"][c["idx"][i]] == 1
        for site in ("critic", "actor"):
            assert np.isnan(s[site][0][dead]).any(1).all() and np.isfinite(s[site][0][~dead]).all()


@pytest.mark.parametrize("variant", ["clamp_sqrt", "no_clamp", "transposed"])
def test_the_earlier_fixtures_cannot_tell_these_variants_from_the_kernel(monkeypatch, variant):
    """why section 28 exists: at eps = 0.3 for every pair on Xavier critics the clamp never
    binds and the matrix is its own transpose -- a^ comes out bit for bit the same"""
    c = mc.make_case("spread", "large")
    good = _all_sites(c)
    monkeypatch.setattr(mo, "perturb", _variant(variant, c["eps"]))
    for g, b in zip(good, _all_sites(c)):
        assert np.array_equal(g["critic"][0], b["critic"][0]) and np.array_equal(g["actor"][0], b["actor"][0])
