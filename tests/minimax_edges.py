"""Constructed states for M3DDPG's perturbation where the action gradient vanishes or
is tiny; shared by tests/test_minimax_edges_oracle.py (CPU) and
tests/test_minimax_edges_gpu.py.

Every case is minimax_cases.make_case (ring L = 200, injected idx / u_tgt / u_act,
rows cleaned by minimax_oracle.clean_idx AFTER the state is put in) with one thing
changed in every agent's critic and target critic:

  A  gate        W1[0, :] = -64 and obs_0[:, 0] = obs'_0[:, 0] = a gate bit per ring row:
                 gate 1 switches every layer-1 unit off (g == 0 exactly), gate 0 rows are live
  B  dead        b2 = -64: every layer-2 unit off on every row
  C  clamp       W3 * 2^-20 (exact): every ss below the clamp 1e-12
  D  straddle    W3 * 2^-17: ss on both sides of the clamp
  F  asym        the fixture's critics, eps[i][j] all different with one 0 per row
  G  narrow      act_dims [1, 2, 5], at the fixture's scale and at 2^-20
  H  linear      b1, b2 raised until every unit is active on every row: g is a product
                 of the weights, Q(a^) - Q(a) = -sum_j eps[i][j] |g_j|_2

All but B run at learning rate 0: the actor step differentiates the critic after its
Adam step, and only a critic that stays put keeps the constructed state there.
"""
import functools

import numpy as np

from maddpg_amd.envs import spec
from tests import minimax_cases as mc
from tests import minimax_oracle as mo
from tests import mixed_width

F32, F64 = np.float32, np.float64
CLAMP = float(F32(1e-12))   # fmaxf(ss, 1e-12f)
SHAPES = {
    "spread": mc.CASES["spread"],            # two full 16-row tiles and a ragged one; the actor's par path
    "tag": mc.CASES["tag"],                  # two 16-column tiles of action gradient
    "spread_wide": mc.CASES["spread_wide"],  # the actor's serial critic layer 1: the non-par call
    "narrow": dict(dims=spec("simple_spread").obs_dims, H=64, B=40, n_adv=0, widths=[1, 2, 5]),
}
THREE = ("spread", "tag", "spread_wide")


def uniform_eps(n, e=0.3):
    return (F32(e) * (1 - np.eye(n, dtype=F32))).astype(F32)


def asym_eps(n):
    """eps[i][j] = 0.05 (1 + n i + j): no two entries equal, so neither the transpose nor a
    shifted column passes; eps[i][(i + 1) % n] = 0 exactly"""
    e = np.array([[0.05 * (1 + n * i + j) for j in range(n)] for i in range(n)], F32)
    for i in range(n):
        e[i, i] = 0
        e[i, (i + 1) % n] = 0
    return e


def _critics(c):
    for p in c["params"]:
        yield p["critic"]
        yield p["tgt_critic"]


def _gate(c, seed):
    bits = np.random.default_rng(seed).integers(0, 2, size=mc.L).astype(F32)
    for q in _critics(c):
        q["W1"][0, :] = -64
    o, a, r, on, d = c["data"][0]
    o, on = np.array(o, copy=True), np.array(on, copy=True)
    o[:, 0] = bits
    on[:, 0] = bits
    c["data"][0] = (o, a, r, on, d)
    c["gate"] = bits


def _dead(c):
    for q in _critics(c):
        q["b2"][:] = -64


def _scale_w3(c, k):
    for q in _critics(c):
        q["W3"] *= F32(2.0 ** k)


def _bounds(x, W, slots, eps_max):
    """lowest value x @ W can take per unit when every action slot (columns o .. o + k
    of x, a point of the simplex there) moves anywhere in the simplex and then by eps_max
    in 2-norm: x @ W - sum_j |W[slot j]|_2 (sqrt(2) + eps_max)"""
    slack = sum(np.linalg.norm(W[o:o + k], axis=0) for o, k in slots) * (np.sqrt(2.0) + eps_max)
    return (x @ W).min(0) - slack, slack


def _linear(c, margin=0.1):
    """b1, b2 of every critic so that both layers are active on every ring row (obs and
    obs', any actions in the simplex, any step of the case's eps), no higher than needed:
    a large Q would put the stats tolerance above the drop that case H measures"""
    data, n = c["data"], len(c["params"])
    S = sum(d[0].shape[1] for d in data)
    slots, o = [], S
    for w in c["widths"]:
        slots.append((o, w))
        o += w
    xs = [np.concatenate([np.asarray(d[k], F64) for d in data] + [np.asarray(d[1], F64) for d in data], 1)
          for k in (0, 3)]
    x = np.concatenate(xs, 0)
    e = float(c["eps"].max())
    for q in _critics(c):
        W1, W2 = np.asarray(q["W1"], F64), np.asarray(q["W2"], F64)
        lo1, slack1 = _bounds(x, W1, slots, e)
        b1 = (margin - lo1).astype(F32)
        h1 = x @ W1 + b1
        lo2 = (h1 @ W2).min(0) - np.abs(W2).T @ slack1
        q["b1"][:] = b1
        q["b2"][:] = (margin - lo2).astype(F32)
    assert n == len(slots)


@functools.lru_cache(maxsize=None)
def case(kind, shape, scale=0):
    """the constructed case `kind` (a letter of the module docstring) on SHAPES[shape];
    treat the result as read-only (it is shared between tests)"""
    sp = SHAPES[shape]
    n = len(sp["dims"])
    eps = asym_eps(n) if kind in "FH" else uniform_eps(n)
    prep = {"A": None, "B": _dead, "C": lambda c: _scale_w3(c, -20), "D": lambda c: _scale_w3(c, -17),
            "F": None, "G": (lambda c: _scale_w3(c, scale)) if scale else None, "H": _linear}[kind]
    if kind == "A":     # the first gate seed whose batches put >= 2 dead and >= 2 live rows in every tile
        for seed in range(64):
            c = mc.make_case(shape, eps, spec=sp, prepare=lambda c: _gate(c, seed))
            if min(min(t) for t in gate_tiles(c)) >= 2:
                break
        else:
            raise RuntimeError("no gate seed fills every tile")
    else:
        c = mc.make_case(shape, eps, spec=sp, prepare=prep)
    c["lr"] = 1e-2 if kind == "B" else 0.0
    return c


def with_eps(c, eps):
    """c with another matrix (shares everything else)"""
    d = dict(c)
    d["eps"] = np.asarray(eps, F32)
    return d


def gate_tiles(c):
    """(dead, live) row counts of every 16-row tile of every agent's batch"""
    out = []
    for idx in c["idx"]:
        bits = c["gate"][idx]
        for t in range(0, len(bits), 16):
            b = bits[t:t + 16]
            out.append((int(b.sum()), int(len(b) - b.sum())))
    return out


def sites(c, ags, i, dt=F32):
    """both perturbation sites of agent i at ags' present weights (with lr = 0 those are
    also the critic's weights after its step): {site: (a^ [B, n, 5], ss [n, B])}, mean q', p_loss"""
    bn = mc.batches(c, i)
    _, st = mo.critic_grads(ags, i, bn, mixed_width.narrow(c["u_tgt"][i], c["widths"]), c["eps"][i], dt=dt)
    _, p_loss, ex = mo.actor_grads(ags, i, bn, c["u_act"][i], c["eps"][i], dt=dt)
    return {"critic": (mo.pad5(st["adv"]), st["ss"]), "actor": (mo.pad5(ex["adv"]), ex["ss"]),
            "q_next": float(np.mean(st["target_q_next"].astype(F64))), "p_loss": p_loss}


def adv_bound(ss, eps_row, own):
    """the a^ bound [B, n] of section 28, from the suite's gradient tolerance dg = 1e-5 x the
    largest |g_j|_2 of the batch and inv = 1 / sqrt(max(ss, 1e-12)):
      ss >= 1e-12: 2e-6 + eps_j 2 dg / sqrt(ss)   (tests/test_minimax_gpu.py's bound: the first-order
                                                   error of g / |g| is at most 2 |dg| / |g|)
      ss <  1e-12: 2e-6 + eps_j dg 1e6            (inv is the constant 1e6: the error of g inv is dg inv)
    within 1 +- 1e-4 of the clamp the larger of the two; no row is left out"""
    ss = np.asarray(ss, F64)
    n, B = ss.shape
    tol = np.full((B, n), 2e-6)
    for j in range(n):
        if j == own:
            continue
        s, e = ss[j], float(eps_row[j])
        dg = 1e-5 * np.sqrt(s.max())
        with np.errstate(divide="ignore", invalid="ignore"):
            above = np.where(s > 0, e * 2 * dg / np.sqrt(s), np.inf)
        below = np.full(B, e * dg * 1e6)
        t = np.where(s >= CLAMP, above, below)
        near = np.abs(s / CLAMP - 1) <= 1e-4
        tol[:, j] += np.where(near, np.maximum(above, below), t)
    return tol


def linear_drop(p, c, i):
    """sum_{j != i} eps[i][j] |g_j|_2 with g_j = W1[action rows of j] @ W2 @ W3 of critic
    weights p, float64: how far the step lowers Q on every row once no ReLU is inactive"""
    W1, W2, W3 = (np.asarray(p[k], F64) for k in ("W1", "W2", "W3"))
    g = (W1 @ W2 @ W3)[:, 0]
    o = sum(c["spec"]["dims"])
    total = 0.0
    for j, w in enumerate(c["widths"]):
        if j != i:
            total += float(c["eps"][i][j]) * float(np.linalg.norm(g[o:o + w]))
        o += w
    return total


def linear_margins(c, ags, i):
    """smallest ReLU input of the critic's and the target critic's two layers over agent
    i's batch, at the unperturbed and at the perturbed inputs of both sites, in units of the
    layer's largest |input| (float64)"""
    n = len(ags)
    bn = mc.batches(c, i)
    obs = [b[0].astype(F32).astype(F64) for b in bn]
    act = [b[1].astype(F32).astype(F64) for b in bn]
    nobs = [b[3].astype(F32).astype(F64) for b in bn]
    u_t = mixed_width.narrow(c["u_tgt"][i], c["widths"])
    at = [mo.gsm(mo.fwd(ags[j].tgt_actor, nobs[j], F64)[0], u_t[j], F64) for j in range(n)]
    a_in = list(act)
    a_in[i] = mo.gsm(mo.fwd(ags[i].actor, obs[i], F64)[0], np.asarray(c["u_act"][i])[:, :c["widths"][i]], F64)
    worst = np.inf
    for p, o_n, a_n in ((ags[i].tgt_critic, nobs, at), (ags[i].critic, obs, a_in), (ags[i].critic, obs, act)):
        x = mo.cin(o_n, a_n, i, False, F64)
        xh, _ = mo.perturb(p, x, mo.act_offsets(o_n, a_n), c["widths"], i, c["eps"][i], F64)
        q = {k: np.asarray(v, F64) for k, v in p.items()}
        for xx in (x, xh):
            z1 = xx @ q["W1"] + q["b1"]
            z2 = np.maximum(z1, 0) @ q["W2"] + q["b2"]
            worst = min(worst, float(z1.min() / np.abs(z1).max()), float(z2.min() / np.abs(z2).max()))
    return worst
