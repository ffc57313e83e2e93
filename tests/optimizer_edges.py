"""The optimizer step (clip_by_norm, TF1 ApplyAdam, Polyak, the beta-power
advance) restated in the device's operation order, and the constructed states
it is run from (host side only).

* ``tensor_step`` / ``net_step`` / ``polyak`` / ``advance_powers``: one step of
  one net as ``reduce_apply_body`` (mdp_apply_fused.hip) and ``k_apply``
  (mdp_kernels.hip) spell it, every elementwise op separately rounded (the
  library is built with -ffp-contract=off), written once over a dtype.  In
  float32 it is what the device must compute; in float64 it is the yardstick's
  other end (``bound``).  ``wrong=`` selects one of the deliberately wrong
  variants ``WRONG`` that the cases must be able to see.
* ``build_cases``: for a net's six tensor sizes the cases of five groups
  (``GROUPS``).  Gradients are integers times a power of two whose squares sum
  to a perfect square (``ints_with_norm``): the fp64 sum of squares is exact in
  any order, so the three kernels' summation orders cannot differ and the
  tensor norm is exactly the fp32 value the case names.  Only the two
  ``scale = 1/3`` cases have no such norm: ``third-inactive`` keeps the norm
  well below the clip, where ``denom = clip`` whatever the norm's last bit is,
  and stays exact; ``third-active`` is the one case of the unfused test held
  to the yardstick instead (``exact`` is False).
* ``fused_case``: the replay contents and weights of the three regimes (clip
  active / inactive / zero critic gradient) for the paths that compute their
  own gradient (``update``, ``update_all``, MATD3), with a loaded state.
"""
from math import isqrt

import numpy as np

F32, F64 = np.float32, np.float64
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
CHUNK = 256                         # MDP_RA_CHUNK: parameters per k_reduce_apply workgroup
ACT = 5

WRONG = ("no_clip", "norm_unscaled", "c1c2_swapped", "eps_in_sqrt", "alpha_no_sqrt", "polyak_swapped",
         "clip_per_chunk")


class Hyper:
    """the step's constants as the device holds them: fp32 values (MdpConfig's
    floats; pa, pb as apply_args rounds them), cast to `dtype`"""

    def __init__(self, dtype, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, clip=0.5, tau=1e-2):
        f = dtype
        self.dtype = f
        self.lr, self.b1, self.b2, self.eps, self.clip = (f(F32(x)) for x in (lr, b1, b2, eps, clip))
        t = float(F32(tau))
        self.pa, self.pb = f(F32(1.0 - t)), f(F32(1.0 - (1.0 - t)))


def sum_squares(gs):
    """the fp64 sum of squares of an fp32 (or fp64) vector"""
    x = np.asarray(gs, F64)
    return float(np.sum(x * x))


def alpha_of(hp, b1p, b2p, wrong=None):
    f = hp.dtype
    one = f(1)
    if wrong == "alpha_no_sqrt":
        return f(hp.lr / (one - f(b1p)))
    return f(hp.lr * np.sqrt(one - f(b2p)) / (one - f(b1p)))


def polyak(hp, target, theta, wrong=None):
    f = hp.dtype
    pa, pb = (hp.pb, hp.pa) if wrong == "polyak_swapped" else (hp.pa, hp.pb)
    return (pa * np.asarray(target, f) + pb * np.asarray(theta, f)).astype(f)


def advance_powers(hp, b1p, b2p):
    f = hp.dtype
    return f(f(b1p) * hp.b1), f(f(b2p) * hp.b2)


def tensor_step(hp, theta, m, v, g, b1p, b2p, scale, target=None, wrong=None):
    """(theta', m', v', target' or None, info) of one tensor; info: the norm and denom used"""
    f = hp.dtype
    theta, m, v = (np.asarray(x, f) for x in (theta, m, v))
    one = f(1)
    gs = (np.asarray(g, f) * f(F32(scale))).astype(f)
    with np.errstate(over="ignore", under="ignore"):
        if wrong == "clip_per_chunk":
            norm = np.concatenate([np.full(len(gs[c:c + CHUNK]), np.sqrt(sum_squares(gs[c:c + CHUNK])))
                                   for c in range(0, len(gs), CHUNK)])
        else:
            norm = np.sqrt(sum_squares(np.asarray(g, f) if wrong == "norm_unscaled" else gs))
        norm = np.asarray(F32(norm) if f is F32 else norm, f)      # (float)sqrt(ss) on the device
        denom = np.maximum(norm, hp.clip)
        gc = gs if wrong == "no_clip" else ((gs * hp.clip) / denom).astype(f)
        c1, c2 = one - hp.b1, one - hp.b2
        if wrong == "c1c2_swapped":
            c1, c2 = c2, c1
        alpha = alpha_of(hp, b1p, b2p, wrong)
        mo = (m + (gc - m) * c1).astype(f)
        vo = (v + (gc * gc - v) * c2).astype(f)
        root = np.sqrt(vo + hp.eps) if wrong == "eps_in_sqrt" else np.sqrt(vo) + hp.eps
        tho = (theta - (mo * alpha) / root).astype(f)
    tgo = None if target is None else polyak(hp, target, tho, wrong)
    return tho, mo, vo, tgo, {"norm": norm, "denom": denom, "alpha": alpha, "gc": gc, "gs": gs}


def net_step(hp, tensors, b1p, b2p, scale, with_polyak, wrong=None):
    """tensors: six dicts {theta, target, m, v, g} -> six dicts of the stepped
    values (target unchanged without Polyak), and the advanced beta powers"""
    out = []
    for t in tensors:
        th, m, v, tg, info = tensor_step(hp, t["theta"], t["m"], t["v"], t["g"], b1p, b2p, scale,
                                         t["target"] if with_polyak else None, wrong)
        out.append({"theta": th, "m": m, "v": v, "target": np.asarray(t["target"], hp.dtype) if tg is None else tg,
                    "info": info})
    return out, advance_powers(hp, b1p, b2p)


def bound(r32, r64, factor=4.0):
    """the yardstick: per entry max(factor x the tensor's worst |fp32 restatement -
    fp64 restatement|, one fp32 spacing of the value) -- what |device - r64| is held to
    where a case has no exact norm"""
    r64 = np.asarray(r64, F64)
    y = float(np.max(np.abs(np.asarray(r32, F64) - r64))) if r64.size else 0.0
    return np.maximum(factor * y, np.spacing(np.abs(r64).astype(F32)).astype(F64))


# ------------------------------------------------------------ exact norms
def four_squares(r):
    """non-negative integers a >= b >= c >= d with a^2 + b^2 + c^2 + d^2 == r (Lagrange)"""
    r = int(r)
    a = isqrt(r)
    while a >= 0:
        r1 = r - a * a
        b = isqrt(r1)
        while b >= 0 and 3 * b * b >= r1:
            r2 = r1 - b * b
            c = isqrt(r2)
            while c >= 0 and 2 * c * c >= r2:
                d = isqrt(r2 - c * c)
                if d * d == r2 - c * c:
                    return a, b, c, d
                c -= 1
            b -= 1
        a -= 1
    raise AssertionError(r)


def ints_with_norm(n, N, rng, big_at=None, share=0.6):
    """n integers whose squares sum to N^2 exactly: n - 5 small ones (1..8, random
    sign), one entry that carries `share` of what they leave (share = 1: as much
    as an integer can) and four that close the remainder.  big_at: where the
    carrying entry goes (default: a random place).  n == 1: [N]"""
    N = int(N)
    if n == 1:
        return np.array([N], np.int64)
    assert n >= 5, n
    small = rng.integers(1, 9, size=n - 5) * rng.choice([-1, 1], size=n - 5)
    S = int(np.sum(small.astype(np.int64) ** 2))
    assert S < N * N, (n, N, S)
    a = isqrt(int((N * N - S) * share)) if share < 1 else isqrt(N * N - S)
    rest = np.array(four_squares(N * N - S - a * a), np.int64) * rng.choice([-1, 1], size=4)
    k = np.concatenate([small, rest]).astype(np.int64)
    rng.shuffle(k)
    at = int(rng.integers(0, n)) if big_at is None else int(big_at)
    k = np.insert(k, at, -a if rng.random() < 0.5 else a)
    assert len(k) == n and sum(int(x) ** 2 for x in k) == N * N
    return k


def grad_with_norm(n, norm_int, unit_exp, rng, big_at=None, share=0.6):
    """fp32 gradient k * 2^unit_exp with tensor norm norm_int * 2^unit_exp exactly"""
    k = ints_with_norm(n, norm_int, rng, big_at, share)
    assert np.abs(k).max() < 2 ** 24
    g = np.ldexp(k.astype(F64), unit_exp).astype(F32)
    assert np.array_equal(g.astype(F64), np.ldexp(k.astype(F64), unit_exp))
    return g


def pow2_norm_grad(n, norm_exp, rng, big_at=None, spread=True):
    """gradient of norm 2^norm_exp: the power-of-two integer norm N is chosen so the
    small entries carry a good part of it (spread) or almost none (one entry carries it)"""
    S = 26 * max(n - 5, 0)                      # about the small entries' sum of squares
    j = 1
    while 4 ** j <= 2 * S:
        j += 1
    if not spread:
        j += 8
    return grad_with_norm(n, 2 ** j, norm_exp - j, rng, big_at, share=0.6 if spread else 1.0)


# ------------------------------------------------------------------ cases
def net_sizes(dims, agent, net, H):
    """device sizes of the six tensors of (agent, net) for full-width actions"""
    cin = sum(dims) + ACT * len(dims)
    if net == 0:
        return [dims[agent] * H, H, H * H, H, H * ACT, ACT]
    return [cin * H, H, H * H, H, H, 1]


def loaded_state(n, rng):
    return {"theta": rng.normal(0, 0.3, n).astype(F32), "target": rng.normal(0, 0.3, n).astype(F32),
            "m": rng.normal(0, 0.05, n).astype(F32), "v": rng.uniform(1e-6, 1e-2, n).astype(F32)}


def powers_at(t, hp=None):
    """(b1^t, b2^t) as the device reaches them: t - 1 fp32 products from (b1, b2)"""
    hp = hp or Hyper(F32)
    p1, p2 = hp.b1, hp.b2
    for _ in range(t - 1):
        p1, p2 = advance_powers(hp, p1, p2)
    return p1, p2


def step_count_powers():
    """({name: (b1p, b2p)} of the step-count group, the step t at which b1^t is the last normal fp32)"""
    hp = Hyper(F32)
    tiny = np.finfo(F32).tiny
    out = {"t1": powers_at(1), "t2": powers_at(2), "t50": powers_at(50)}
    p1, t = hp.b1, 1
    while F32(p1 * hp.b1) >= tiny:
        p1, t = F32(p1 * hp.b1), t + 1
    late = powers_at(7000)[1]
    out["last-normal"] = (p1, late)
    sub = p1
    for _ in range(60):
        sub = F32(sub * hp.b1)
    assert 0 < sub < tiny
    out["subnormal"] = (sub, late)
    out["b1p-zero"] = (F32(0), late)
    return out, t


GROUPS = {"clip": 9, "one-chunk": 6, "loaded": 4, "steps": 6, "scale": 5}
CLIP_EXP = -1                                  # clip = 0.5 = 2^-1


def build_cases(sizes, seed=0):
    """the constructed states of one net (six tensor sizes).  Each case: name, group,
    exact (the norm is an exact fp32 value on every tensor), t (six dicts theta /
    target / m / v / g), b1p, b2p, scale, norm (per tensor: the exact norm of the
    scaled gradient, None where it has none), active (per tensor: clip active)"""
    rng = np.random.default_rng(1000 + seed)
    big = int(np.argmax(sizes))                 # the multi-chunk tensor (W2, or the critic's W1)
    p50 = powers_at(50)
    cases = []

    def add(name, group, grads, norms, b1p=p50[0], b2p=p50[1], scale=1.0, exact=True, state=None):
        ts = []
        for q, n in enumerate(sizes):
            st = loaded_state(n, rng) if state is None else state(q, n)
            st["g"] = np.asarray(grads[q], F32)
            assert st["g"].shape == (n,)
            ts.append(st)
        clip = float(Hyper(F32).clip)
        cases.append({"name": name, "group": group, "exact": exact, "t": ts, "b1p": F32(b1p), "b2p": F32(b2p),
                      "scale": F32(scale), "norm": list(norms),
                      "active": [None if x is None else bool(x > clip) for x in norms]})

    def pow2(name, group, e, **kw):
        add(name, group, [pow2_norm_grad(n, e, rng) for n in sizes], [2.0 ** e] * 6, **kw)

    # -- the clip's own boundaries
    pow2("at", "clip", CLIP_EXP)
    up, dn = 2 ** 23 + 1, 2 ** 24 - 1           # the fp32 neighbours of 0.5: 0.5 + 2^-24, 0.5 - 2^-25
    add("above", "clip", [grad_with_norm(n, up, -24, rng) for n in sizes], [float(np.ldexp(up, -24))] * 6)
    add("below", "clip", [grad_with_norm(n, dn, -25, rng) for n in sizes], [float(np.ldexp(dn, -25))] * 6)
    assert F32(np.ldexp(up, -24)) == np.nextafter(F32(0.5), F32(1)) and F32(np.ldexp(dn, -25)) == np.nextafter(F32(0.5), F32(0))
    pow2("far-below", "clip", -10)
    pow2("tiny", "clip", -60)
    pow2("x1e3", "clip", 9)                     # 1024 x clip
    pow2("x1e18", "clip", 59)                   # 2^60 x clip = 1.15e18 x clip
    pow2("huge", "clip", 100)
    add("zero", "clip", [np.zeros(n, F32) for n in sizes], [0.0] * 6)

    # -- the norm of a multi-chunk tensor carried by one chunk (norm 4 = 8 x clip)
    nb = sizes[big]
    assert nb >= 3 * CHUNK
    spots = {"first": 5, "middle": (nb // CHUNK // 2) * CHUNK + 100, "last": nb - 1}
    for where, at in spots.items():
        lone = np.zeros(nb, F32)
        lone[at] = 4.0
        for kind in ("lone", "dominant"):
            grads = [pow2_norm_grad(n, 0, rng) for n in sizes]
            grads[big] = lone if kind == "lone" else pow2_norm_grad(nb, 2, rng, big_at=at, spread=False)
            norms = [1.0] * 6
            norms[big] = 4.0
            if kind == "dominant":
                assert abs(grads[big][at]) > 3.9 and np.count_nonzero(grads[big]) >= nb - 4
            add(f"{kind}-{where}", "one-chunk", grads, norms)

    # -- a loaded state
    for name in ("opposed", "v-zero", "v-eps", "polyak"):
        e = -26 if name == "v-eps" else 1       # v-eps: |gc| ~ 1e-8
        grads = [pow2_norm_grad(n, e, rng) for n in sizes]

        def state(q, n, name=name, grads=grads):
            st = loaded_state(n, rng)
            sg = np.where(grads[q] >= 0, F32(1), F32(-1))
            st["m"] = (-sg * np.abs(st["m"]) - sg * F32(1e-3)).astype(F32)
            if name == "v-zero":
                st["v"] = np.zeros(n, F32)
            if name == "v-eps":                 # sqrt(v') of the order of eps = 1e-8, and m small with it
                st["v"] = rng.uniform(0.2e-16, 4e-16, n).astype(F32)
                st["m"] = (st["m"] * F32(1e-7)).astype(F32)
            if name == "polyak":                # pb * theta' far above pa * target: the sum rounds visibly
                st["theta"] = rng.normal(0, 100.0, n).astype(F32)
                st["target"] = rng.normal(0, 1e-3, n).astype(F32)
            return st
        add(name, "loaded", grads, [2.0 ** e] * 6, state=state)

    # -- the step count
    for name, (p1, p2) in step_count_powers()[0].items():
        pow2(name, "steps", 0, b1p=p1, b2p=p2)

    # -- scale: the norm is the scaled gradient's (the slab holds g = gs / scale)
    for s, e in ((1.0, 0), (0.5, 0), (0.125, 0)):       # gs: norm 1 = 2 x clip; g: norm 1, 2, 8
        gs = [pow2_norm_grad(n, e, rng) for n in sizes]
        grads = [(x / F32(s)).astype(F32) for x in gs]
        add(f"s{s}", "scale", grads, [2.0 ** e] * 6, scale=s)
    third = F32(1.0 / 3.0)
    # g of norm 1: clip active on g itself, inactive on gs (norm ~ 1/3 < clip, denom = clip: exact)
    add("third-inactive", "scale", [pow2_norm_grad(n, 0, rng) for n in sizes], [None] * 6, scale=third)
    # g of norm 4: gs of norm ~ 4/3 has no exact value
    add("third-active", "scale", [pow2_norm_grad(n, 2, rng) for n in sizes], [None] * 6, scale=third, exact=False)
    cases[-2]["active"] = [False] * 6
    cases[-1]["active"] = [True] * 6

    got = {g: sum(1 for c in cases if c["group"] == g) for g in GROUPS}
    assert got == GROUPS, got
    return cases


def net_vector(tensors, key, offs, size):
    """the net's flat device span (4-padded tensors at offs, relative to the net) of one field"""
    out = np.zeros(size, F32)
    for t, o in zip(tensors, offs):
        out[o:o + len(t[key])] = t[key]
    return out


# --------------------------------------------- the paths with their own gradient
REGIMES = ("active", "inactive", "zero-critic")
FUSED_DIMS = [6, 5]


def fused_case(regime, B, seed, L=100, H=64, dims=None):
    """helpers.synthetic_trainer_case shaped into one regime, plus a loaded optimizer
    state per agent and net (m, v at the tensors' logical shapes) and beta powers at t = 50:
    active: rewards x 1000 and the critics' output layers x 3000 (huge TD errors and dq/da);
    inactive: rewards x 1e-3 and both output layers x 1e-3 (q, y and dq/da ~ 1e-3);
    zero-critic: every critic and target-critic weight zero, rewards zero (q = y = 0)"""
    from tests.helpers import synthetic_trainer_case
    dims = FUSED_DIMS if dims is None else dims
    c = synthetic_trainer_case(dims, B, L, seed, None, H)
    k_rew, k_out = {"active": (1e3, 3000.0), "inactive": (1e-3, 1e-3), "zero-critic": (0.0, 0.0)}[regime]
    c["data"] = [(o, a, (r * k_rew + 0.0).astype(F32).astype(F64), on, d) for (o, a, r, on, d) in c["data"]]
    rng = np.random.default_rng(seed + 500)
    for p in c["params"]:
        for w in ("critic", "tgt_critic"):
            for k in NAMES:
                if regime == "zero-critic":
                    p[w][k] = np.zeros_like(p[w][k])
                elif k in ("W3", "b3"):
                    p[w][k] = (p[w][k] * F32(k_out)).astype(F32)
        for w in ("actor", "critic"):
            p["m_" + w] = {k: rng.normal(0, 0.05, v.shape).astype(F32) for k, v in p[w].items()}
            p["v_" + w] = {k: rng.uniform(1e-6, 1e-2, v.shape).astype(F32) for k, v in p[w].items()}
    c["regime"] = regime
    c["powers"] = powers_at(50)
    return c


def clip_sides(grads, hp=None):
    """per tensor name: +1 norm > clip, -1 norm < clip (0: exactly at it) of a dict of gradients"""
    hp = hp or Hyper(F32)
    out = {}
    for k in NAMES:
        nrm = F32(np.sqrt(sum_squares(np.asarray(grads[k], F32))))
        out[k] = int(np.sign(float(nrm) - float(hp.clip)))
    return out


def regime_sides(regime):
    """what the regime promises: {net: side of every tensor, or None where it promises nothing}"""
    return {"active": {1: 1, 0: 1}, "inactive": {1: -1, 0: -1}, "zero-critic": {1: -1, 0: None}}[regime]
