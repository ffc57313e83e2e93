"""tests/optimizer_edges.py without a GPU: the restatement against oracle/nets.py,
the builder's own claims, hand-derived values, and proof that the built cases
see the bugs that today's parity check (theta only, t = 1 from m = v = 0)
cannot."""
import copy
import functools

import numpy as np
import pytest

from oracle import nets, trainer
from tests import optimizer_edges as oe

F32, F64 = np.float32, np.float64
DIMS = [6, 5]
# (agent, net, H): what tests/test_optimizer_edges_gpu.py steps
NETS = {"a64": (0, 0, 64), "c64": (1, 1, 64), "a128": (0, 0, 128), "c128": (1, 1, 128)}


@functools.lru_cache(maxsize=None)
def cases_of(tag):
    agent, net, H = NETS[tag]
    return oe.build_cases(oe.net_sizes(DIMS, agent, net, H), seed=sorted(NETS).index(tag))


def test_numpy_keeps_fp32_subnormals():
    """the restatement's beta powers pass through fp32's subnormal range: numpy must not flush them"""
    p = F32(1.5e-38) * F32(0.5)
    assert 0 < p < np.finfo(F32).tiny and F32(p * F32(2)) == F32(1.5e-38)
    pw, t_last = oe.step_count_powers()
    assert 800 < t_last < 860                       # b1^t leaves the normal range after ~830 steps
    assert 0 < pw["subnormal"][0] < np.finfo(F32).tiny <= pw["last-normal"][0]
    assert F32(pw["last-normal"][0] * F32(0.9)) < np.finfo(F32).tiny
    hp = oe.Hyper(F32)
    for name, (p1, p2) in pw.items():
        a = oe.alpha_of(hp, p1, p2)
        assert np.isfinite(a) and a > 0, name
    # b1p = 0: alpha = lr sqrt(1 - b2p) / 1
    assert oe.alpha_of(hp, F32(0), pw["b1p-zero"][1]) == F32(hp.lr * np.sqrt(F32(1) - pw["b1p-zero"][1]))


def test_case_counts():
    for tag in NETS:
        cs = cases_of(tag)
        assert {g: sum(c["group"] == g for c in cs) for g in oe.GROUPS} == oe.GROUPS
        assert len({c["name"] for c in cs}) == len(cs) == sum(oe.GROUPS.values())
        assert [c["name"] for c in cs if not c["exact"]] == ["third-active"]


def _as_dict(tensors, key, dtype):
    return {k: np.asarray(t[key], dtype).copy() for k, t in zip(oe.NAMES, tensors)}


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("tag", ["a64", "c64"])
def test_restatement_is_the_oracles_clip_adam_polyak(monkeypatch, tag, dtype):
    """fp32: bit for bit the oracle's fp32 step with the fp64-norm clip.  fp64 (the
    oracle's F32 switched to float64, its constants given as the fp32 values): m, v,
    theta and the powers bit for bit; target within 2^-24 (|target| + |theta'|), because
    oracle.nets.polyak then keeps 1 - tau in fp64 where the device rounds pa, pb to fp32"""
    monkeypatch.setattr(nets, "F32", dtype)
    hp = oe.Hyper(dtype)
    f32c = lambda x: float(F32(x))  # noqa: E731
    for c in cases_of(tag):
        want, wp = oe.net_step(hp, c["t"], c["b1p"], c["b2p"], c["scale"], True)
        params = _as_dict(c["t"], "theta", dtype)
        target = _as_dict(c["t"], "target", dtype)
        opt = nets.Adam(params, lr=f32c(1e-2), b1=f32c(0.9), b2=f32c(0.999), eps=f32c(1e-8))
        opt.m, opt.v = _as_dict(c["t"], "m", dtype), _as_dict(c["t"], "v", dtype)
        opt.b1p, opt.b2p = dtype(c["b1p"]), dtype(c["b2p"])
        gs = {k: (np.asarray(t["g"], dtype) * dtype(c["scale"])).astype(dtype) for k, t in zip(oe.NAMES, c["t"])}
        with np.errstate(over="ignore", under="ignore"):
            opt.apply(params, {k: nets.clip_by_norm(v, 0.5, "fp64") for k, v in gs.items()})
        nets.polyak(target, params, tau=f32c(1e-2))
        for k, w in zip(oe.NAMES, want):
            assert params[k].dtype == dtype and w["theta"].dtype == dtype
            assert np.array_equal(params[k], w["theta"]), (c["name"], k)
            assert np.array_equal(opt.m[k], w["m"]) and np.array_equal(opt.v[k], w["v"]), (c["name"], k)
            if dtype is F32:
                assert np.array_equal(target[k], w["target"]), (c["name"], k)
            else:
                lim = 2.0 ** -24 * (np.abs(target[k]) + np.abs(w["theta"])) + 1e-300
                assert np.all(np.abs(target[k] - w["target"]) <= lim), (c["name"], k)
        assert (opt.b1p, opt.b2p) == wp and type(opt.b1p) is dtype


def test_polyak_constants_are_the_oracles():
    hp = oe.Hyper(F32)
    assert hp.pa == F32(1.0 - 1e-2) and hp.pb == F32(1.0 - (1.0 - 1e-2))


def _sum_orders(x):
    """the fp64 sum of squares three ways: numpy's pairwise order, first to last, last to first"""
    sq = np.asarray(x, F64) ** 2
    return float(np.sum(sq)), float(np.cumsum(sq)[-1]), float(np.cumsum(sq[::-1])[-1])


@pytest.mark.parametrize("tag", list(NETS))
def test_builder_conditions(tag):
    hp = oe.Hyper(F32)
    clip = float(hp.clip)
    for c in cases_of(tag):
        out, _ = oe.net_step(hp, c["t"], c["b1p"], c["b2p"], c["scale"], NETS[tag][1] == 0)
        for q, (t, o) in enumerate(zip(c["t"], out)):
            gs = o["info"]["gs"]
            assert t["g"].dtype == F32 and np.all(np.isfinite(t["g"]))
            norm = c["norm"][q]
            if norm is not None:
                # gs is exact, its squares sum exactly in any order, and to the claimed norm's square
                assert np.array_equal(gs.astype(F64), t["g"].astype(F64) * float(c["scale"])), (c["name"], q)
                assert float(F32(norm)) == norm
                s = _sum_orders(gs)
                assert s[0] == s[1] == s[2] == norm * norm, (c["name"], q, s, norm)
                assert float(o["info"]["norm"]) == norm
            else:
                assert c["name"].startswith("third")
                got = float(o["info"]["norm"])
                assert (got < 0.75 * clip) if c["name"] == "third-inactive" else (got > 2 * clip)
            # the clip is active exactly where the case claims it
            assert c["active"][q] == bool(o["info"]["norm"] > hp.clip), (c["name"], q)
            assert (o["info"]["denom"] == hp.clip) == (not c["active"][q])
            if not c["active"][q]:
                assert np.array_equal(o["info"]["gc"], gs), (c["name"], q)      # gc == gs bit for bit
            else:
                assert np.all(np.abs(o["info"]["gc"]) <= np.abs(gs))
                if gs.size > 1:
                    assert not np.array_equal(o["info"]["gc"], gs)
            # gs * clip neither overflows nor loses bits
            assert np.array_equal((gs * hp.clip) / hp.clip, gs) and np.all(np.isfinite(gs * hp.clip))
            for key in ("theta", "m", "v", "target"):
                assert np.all(np.isfinite(o[key])), (c["name"], q, key)
    by = {c["name"]: c for c in cases_of(tag)}
    assert by["at"]["active"] == [False] * 6 and by["below"]["active"] == [False] * 6
    assert by["above"]["active"] == [True] * 6 and by["zero"]["active"] == [False] * 6
    assert by["x1e18"]["norm"][0] == 2.0 ** 59 and by["huge"]["norm"][0] == 2.0 ** 100
    big = int(np.argmax([len(t["g"]) for t in by["lone-first"]["t"]]))
    chunks = set()
    for where in ("first", "middle", "last"):
        g = by[f"lone-{where}"]["t"][big]["g"]
        assert np.count_nonzero(g) == 1
        at = int(np.flatnonzero(g)[0])
        chunks.add(at // oe.CHUNK)
        d = by[f"dominant-{where}"]["t"][big]["g"]
        assert int(np.argmax(np.abs(d))) == at and abs(d[at]) > 0.97 * 4.0
    n_chunks = -(-len(g) // oe.CHUNK)
    assert min(chunks) == 0 and max(chunks) == n_chunks - 1 and len(chunks) == 3
    v = by["v-eps"]["t"][0]
    o = oe.tensor_step(hp, v["theta"], v["m"], v["v"], v["g"], by["v-eps"]["b1p"], by["v-eps"]["b2p"], 1.0)
    assert 0.2e-8 < float(np.sqrt(o[2]).min()) and float(np.sqrt(o[2]).max()) < 4e-8    # sqrt(v') ~ eps = 1e-8
    for t in by["v-zero"]["t"]:
        assert not t["v"].any() and np.all(t["m"] != 0)
    for t in by["opposed"]["t"]:
        assert np.all(np.sign(t["m"]) == -np.where(t["g"] >= 0, 1, -1))


def test_shapes_cover_the_tail_branches():
    """sizes that are no multiple of 4 (b3: the p0 + 3 < n tail), none of 256 (aact, the
    e1 tail of k_apply), a single chunk (nch == 1 skips the handshake) and more than
    one chunk without being chunk-aligned"""
    sizes = sorted({n for (a, net, H) in NETS.values() for n in oe.net_sizes(DIMS, a, net, H)})
    assert any(n % 4 for n in sizes) and 1 in sizes and 5 in sizes
    assert any(n < oe.CHUNK for n in sizes)
    assert any(n > oe.CHUNK and n % oe.CHUNK for n in sizes)
    assert any(n > 1024 and n % 1024 for n in sizes)            # k_apply's chunk is 1024
    assert any(n >= 16 * oe.CHUNK for n in sizes)


def test_hand_derived_scalar_cases():
    one = np.ones(1)
    for f, tol in ((F32, 3e-7), (F64, 2e-8)):       # (fp64 still carries the constants' fp32 rounding)
        hp = oe.Hyper(f)
        # 1. t = 1 from m = v = 0, g = 1 = 2 x clip: gc = 1/2, m' = gc c1, v' = gc^2 c2, and
        #    theta' = -lr gc / (|gc| + eps sqrt(..)/..) = -lr to eps / gc
        th, m, v, tg, info = oe.tensor_step(hp, 0 * one, 0 * one, 0 * one, one, F32(0.9), F32(0.999), 1.0, target=one)
        assert info["norm"] == 1 and info["gc"][0] == 0.5
        assert m[0] == f(0.5) * (f(1) - hp.b1) and v[0] == f(0.25) * (f(1) - hp.b2)
        assert abs(m[0] - 0.05) < tol and abs(v[0] - 0.00025) < 1e-8      # (c2 = 1 - fp32(0.999) is 1.3e-5 off 1e-3)
        assert abs(th[0] + 0.01) < tol
        assert abs(tg[0] - (0.99 - 0.01 * 0.01)) < tol           # pa target + pb theta'
        # 2. a zero gradient moves theta by the carried m alone (decimal constants)
        th, m, v, _, info = oe.tensor_step(hp, one, 0.1 * one, 0.04 * one, 0 * one, 0.9 ** 3, 0.999 ** 3, 1.0)
        assert info["denom"] == hp.clip and info["gc"][0] == 0
        alpha = 0.01 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)
        assert abs(m[0] - 0.09) < tol and abs(v[0] - 0.03996) < tol
        assert abs(th[0] - (1 - 0.09 * alpha / (np.sqrt(0.03996) + 1e-8))) < tol
        # 3. the norm exactly at the clip leaves the gradient as it is; scale enters the norm:
        #    g = 2, scale = 1/4 is that same tensor
        for g, s in ((0.5, 1.0), (2.0, 0.25)):
            _, m, _, _, info = oe.tensor_step(hp, one, 0 * one, 0 * one, g * one, F32(0.9), F32(0.999), s)
            assert info["norm"] == 0.5 and info["gc"][0] == 0.5 and abs(m[0] - 0.05) < tol
        # 4. b1^t = 0 (t beyond ~980): alpha = lr sqrt(1 - b2^t)
        assert abs(oe.alpha_of(hp, 0.0, 0.25) - 0.01 * np.sqrt(0.75)) < tol
    assert oe.advance_powers(oe.Hyper(F32), F32(0.9), F32(0.999)) == (F32(0.9) * F32(0.9), F32(0.999) * F32(0.999))


QUANT = ("theta", "m", "v", "target")


def _excess(hp32, hp64, c, with_polyak, wrong):
    """how far the wrong fp32 variant lies outside what the GPU test allows on case c: the
    largest |wrong - r64| - bound over the quantities (<= 0: the case cannot see it)"""
    r32, _ = oe.net_step(hp32, c["t"], c["b1p"], c["b2p"], c["scale"], with_polyak)
    r64, _ = oe.net_step(hp64, c["t"], c["b1p"], c["b2p"], c["scale"], with_polyak)
    w32, _ = oe.net_step(hp32, c["t"], c["b1p"], c["b2p"], c["scale"], with_polyak, wrong)
    worst = -np.inf
    for a, b, w in zip(r32, r64, w32):
        for key in QUANT:
            lim = oe.bound(a[key], b[key])
            assert np.all(np.abs(a[key].astype(F64) - b[key]) <= lim)       # the right step passes
            worst = max(worst, float(np.max(np.abs(w[key].astype(F64) - b[key]) - lim)))
    return worst


@pytest.mark.parametrize("wrong", oe.WRONG)
def test_cases_see_each_wrong_variant(wrong):
    """each deliberately wrong step leaves the GPU test's tolerance (the yardstick bound,
    which bit-equality implies) on at least one built case"""
    hp32, hp64 = oe.Hyper(F32), oe.Hyper(F64)
    seen = []
    for tag in ("a64", "c64"):
        for c in cases_of(tag):
            if _excess(hp32, hp64, c, NETS[tag][1] == 0, wrong) > 0:
                seen.append((tag, c["group"], c["name"]))
    print(f"{wrong}: seen by {len(seen)} cases, groups {sorted({s[1] for s in seen})}")
    assert seen, wrong
    # and by the group built for it
    want = {"no_clip": "clip", "norm_unscaled": "scale", "clip_per_chunk": "one-chunk", "alpha_no_sqrt": "steps",
            "eps_in_sqrt": "loaded", "c1c2_swapped": "loaded", "polyak_swapped": "loaded"}[wrong]
    assert any(s[1] == want for s in seen), (wrong, want)


def test_todays_theta_check_cannot_see_a_missing_clip():
    """_update_parity's clip check (tests/test_gpu_parity.py): theta only, at t = 1 from
    m = v = 0, to 1e-6 absolute.  There the step is lr g / (|g| + eps / sqrt(c2)), eps /
    sqrt(c2) = 3.2e-7: a common factor of the gradient moves theta by lr x 3.2e-7 x (1 /
    |gc| - 1 / |g|).  On a random gradient of norm 10 x clip whose entries lie within 20 %
    of their rms the step without any clip moves theta by less than the 1e-6; on a
    Gaussian one it shows only at the entries below 0.03 (near-cancelling sums).  m and
    v, which the check now reads too, move by 9/10 and 99/100 of themselves"""
    rng = np.random.default_rng(5)
    hp = oe.Hyper(F32)
    worst = {"theta": 0.0, "m": 0.0, "v": 0.0}
    for n in oe.net_sizes(DIMS, 0, 0, 64):
        for kind in ("even", "gauss"):
            g = rng.normal(size=n) if kind == "gauss" else rng.uniform(0.8, 1.2, n) * rng.choice([-1, 1], n)
            g = (g * (10 * 0.5 / np.sqrt(np.sum(g * g)))).astype(F32)
            z = np.zeros(n, F32)
            theta = rng.normal(0, 0.3, n).astype(F32)
            right = oe.tensor_step(hp, theta, z, z, g, F32(0.9), F32(0.999), 1.0)
            wrong = oe.tensor_step(hp, theta, z, z, g, F32(0.9), F32(0.999), 1.0, wrong="no_clip")
            assert abs(float(right[4]["norm"]) - 5.0) < 1e-5
            d = [np.abs(right[k].astype(F64) - wrong[k]) for k in range(3)]
            if kind == "gauss":
                assert np.all(d[0][np.abs(g) >= 0.03] < 1e-6)
                continue
            for k, key in enumerate(("theta", "m", "v")):
                worst[key] = max(worst[key], float(d[k].max()))
            assert np.all(np.abs(wrong[1]) > 9 * np.abs(right[1]))
    print(f"no clip at t = 1 from m = v = 0, norm 10 x clip: theta moves {worst['theta']:.2e}, "
          f"m {worst['m']:.2e}, v {worst['v']:.2e}")
    assert worst["theta"] < 1e-6
    assert worst["m"] > 1e-3 and worst["v"] > 1e-4


@pytest.mark.parametrize("B", [64, 1040])
@pytest.mark.parametrize("regime", oe.REGIMES)
def test_fused_regimes_hold_on_the_oracle_gradients(regime, B):
    """the replay contents and weights of each regime put every tensor's norm on the
    promised side of the clip with a factor 2 to spare, on the oracle's gradients (the
    actor's after the critic step from the loaded state, as a strict update orders them)"""
    c = oe.fused_case(regime, B, seed=7)
    n = len(oe.FUSED_DIMS)
    hp = oe.Hyper(F32)
    want = oe.regime_sides(regime)
    sets = ("actor", "critic", "tgt_actor", "tgt_critic")
    for i in range(n):
        agents = [trainer.AgentParams(**{w: copy.deepcopy(p[w]) for w in sets}) for p in c["params"]]
        batch_n = [tuple(x[c["idx"][i]] for x in c["data"][j]) for j in range(n)]
        gc = trainer.critic_grads(agents, i, batch_n, c["u_tgt"][i])[0]
        p = c["params"][i]
        ts = [{"theta": p["critic"][k].ravel(), "target": p["tgt_critic"][k].ravel(), "m": p["m_critic"][k].ravel(),
               "v": p["v_critic"][k].ravel(), "g": np.asarray(gc[k], F32).ravel()} for k in oe.NAMES]
        out, _ = oe.net_step(hp, ts, *c["powers"], 1.0, False)
        for k, o in zip(oe.NAMES, out):
            agents[i].critic[k] = o["theta"].reshape(p["critic"][k].shape)
        ga = trainer.actor_grads(agents, i, batch_n, c["u_act"][i])[0]
        for net, g in ((1, gc), (0, ga)):
            norms = {k: float(np.sqrt(oe.sum_squares(np.asarray(g[k], F32)))) for k in oe.NAMES}
            print(regime, B, i, "critic" if net else "actor", {k: f"{v:.3g}" for k, v in norms.items()})
            if regime == "zero-critic" and net == 1:
                assert not any(norms.values())
            elif want[net] == 1:
                assert all(v > 2 * 0.5 for v in norms.values()), (i, net, norms)
            elif want[net] == -1:
                assert all(v < 0.5 / 2 for v in norms.values()), (i, net, norms)
