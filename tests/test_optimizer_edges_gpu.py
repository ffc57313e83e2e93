"""The optimizer step on the device against tests/optimizer_edges.py's restatement
(DESIGN.md section 18): k_reduce + k_apply on crafted gradients from constructed
states, and k_reduce_apply<256> / <1024>, k_reduce_apply_batch, k_polyak and the
MATD3 steps on the gradient each left in the GRAD region.

Tolerance.  Where the builder guarantees an exact tensor norm the device equals
the fp32 restatement bit for bit on theta, target, m, v and the beta powers.
Where it does not (`third-active`, and every gradient a kernel computed itself)
the device is held to the yardstick |device - fp64 restatement| <= max(4 x the
tensor's worst |fp32 restatement - fp64 restatement|, one fp32 spacing of the
value), and the count of bit-equal entries is printed.  Everything a step does
not own -- the other agent, the other net's Adam slots, a critic step's
targets, the pad floats between tensors -- is compared bit for bit with a
snapshot taken before the step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd import _lib  # noqa: E402
from maddpg_amd.engine import Engine  # noqa: E402
from tests import optimizer_edges as oe  # noqa: E402
from tests import td3_oracle  # noqa: E402
from tests.helpers import joint_rows  # noqa: E402
from tests.test_optimizer_edges_oracle import DIMS, NETS, cases_of  # noqa: E402

F32, F64 = np.float32, np.float64
APRE_W, CPRE_W = 144, 212          # MDP_APRE_W, MDP_CPRE_W (mdp_kernels.h)
RA_MAXCH = 256                     # MDP_RA_MAXCH
SENTINEL = 12345.0
CTL_FAULT_OFFSET = 2572            # Ctl.fault (mdp_topo.h)
STATE = ("theta", "target", "adam_m", "adam_v")     # the param-space regions, and a tensor dict's keys for them
KEYS = ("theta", "target", "m", "v")
SETS = {0: ("actor", "tgt_actor", "m_actor", "v_actor"), 1: ("critic", "tgt_critic", "m_critic", "v_critic")}
HP32, HP64 = oe.Hyper(F32), oe.Hyper(F64)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _snapshot(eng):
    eng.synchronize()
    torch.cuda.synchronize()
    snap = {r: eng.region(r).cpu().numpy().copy() for r in STATE + ("beta", "grad")}
    if eng.td3:
        for r in Engine.TD3_REGIONS:
            snap[r] = eng.td3_region(r).cpu().numpy().copy()
    return snap


def _fault(eng):
    ctl = eng.region("ctl", torch.uint8).cpu().numpy()
    return int(ctl[CTL_FAULT_OFFSET:CTL_FAULT_OFFSET + 4].view(np.uint32)[0])


def _spans(eng, agent, net):
    """[(offset, size)] of the six tensors of (agent, net) in the param-space regions"""
    return [(off, dr * dc) for (off, _r, _c, dr, dc) in eng.net_tensors(agent, net)]


def _tensors(snap, spans, regions=STATE, grad="grad"):
    """six dicts theta / target / m / v / g cut from a snapshot"""
    return [dict({k: snap[r][o:o + n] for k, r in zip(KEYS, regions)}, g=snap[grad][o:o + n]) for o, n in spans]


class Tally:
    """per (group, quantity): entries compared, entries bit-equal to the fp32 restatement,
    the worst |device - r64| / bound"""

    def __init__(self):
        self.rows = {}

    def add(self, group, key, got, r32, r64):
        lim = oe.bound(r32, r64)
        ratio = float(np.max(np.abs(got.astype(F64) - r64) / lim)) if got.size else 0.0
        row = self.rows.setdefault((group, key), [0, 0, 0.0])
        row[0] += got.size
        row[1] += int(np.sum(_bits(got) == _bits(r32)))
        row[2] = max(row[2], ratio)
        return ratio

    def report(self, title):
        for (group, key), (n, eq, ratio) in sorted(self.rows.items()):
            print(f"{title} {group:12s} {key:7s}: {eq}/{n} entries bit-equal to the fp32 restatement; "
                  f"worst |device - fp64| / yardstick bound = {ratio:.3g}")


def _check_step(tally, group, name, got, want, snap, spans, regions, r32, r64, exact, with_target):
    """the stepped net's quantities in `got` (region name -> array) against the restatement;
    fills `want` (a copy of the snapshot being turned into the expected regions) with the
    fp32 restatement where exact, else with the device's own values once they passed the yardstick"""
    for q, (o, n) in enumerate(spans):
        for key, reg in zip(KEYS, regions):
            if key == "target" and not with_target:
                continue
            g = got[reg][o:o + n]
            ratio = tally.add(group, key, g, r32[q][key], r64[q][key])
            if exact:
                bad = np.flatnonzero(_bits(g) != _bits(r32[q][key]))
                assert bad.size == 0, (name, oe.NAMES[q], key, bad[:6], g[bad[:6]], r32[q][key][bad[:6]], ratio)
            assert ratio <= 1.0, (name, oe.NAMES[q], key, ratio)
            want[reg][o:o + n] = r32[q][key] if exact else g


def _assert_regions(name, got, want, regions):
    for reg in regions:
        bad = np.flatnonzero(_bits(got[reg]) != _bits(want[reg]))
        assert bad.size == 0, (name, reg, bad[:8], got[reg][bad[:8]], want[reg][bad[:8]])


# ------------------------------------------------ k_reduce + k_apply, full control
def _slab_bytes(n, nwg, B, slab_c, slab_a, row_stride):
    """MDP_R_SLAB as mdp_api.cpp build_layout sizes it (tests/test_reduce_batch_sizes_gpu.py)"""
    ra_sync = _lib.MAX_AGENTS * 2 * 8 * 128 + _lib.MAX_AGENTS * 2 * 6 * RA_MAXCH * 16
    return (n * (4 * nwg * (slab_c + slab_a) + 2 * 8 * 8 * nwg + 8 * B) + 256 + 256 + ra_sync
            + 4 * nwg * 16 * (APRE_W + CPRE_W + 2 * row_stride) + 512)


def _slab_rows(eng, nwg, B):
    n = eng.n
    size = {(i, net): eng.grad_view(i, net).numel() for i in range(n) for net in (0, 1)}
    slab_c = max(size[(i, 1)] for i in range(n))
    slab_a = max(size[(i, 0)] for i in range(n))
    slab = eng.region("slab")
    assert slab.numel() * 4 == _slab_bytes(n, nwg, B, slab_c, slab_a, eng.row_stride), \
        "the SLAB region's layout changed: this test writes its rows by that layout"
    rows_c = slab[:n * nwg * slab_c].view(n * nwg, slab_c)
    rows_a = slab[n * nwg * slab_c: n * nwg * (slab_c + slab_a)].view(n * nwg, slab_a)
    return {1: rows_c, 0: rows_a}, size


@pytest.mark.parametrize("tag", list(NETS))
def test_unfused_step_from_constructed_states(tag):
    """set_params + set_beta_powers, the crafted gradient as slab row 0 (rows 1, 2 zero),
    reduce_grad, apply_grad(agent, net, scale): every region afterwards, bit for bit"""
    agent, net, H = NETS[tag]
    B, nwg = 48, 3
    eng = Engine(DIMS, num_units=H, batch_size=B, capacity=64)
    rng = np.random.default_rng(3)
    for i in range(eng.n):                       # every set of every agent holds something to disturb
        for which in SETS[0] + SETS[1]:
            nfl = sum(r * c for r, c in eng._flat_shapes(i, which))
            lo = 1e-6 if which.startswith("v_") else -0.3
            eng.set_params(i, which, rng.uniform(lo, 0.3, nfl).astype(F32))
        for k in (0, 1):
            eng.set_beta_powers(i, k, oe.powers_at(7 + 3 * i + k))
    spans = _spans(eng, agent, net)
    assert [n for _o, n in spans] == oe.net_sizes(DIMS, agent, net, H)
    assert all((r, c) == (dr, dc) for (_o, r, c, dr, dc) in eng.net_tensors(agent, net))
    other = _spans(eng, agent, 1 - net)
    rows, size = _slab_rows(eng, nwg, B)
    net_off = spans[0][0]
    rel = [o - net_off for o, _n in spans]
    beta_at = agent * 8 + net * 4
    tally, ran = Tally(), {g: 0 for g in oe.GROUPS}
    for c in cases_of(tag):
        for which, key in zip(SETS[net], KEYS):
            eng.set_params(agent, which, np.concatenate([t[key] for t in c["t"]]))
        eng.set_beta_powers(agent, net, np.array([c["b1p"], c["b2p"]], F32))
        rows[net].fill_(float("nan"))
        rows[net][:nwg] = 0.0
        gvec = oe.net_vector(c["t"], "g", rel, size[(agent, net)])
        rows[net][0, :gvec.size] = torch.from_numpy(gvec).to(rows[net].device)
        eng.region("grad").fill_(SENTINEL)
        snap = _snapshot(eng)
        for q, (o, n) in enumerate(spans):       # set_params wrote the tensors where mdp_tensor says they live
            for key, reg in zip(KEYS, STATE):
                assert _same_bits(snap[reg][o:o + n], c["t"][q][key]), (c["name"], q, key)
        eng.reduce_grad(agent, net)
        eng.apply_grad(agent, net, float(c["scale"]))
        got = _snapshot(eng)
        want = {r: a.copy() for r, a in snap.items()}
        want["grad"][net_off:net_off + gvec.size] = gvec
        r32, p32 = oe.net_step(HP32, c["t"], c["b1p"], c["b2p"], c["scale"], net == 0)
        r64, _ = oe.net_step(HP64, c["t"], c["b1p"], c["b2p"], c["scale"], net == 0)
        _check_step(tally, c["group"], c["name"], got, want, snap, spans, STATE, r32, r64, c["exact"], net == 0)
        if net == 0:                             # the actor step's Polyak of the critic's target, from its current theta
            for o, n in other:
                want["target"][o:o + n] = oe.polyak(HP32, snap["target"][o:o + n], snap["theta"][o:o + n])
        want["beta"][beta_at:beta_at + 4] = [p32[0], p32[1], c["b1p"], c["b2p"]]
        _assert_regions(c["name"], got, want, STATE + ("beta", "grad"))
        assert np.all(np.isfinite(got["theta"])) and oe.alpha_of(HP32, c["b1p"], c["b2p"]) > 0
        ran[c["group"]] += 1
    assert _fault(eng) == 0
    tally.report(f"unfused {tag}")
    assert ran == oe.GROUPS


# ---------------------------------------- the paths that compute their own gradient
def _load(eng, c, twins=None):
    eng.add_rows(torch.from_numpy(joint_rows(c["data"], oe.FUSED_DIMS)))
    for i, p in enumerate(c["params"]):
        for w in SETS[0] + SETS[1]:
            eng.set_params(i, w, p[w])
        for k in (0, 1):
            eng.set_beta_powers(i, k, np.array(oe.powers_at(50 + 20 * k + i), F32))
        if twins is not None:
            for w in Engine.TD3_SETS:
                eng.set_params(i, w, twins[i][w])
            eng.set_beta_powers(i, 2, np.array(oe.powers_at(30 + i), F32))


OPT_KINDS = ("reduce_apply", "apply", "reduce")


def _count_optimizer_launches(eng):
    for k in OPT_KINDS:
        eng.prof_enable(k)


def _optimizer_launches(eng):
    """(k_reduce_apply, k_apply or k_polyak, k_reduce) launches since _count_optimizer_launches"""
    return tuple(eng.prof_read(k)[1] for k in OPT_KINDS)


def _restated(snap, spans, b, with_polyak, regions=STATE, grad_from=None, grad="grad"):
    ts = _tensors(dict(snap, **{grad: grad_from[grad]}), spans, regions, grad)
    r32, p32 = oe.net_step(HP32, ts, b[0], b[1], 1.0, with_polyak)
    r64, _ = oe.net_step(HP64, ts, b[0], b[1], 1.0, with_polyak)
    return ts, r32, r64, p32


def _sides(ts):
    return oe.clip_sides({k: t["g"] for k, t in zip(oe.NAMES, ts)})


def _assert_regime(regime, net, ts, where):
    sides = _sides(ts)
    want = oe.regime_sides(regime)[net]
    if regime == "zero-critic" and net == 1:
        assert not any(t["g"].any() for t in ts), where
    if want is not None:
        assert all(s == want for s in sides.values()), (where, regime, net, sides)
    return sides


def _strict_update(eng, c, i, tally, regime, title):
    """one mdp_update of agent i from the engine's current state, checked against the
    restatement on the gradient each step left in GRAD; returns the regions afterwards"""
    snap = _snapshot(eng)
    eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
               u_act=torch.from_numpy(c["u_act"][i]))
    got = _snapshot(eng)
    want = {r: a.copy() for r, a in snap.items()}
    for net in (1, 0):
        spans = _spans(eng, i, net)
        at = i * 8 + net * 4
        ts, r32, r64, p32 = _restated(snap, spans, snap["beta"][at:at + 2], net == 0, grad_from=got)
        sides = _assert_regime(regime, net, ts, title)
        print(f"{title} agent {i} {'critic' if net else 'actor'}: clip "
              + " ".join(f"{k}:{'on' if s > 0 else 'off'}" for k, s in sides.items()))
        _check_step(tally, regime, title, got, want, snap, spans, STATE, r32, r64, False, net == 0)
        want["beta"][at:at + 4] = [p32[0], p32[1], snap["beta"][at], snap["beta"][at + 1]]
    for o, n in _spans(eng, i, 1):              # Polyak of the critic's target from the critic's stepped theta
        want["target"][o:o + n] = oe.polyak(HP32, snap["target"][o:o + n], got["theta"][o:o + n])
    _assert_regions(title, got, want, STATE + ("beta",))
    return snap, got


@pytest.mark.parametrize("B", [64, 1040])
@pytest.mark.parametrize("regime", oe.REGIMES)
def test_fused_update_from_a_loaded_state(monkeypatch, regime, B):
    """mdp_update through k_reduce_apply<256> (B = 64: 4 partials) and <1024> (B = 1040: 65),
    and the same through k_reduce + k_apply (MDP_UNFUSED_APPLY=1); fused and unfused agree
    bit for bit wherever their GRAD regions do"""
    c = oe.fused_case(regime, B, seed=7)
    assert (B + 15) // 16 == (4 if B == 64 else 65)
    out = {}
    for path in ("fused", "unfused"):
        if path == "unfused":
            monkeypatch.setenv("MDP_UNFUSED_APPLY", "1")
        eng = Engine(oe.FUSED_DIMS, batch_size=B, capacity=128)
        _load(eng, c)
        _count_optimizer_launches(eng)
        tally = Tally()
        for i in range(eng.n):
            out[(path, i)] = _strict_update(eng, c, i, tally, regime, f"{path} B={B} {regime}")
        assert _fault(eng) == 0
        # the path really taken: two k_reduce_apply per update, or two k_reduce + k_apply pairs
        assert _optimizer_launches(eng) == ((4, 0, 0) if path == "fused" else (0, 4, 4))
        tally.report(f"{path} B={B}")
    compared = 0
    for i in range(2):
        (sa, a), (sb, b) = out[("fused", i)], out[("unfused", i)]
        for net in (1, 0):
            # the same state before the update and the same gradient: the same step, bit for bit
            # (else each path was held to its own restatement above)
            spans = _spans(eng, i, net)
            same = (all(_same_bits(sa[r], sb[r]) for r in STATE + ("beta",))
                    and all(_same_bits(a["grad"][o:o + n], b["grad"][o:o + n]) for o, n in spans))
            print(f"B={B} {regime} agent {i} {'critic' if net else 'actor'}: fused and unfused start from the same "
                  f"bits with bit-equal GRAD spans: {same}")
            if same:
                compared += 1
                for reg in STATE:
                    for o, n in spans:
                        assert _same_bits(a[reg][o:o + n], b[reg][o:o + n]), (regime, B, i, net, reg)
                at = i * 8 + net * 4
                assert _same_bits(a["beta"][at:at + 4], b["beta"][at:at + 4])
    print(f"B={B} {regime}: {compared} of 4 steps compared fused against unfused")
    if regime == "zero-critic":                  # agent 0's critic gradient is all zeros on both paths
        assert compared >= 1


@pytest.mark.parametrize("B,general", [(64, False), (1040, False), (64, True)])
@pytest.mark.parametrize("regime", oe.REGIMES)
def test_throughput_round_from_a_loaded_state(monkeypatch, regime, B, general):
    """one mdp_update_all round: k_reduce_apply_batch (every net Polyaks its own chunk), and on
    the general kernels the per-agent pairs followed by k_polyak"""
    if general:
        monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
    c = oe.fused_case(regime, B, seed=8)
    eng = Engine(oe.FUSED_DIMS, batch_size=B, capacity=128)
    _load(eng, c)
    eng.set_update_mode("throughput")
    snap = _snapshot(eng)
    eng.update_all(idx=torch.from_numpy(c["idx"]), u_tgt=torch.from_numpy(c["u_tgt"]), u_act=torch.from_numpy(c["u_act"]))
    got = _snapshot(eng)
    want = {r: a.copy() for r, a in snap.items()}
    tally, title = Tally(), f"throughput B={B} general={general} {regime}"
    for i in range(eng.n):
        for net in (1, 0):
            spans = _spans(eng, i, net)
            at = i * 8 + net * 4
            ts, r32, r64, p32 = _restated(snap, spans, snap["beta"][at:at + 2], True, grad_from=got)
            if regime != "active" or net == 1:  # (the actor's gradient here is from the round-start critic)
                _assert_regime(regime, net, ts, title)
            _check_step(tally, regime, title, got, want, snap, spans, STATE, r32, r64, False, True)
            want["beta"][at:at + 4] = [p32[0], p32[1], snap["beta"][at], snap["beta"][at + 1]]
    _assert_regions(title, got, want, STATE + ("beta",))
    assert _fault(eng) == 0
    tally.report(title)


@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("regime", ["active", "inactive"])
def test_td3_update_from_a_loaded_state(monkeypatch, regime, d, unfused):
    """one MATD3 update of agent 0: both critics' steps against g_critic / g_critic2; with
    policy_delay = 1 the actor step and all three targets, with 2 the actor's slots and
    every target bit-unchanged; agent 1 untouched either way"""
    if unfused:
        monkeypatch.setenv("MDP_UNFUSED_APPLY", "1")
    B = 64
    c = oe.fused_case(regime, B, seed=9)
    twins = td3_oracle.twin_case(c, oe.FUSED_DIMS, 9)
    k_out = {"active": 3000.0, "inactive": 1e-3}[regime]
    rng = np.random.default_rng(17)
    for tw in twins:
        for w in ("critic2", "tgt_critic2"):
            for k in ("W3", "b3"):
                tw[w][k] = (tw[w][k] * F32(k_out)).astype(F32)
        tw["m_critic2"] = {k: rng.normal(0, 0.05, v.shape).astype(F32) for k, v in tw["critic2"].items()}
        tw["v_critic2"] = {k: rng.uniform(1e-6, 1e-2, v.shape).astype(F32) for k, v in tw["critic2"].items()}
    eng = Engine(oe.FUSED_DIMS, batch_size=B, capacity=128, td3=True, policy_delay=d)
    _load(eng, c, twins)
    b2_before = [eng.get_beta_powers(i, 2) for i in range(eng.n)]
    _count_optimizer_launches(eng)
    snap = _snapshot(eng)
    eng.update(0, idx=torch.from_numpy(c["idx"][0]), u_tgt=torch.from_numpy(c["u_tgt"][0]),
               u_act=torch.from_numpy(c["u_act"][0]))
    got = _snapshot(eng)
    want = {r: a.copy() for r, a in snap.items()}
    want["grad"], want["grad2"] = got["grad"].copy(), got["grad2"].copy()
    tally, title = Tally(), f"td3 d={d} unfused={unfused} {regime}"
    twin_regions = ("theta2", "target2", "adam_m2", "adam_v2")
    cspans = _spans(eng, 0, 1)
    # critic 1 and critic 2 (no Polyak in their launches)
    ts, r32, r64, p32 = _restated(snap, cspans, snap["beta"][4:6], False, grad_from=got)
    _assert_regime(regime, 1, ts, title)
    _check_step(tally, regime, title + " critic", got, want, snap, cspans, STATE, r32, r64, False, False)
    want["beta"][4:8] = [p32[0], p32[1], snap["beta"][4], snap["beta"][5]]
    ts, r32, r64, p2 = _restated(snap, cspans, b2_before[0], False, twin_regions, grad_from=got, grad="grad2")
    _assert_regime(regime, 1, ts, title)
    _check_step(tally, regime + "/critic2", title + " critic2", got, want, snap, cspans, twin_regions, r32, r64,
                False, False)
    assert tuple(eng.get_beta_powers(0, 2)) == p2
    assert np.array_equal(eng.get_beta_powers(1, 2), b2_before[1])
    if d == 1:
        aspans = _spans(eng, 0, 0)
        ts, r32, r64, p32 = _restated(snap, aspans, snap["beta"][0:2], True, grad_from=got)
        _assert_regime(regime, 0, ts, title)
        _check_step(tally, regime, title + " actor", got, want, snap, aspans, STATE, r32, r64, False, True)
        want["beta"][0:4] = [p32[0], p32[1], snap["beta"][0], snap["beta"][1]]
        for o, n in cspans:                      # both critics' targets from their stepped weights
            want["target"][o:o + n] = oe.polyak(HP32, snap["target"][o:o + n], got["theta"][o:o + n])
            want["target2"][o:o + n] = oe.polyak(HP32, snap["target2"][o:o + n], got["theta2"][o:o + n])
    else:
        assert eng.td3_info(0)["actor_updates"] == 0
    # the path really taken (the second target critic's k_polyak is timed as an apply launch)
    steps = 3 if d == 1 else 2
    assert _optimizer_launches(eng) == ((0, steps + (d == 1), steps) if unfused else (steps, int(d == 1), 0))
    # everything else -- at d = 2 the actor's theta, m, v, beta powers and all three targets -- bit-unchanged
    _assert_regions(title, got, want, STATE + ("beta",) + twin_regions)
    assert _fault(eng) == 0
    tally.report(title)
