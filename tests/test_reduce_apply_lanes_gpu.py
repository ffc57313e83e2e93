"""The fused optimizer step with the reduced gradient kept in registers
(reduce_apply_lanes, mdp_apply_fused.hip) against the two
paths it must not differ from: the LDS body of the same launch (MDP_RA_LANES=0)
and k_reduce + k_apply (MDP_UNFUSED_APPLY=1).

Three agents with 18 observations at H = 64, the last one a DDPG agent: the
MADDPG critics' W1 is 69 x 64 = 4,416 parameters (17 chunks and a last chunk of
one wave's quarter), the DDPG critic's 23 x 64 = 1,472 (a last chunk of three
quarters), the actors' 18 x 64 = 1,152 (half a chunk), the biases and the output
layers one wave or less.  One strict round (every agent's update, injected
indices and noise) from tests/optimizer_edges.fused_case's loaded state, at
B = 16, 40, 64, 80, 1000, 1024 -- 1, 3, 4, 5, 63 and 64 partial gradients: fewer
partials than lane groups, a ragged last tile, the full fan-in -- in the regimes
where the clip binds and where it does not.  Everything is compared bit for bit:
theta, targets, Adam m and v, the beta powers, the reduced gradient, the stats.

The two fused bodies sum the partials in one order by construction, and k_reduce
follows it (4 lanes per element up to 64 partials, lane q taking partials q + 4 k,
the same pairwise tree), so all three paths are one step bit for bit.
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd.engine import Engine  # noqa: E402
from tests import optimizer_edges as oe  # noqa: E402
from tests.helpers import joint_rows  # noqa: E402

F32 = np.float32
DIMS, LOCAL_Q = [18, 18, 18], [False, False, True]
BATCHES = {16: 1, 40: 3, 64: 4, 80: 5, 1000: 63, 1024: 64}       # B -> partial gradients (B / 16 rounded up)
REGIMES = ("active", "inactive")
STATE = ("theta", "target", "adam_m", "adam_v")
SETS = ("actor", "tgt_actor", "m_actor", "v_actor", "critic", "tgt_critic", "m_critic", "v_critic")
PATHS = {"lanes": {}, "lds": {"MDP_RA_LANES": "0"}, "unfused": {"MDP_UNFUSED_APPLY": "1"}}
OPT_KINDS = ("reduce_apply", "apply", "reduce")
CTL_FAULT_OFFSET = 2572            # Ctl.fault (mdp_topo.h)


@contextlib.contextmanager
def _environ(env):
    """the switches are read at mdp_create: set around the engine's construction only"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _case(regime, B, H=64, dims=DIMS):
    c = oe.fused_case(regime, B, seed=11, H=H, dims=dims)
    cin = dims[2] + oe.ACT          # the DDPG agent's critic sees its own observation and action only
    p = c["params"][2]
    for w in ("critic", "tgt_critic", "m_critic", "v_critic"):
        p[w] = dict(p[w], W1=np.ascontiguousarray(p[w]["W1"][:cin]))
    return c


def _round(c, B, env, H=64, dims=DIMS):
    """one strict round on a fresh engine created under `env`; every region the round writes"""
    with _environ(env):
        eng = Engine(dims, LOCAL_Q, num_units=H, batch_size=B, capacity=128)
    eng.add_rows(torch.from_numpy(joint_rows(c["data"], dims)))
    for i, p in enumerate(c["params"]):
        for w in SETS:
            eng.set_params(i, w, p[w])
        for k in (0, 1):
            eng.set_beta_powers(i, k, np.array(oe.powers_at(50 + 20 * k + i), F32))
    for k in OPT_KINDS:
        eng.prof_enable(k)
    stats = []
    for i in range(eng.n):
        eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                   u_act=torch.from_numpy(c["u_act"][i]))
        stats.append(np.array(eng.stats(i), np.float64))
    eng.synchronize()
    torch.cuda.synchronize()
    out = {r: eng.region(r).cpu().numpy().copy() for r in STATE + ("beta",)}
    grad = eng.region("grad").cpu().numpy()
    spans = {(i, net): [(off, dr * dc) for (off, _r, _c, dr, dc) in eng.net_tensors(i, net)]
             for i in range(eng.n) for net in (0, 1)}
    out["grad"] = np.concatenate([grad[o:o + n] for key in sorted(spans) for o, n in spans[key]])
    out["stats"] = np.stack(stats)
    ctl = eng.region("ctl", torch.uint8).cpu().numpy()
    fault = int(ctl[CTL_FAULT_OFFSET:CTL_FAULT_OFFSET + 4].view(np.uint32)[0])
    launches = tuple(eng.prof_read(k)[1] for k in OPT_KINDS)
    sides = {key: oe.clip_sides({k: grad[o:o + n] for k, (o, n) in zip(oe.NAMES, spans[key])}) for key in spans}
    sizes = {key: [n for _o, n in spans[key]] for key in spans}
    eng.close()
    return out, fault, launches, sides, sizes


_RUNS = {}


def _runs(regime, B):
    """the three paths' rounds of one case, computed once and shared"""
    key = (regime, B)
    if key not in _RUNS:
        c = _case(regime, B)
        _RUNS[key] = {path: _round(c, B, env) for path, env in PATHS.items()}
    return _RUNS[key]


def _differing(a, b):
    """{region: entries whose bits differ} of two rounds' outputs, empty where they are identical"""
    bad = {}
    for r in a:
        x = np.ascontiguousarray(a[r]).view(np.uint32 if a[r].dtype == F32 else np.uint64)
        y = np.ascontiguousarray(b[r]).view(x.dtype)
        assert x.shape == y.shape, r
        k = int(np.count_nonzero(x != y))
        if k:
            bad[r] = f"{k}/{x.size}"
    return bad


@pytest.mark.parametrize("B", list(BATCHES))
@pytest.mark.parametrize("regime", REGIMES)
def test_register_body_equals_lds_body(regime, B):
    """the same launch with the gradient in registers and through LDS: every bit the same"""
    assert (B + 15) // 16 == BATCHES[B]
    runs = _runs(regime, B)
    (a, fa, la, sides, sizes), (b, fb, lb, _s, _z) = runs["lanes"], runs["lds"]
    assert fa == 0 and fb == 0
    assert la == (6, 0, 0) and lb == (6, 0, 0)      # one k_reduce_apply per net: 2 per agent's update
    # the shapes this file is about: one quarter, three quarters and half of a last chunk
    assert [sizes[(i, 1)][0] % oe.CHUNK for i in range(3)] == [64, 64, 192] and sizes[(0, 0)][0] % oe.CHUNK == 128
    for (i, net), s in sorted(sides.items()):
        print(f"B={B} {regime} agent {i} {'critic' if net else 'actor'}: clip "
              + " ".join(f"{k}:{'on' if v > 0 else 'off'}" for k, v in s.items()))
    want = oe.regime_sides(regime)[1]                # the regime's promise for the MADDPG critics
    assert all(v == want for i in (0, 1) for v in sides[(i, 1)].values()), (regime, sides)
    assert _differing(a, b) == {}


@pytest.mark.parametrize("B", list(BATCHES))
@pytest.mark.parametrize("regime", REGIMES)
def test_register_body_equals_unfused(regime, B):
    """... and k_reduce + k_apply from the same state: every bit the same"""
    runs = _runs(regime, B)
    (a, fa, _la, _s, _z), (b, fb, lb, _s2, _z2) = runs["lanes"], runs["unfused"]
    assert fa == 0 and fb == 0
    assert lb == (0, 6, 6)
    bad = _differing(a, b)
    print(f"B={B} ({BATCHES[B]} partials) {regime}: entries differing from the unfused path: {bad or 'none'}")
    assert bad == {}


def test_two_graph_replayed_steps_equal_eager():
    """training steps with rounds due at B = 64, the last two replayed as a graph: the epoch
    tags survive replay (bit-identical to the eager path, and to the LDS body)"""
    from maddpg_amd.runner import VecRunner
    res = []
    for env, graphs in (({}, True), ({}, False), ({"MDP_RA_LANES": "0"}, True)):
        with _environ(env):
            r = VecRunner("simple_spread", 64, batch_size=64, capacity=20000, seed=3, train_every=16,
                          max_episode_len=5)
        r.eng.set_graphs(graphs)
        r.prefill()
        for _ in range(4):
            assert r.step() == 4
        r.eng.synchronize()
        assert r.eng.check_finite() == 0
        res.append([r.eng.region(k).cpu().numpy().view(np.uint32).copy() for k in STATE + ("beta", "grad")]
                   + [np.array([r.eng.stats(i) for i in range(3)]).view(np.uint64)])
        r.eng.close()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            np.testing.assert_array_equal(a, b)


def test_tensor_above_64_chunks():
    """observations of 60, 60 and 18 at H = 128: the MADDPG critics' W1 is 153 x 128 = 19,584
    parameters, 77 chunks -- a tensor whose chunks outnumber a wave's lanes, so a lane polls a
    second pair -- still as one fused launch per net (at H = 256 the grid is no longer
    co-resident and the step runs unfused); both bodies and the unfused path agree"""
    B, H, dims = 64, 128, [60, 60, 18]
    c = _case("active", B, H, dims)
    runs = {path: _round(c, B, env, H, dims) for path, env in PATHS.items()}
    assert max(runs["lanes"][4][(0, 1)]) > 64 * oe.CHUNK >= max(runs["lanes"][4][(2, 1)])
    assert all(r[1] == 0 for r in runs.values())
    assert runs["lanes"][2] == (6, 0, 0) and runs["unfused"][2] == (0, 6, 6)
    assert _differing(runs["lanes"][0], runs["lds"][0]) == {}
    assert _differing(runs["lanes"][0], runs["unfused"][0]) == {}
