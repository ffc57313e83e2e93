"""GPU: Box action spaces (mdp_set_act_spaces) -- diagonal-Gaussian policies
through the sampling sites, the general gradient kernels, the env and the
evaluation launch, against the restatement of tests/box_actions.py.

Gradients, stats and parameters are compared as tests/test_act_dims_gpu.py's
_check_agent does, with its tolerances.  The one number of its own is the
sampled action's tolerance: the larger of the project's atol 2e-6 and four
times the float32 restatement's own deviation from the float64 one on the same
case (the device's log / exp / sincospi are the libm forms, a few ulp).
"""
import copy
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd import _lib  # noqa: E402
from maddpg_amd.engine import Engine  # noqa: E402
from oracle import mpe, nets, philox, trainer  # noqa: E402
from tests import box_actions as ba  # noqa: E402
from tests import eval_oracle as eo  # noqa: E402
from tests import mixed_width as mw  # noqa: E402
from tests.helpers import row_layout  # noqa: E402
from tests.test_act_dims_gpu import _bits, _check_agent  # noqa: E402

ACT = 5
SETS = ("actor", "critic", "tgt_actor", "tgt_critic")
BOX2, BOX1 = ("box", 2), ("box", 1)
D3, D5 = ("discrete", 3), ("discrete", 5)

# name -> (dims, spaces, B, local_q, H); L = 64 rows everywhere
ROUND_CASES = {
    "box2_box2_b16": ([6, 4], [BOX2, BOX2], 16, None, 64),
    "box2_box2_b40": ([6, 4], [BOX2, BOX2], 40, None, 64),          # a partial last tile
    "d3_box2": ([3, 11], [D3, BOX2], 16, None, 64),
    "box2_d5": ([11, 3], [BOX2, D5], 16, None, 64),
    "box1_d5_box2": ([5, 7, 4], [BOX1, D5, BOX2], 16, None, 64),
    "ddpg_critic": ([6, 4], [BOX2, D5], 16, [True, False], 64),
    "h128": ([6, 4], [BOX2, BOX1], 16, None, 128),
}
L = 64


def _engine(c, B, H=64, **kw):
    eng = Engine(c["dims"], c["local_q"], num_units=H, batch_size=B, capacity=L + 7, act_dims=c["widths"],
                 act_kinds=c["kinds"], **kw)
    eng.add_rows(torch.from_numpy(mw.joint_rows_w(c["data"], c["dims"])))
    for i, p in enumerate(c["params"]):
        for w in SETS:
            eng.set_params(i, w, p[w])
    return eng


def _agents(c):
    return [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][i]) for i, p in enumerate(c["params"])]


def _case(name, seed=51):
    dims, spaces, B, local_q, H = ROUND_CASES[name]
    return ba.box_case(dims, spaces, B, L, seed, local_q, H), B, H


class _fp64:
    """the float64 restatement: what every float32 order approximates"""

    def __enter__(self):
        self.old = (nets.F32, trainer.F32)
        nets.F32 = trainer.F32 = np.float64

    def __exit__(self, *exc):
        nets.F32, trainer.F32 = self.old


def _sample_tol(fn):
    """(want32, tolerance): fn() under the float32 and the float64 restatement"""
    w32 = fn()
    with _fp64():
        w64 = fn()
    dev32 = float(np.abs(w32.astype(np.float64) - w64).max())
    return w32, w64, max(2e-6, 4.0 * dev32), dev32


# ------------------------------------------------------------------ act
@pytest.mark.parametrize("name", list(ROUND_CASES))
def test_act_logits_and_target_act_match_the_restatement(name):
    c, B, H = _case(name)
    eng = _engine(c, B, H)
    agents = _agents(c)
    worst = (0.0, 0.0)
    for j, sp in enumerate(c["spaces"]):
        obs = c["data"][j][0][:B].astype(np.float32)
        flat = eng.actor_logits(j, torch.from_numpy(obs)).cpu().numpy()
        assert flat.shape == (B, ba.head_w(sp))
        np.testing.assert_allclose(flat, nets.mlp_fwd(agents[j].actor, obs)[0], atol=2e-6)
        for target in (False, True):
            u = c["u_act"][j]
            got = eng.act(j, torch.from_numpy(obs), target=target, u=torch.from_numpy(u)).cpu().numpy()
            assert got.shape == (B, ba.act_w(sp))
            _w32, w64, tol, dev32 = _sample_tol(lambda: ba.act(agents[j], obs, u, sp, target))
            err = float(np.abs(got - w64).max())
            print(f"{name} agent {j} {sp} target={target}: device |a - a64| = {err:.3e}, "
                  f"float32 restatement {dev32:.3e}, tolerance {tol:.3e}")
            assert err <= tol, (j, target, err, tol)
            if ba.is_box(sp):
                worst = (max(worst[0], err), max(worst[1], dev32))
                # only the first two uniforms are read: [B, 2] is the same call
                got2 = eng.act(j, torch.from_numpy(obs), target=target, u=torch.from_numpy(u[:, :2])).cpu().numpy()
                assert np.array_equal(got, got2)
    print(f"{name}: Box samples, worst device deviation {worst[0]:.3e}, worst float32 restatement {worst[1]:.3e}")


def test_device_noise_is_the_first_two_uniforms_of_the_pinned_streams():
    """no injected uniforms: act draws uniforms5 on stream 0x40000 | agent << 1 |
    target at the handle's act counter; a Box agent uses u[0], u[1] of them"""
    key = 0x5EED5EED00C0FFEE
    c, B, H = _case("box1_d5_box2")
    eng = _engine(c, B, H, seed=key)
    agents = _agents(c)
    ctr = 0
    for j in (0, 2):
        for target in (False, True):
            obs = c["data"][j][0][:B].astype(np.float32)
            got = eng.act(j, torch.from_numpy(obs), target=target).cpu().numpy()
            u = philox.uniforms5(key, 0x40000 | (j << 1) | int(target), ctr, np.arange(B))
            ctr += 1
            _w32, w64, tol, _d = _sample_tol(lambda: ba.act(agents[j], obs, u, c["spaces"][j], target))
            assert float(np.abs(got - w64).max()) <= tol


def test_nan_in_the_unread_uniforms_changes_no_bit():
    c, B, H = _case("box1_d5_box2")
    out = []
    for fill in (0.25, np.nan):
        u_tgt, u_act = c["u_tgt"].copy(), c["u_act"].copy()
        for j in (0, 2):                    # the Box agents read u[0], u[1] only
            u_tgt[:, j, :, 2:] = fill
            u_act[j, :, 2:] = fill
        eng = _engine(c, B, H)
        for i in range(3):
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(u_tgt[i]),
                       u_act=torch.from_numpy(u_act[i]))
        eng.synchronize()
        res = _bits(eng) + [np.asarray(eng.stats(i)).view(np.uint64) for i in range(3)]
        for j in (0, 2):
            obs = torch.from_numpy(c["data"][j][0][:B].astype(np.float32))
            res.append(eng.act(j, obs, u=torch.from_numpy(u_act[j])).cpu().numpy().view(np.uint32))
        out.append(res)
        assert eng.check_finite() == 0
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------- strict rounds
def _check_adam(eng, i, agents):
    """Adam m / v against the restatement's: m is (1 - b1) x the clipped gradient,
    bounded like the gradients (1e-5 of the tensor's scale); v holds its square"""
    for net, opt in (("actor", agents[i].opt_actor), ("critic", agents[i].opt_critic)):
        for slot, ref, tol in (("m", opt.m, 1e-5), ("v", opt.v, 2e-5)):
            dev = eng.get_params(i, f"{slot}_{net}")
            for k in ref:
                r = np.asarray(ref[k], np.float64).reshape(dev[k].shape)
                scale = float(np.abs(r).max()) or 1.0
                assert float(np.abs(dev[k] - r).max()) / scale < tol, (i, net, slot, k)


def _anchor(eng, agents):
    """the restatement takes the device's state: every agent's four parameter sets and
    its Adam m / v (the beta powers are equal already, and stay checked).  Adam's m and
    v carry a weight's earlier steps, so after an update in which its gradient was
    ill-conditioned (|g| <= 1e-3 max|g|, where a few ulp of g move m / sqrt(v) freely)
    the weight keeps that update's deviation: two float32 summation orders of the
    restatement itself differ by 1.5e-6 after two rounds on weights the second
    gradient calls well-conditioned.  Anchored before each later round, every update
    is the one-step comparison _check_agent's bounds are made for."""
    for i, ag in enumerate(agents):
        for w in SETS:
            dev = eng.get_params(i, w)
            ref = getattr(ag, w)
            for k in ref:
                ref[k] = dev[k].reshape(ref[k].shape).astype(np.float32)
        for net, opt in (("actor", ag.opt_actor), ("critic", ag.opt_critic)):
            for slot, ref in (("m", opt.m), ("v", opt.v)):
                dev = eng.get_params(i, f"{slot}_{net}")
                for k in ref:
                    ref[k] = dev[k].reshape(ref[k].shape).astype(np.float32)


@pytest.mark.parametrize("name", list(ROUND_CASES))
def test_strict_round_parity(name):
    """stats, raw gradients, parameters, targets and Adam m / v of every agent's
    update in each of three rounds, by tests/test_act_dims_gpu.py::_check_agent with
    its tolerances and _check_adam.  Round one starts from the case's parameters;
    before rounds two and three the restatement is anchored on the device's state
    (_anchor), whose deviation from the unanchored restatement is asserted first,
    at _check_agent's every-weight bound 2e-4."""
    c, B, H = _case(name)
    eng = _engine(c, B, H)
    n = len(c["dims"])
    assert [eng.lib.mdp_grad_variant(eng.h, i) for i in range(n)] == [0] * n
    assert eng.act_kinds == c["kinds"] and eng.act_dims == c["widths"]
    agents = _agents(c)
    for rnd in range(3):
        if rnd:
            for i in range(n):              # what the rounds so far left between the two, before it is taken over
                for w in SETS:
                    dev = eng.get_params(i, w)
                    for k, ref in getattr(agents[i], w).items():
                        assert np.abs(dev[k] - ref.reshape(dev[k].shape)).max() < 2e-4, (rnd, i, w, k)
            _anchor(eng, agents)
        wg = ww = 0.0
        for i in range(n):
            k = (i + rnd) % n               # other rows and noise each round
            eng.update(i, idx=torch.from_numpy(c["idx"][k]), u_tgt=torch.from_numpy(c["u_tgt"][k]),
                       u_act=torch.from_numpy(c["u_act"][k]))
            got = eng.stats(i)
            want, og = ba.update(agents, i, c["data"], c["idx"][k], c["u_tgt"][k], c["u_act"][k], c["spaces"])
            g, w = _check_agent(eng, i, agents, got, want, og)
            _check_adam(eng, i, agents)
            wg, ww = max(wg, g), max(ww, w)
        print(f"box round {rnd + 1} {name}: worst grad |diff|/max|g| = {wg:.3e}, worst param |diff| = {ww:.3e}")
    assert eng.check_finite() == 0


def test_update_round_graph_equals_eager():
    """mdp_update_round (device-drawn indices and noise) captured and eager: bit-identical"""
    c, B, H = _case("box1_d5_box2", seed=57)
    res = []
    for graphs in (True, False):
        eng = _engine(c, B, H, seed=9)
        eng.seed_py_random(5)
        eng.set_graphs(graphs)
        for _ in range(3):
            eng.update_round()
        eng.synchronize()
        res.append(_bits(eng))
        assert eng.check_finite() == 0
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["box1_d5_box2", "ddpg_critic"])
def test_pad_entries_stay_exactly_zero(name):
    c, B, H = _case(name, seed=58)
    eng = _engine(c, B, H)
    mask = ba.pad_masks(eng, c)
    n = len(c["dims"])
    want = 0
    for i in range(n):
        want += (ACT - c["heads"][i]) * (H + 1)
        want += H * ((ACT - c["widths"][i]) if c["local_q"][i] else sum(ACT - w for w in c["widths"]))
    assert mask.sum() == want and want > 0
    for _ in range(3):
        for i in range(n):
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                       u_act=torch.from_numpy(c["u_act"][i]))
    eng.synchronize()
    for region in ("theta", "target", "adam_m", "adam_v", "grad"):
        r = eng.region(region).cpu().numpy()[:eng.param_floats]
        assert np.isfinite(r).all()
        assert (r[mask] == 0.0).all(), region
        assert (r[~mask] != 0.0).any(), region
    # the sampled action's pad entries in the device's 5-wide slot
    for j in range(n):
        obs = torch.from_numpy(c["data"][j][0][:B].astype(np.float32)).to(eng.device)
        out = torch.full((B, ACT), 7.0, device=eng.device)
        eng._c("mdp_act", j, 0, eng._ptr(obs), eng._ptr(out), B, None)
        eng.synchronize()
        assert (out[:, c["widths"][j]:] == 0).all() and (out[:, :c["widths"][j]] != 0).all()


def test_all_discrete_kinds_are_the_default_bit_for_bit():
    from tests.helpers import joint_rows, synthetic_trainer_case
    dims, B, LL = [18, 18, 18], 48, 300
    c = synthetic_trainer_case(dims, B, LL, seed=43)
    res = []
    for kw in ({}, {"act_kinds": ["discrete"] * 3, "act_dims": [5, 5, 5]}):
        eng = Engine(dims, batch_size=B, capacity=LL + 7, **kw)
        assert eng.act_dims == [5, 5, 5] and eng.act_kinds == ["discrete"] * 3
        assert [eng.lib.mdp_grad_variant(eng.h, i) for i in range(3)] == [1, 1, 1]
        eng.add_rows(torch.from_numpy(joint_rows(c["data"], dims)))
        for i, p in enumerate(c["params"]):
            for w in SETS:
                eng.set_params(i, w, p[w])
        for _ in range(3):
            for i in range(3):
                eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                           u_act=torch.from_numpy(c["u_act"][i]))
        eng.synchronize()
        res.append(_bits(eng) + [np.asarray(eng.stats(i)).view(np.uint64) for i in range(3)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# --------------------------------------------------------------- contract
def _i32(*w):
    return (ctypes.c_int32 * _lib.MAX_AGENTS)(*w)


def test_set_act_spaces_contract():
    eng = Engine([3, 11], batch_size=8, capacity=64)
    lib, h = eng.lib, eng.h
    D, X = _lib.ACT_DISCRETE, _lib.ACT_BOX
    for kinds, dims, msg in (((X, D), (0, 5), b"1 or 2"), ((X, D), (3, 5), b"1 or 2"), ((D, X), (5, 5), b"1 or 2"),
                             ((D, D), (0, 5), b"1..5"), ((D, D), (3, 6), b"1..5"), ((2, D), (2, 5), b"unknown kind"),
                             ((-1, D), (2, 5), b"unknown kind")):
        assert lib.mdp_set_act_spaces(h, _i32(*kinds), _i32(*dims)) < 0
        assert msg in lib.mdp_last_error(h), (kinds, dims, lib.mdp_last_error(h))
    assert lib.mdp_set_act_spaces(h, None, _i32(2, 5)) < 0 and lib.mdp_set_act_spaces(h, _i32(X, D), None) < 0
    assert lib.mdp_grad_variant(h, 0) == 1
    assert lib.mdp_set_act_spaces(h, _i32(X, D), _i32(2, 5)) == 0
    kk, dd = _i32(), _i32()
    assert lib.mdp_get_act_spaces(h, kk, dd) == 0
    assert list(kk) == [X, D] + [0] * 6 and list(dd) == [2, 5] + [0] * 6
    assert lib.mdp_get_act_dims(h, dd) == 0 and list(dd)[:2] == [2, 5]
    assert lib.mdp_grad_variant(h, 0) == 0 and lib.mdp_grad_variant(h, 1) == 0
    # logical shapes follow at once: W3 [units, 2 d], b3 [2 d], the critic's W1 counts d
    ti = _lib.MdpTensorInfo()
    assert lib.mdp_tensor(h, 0, 0, 4, ctypes.byref(ti)) == 0 and (ti.rows, ti.cols, ti.dev_cols) == (64, 4, 5)
    assert lib.mdp_tensor(h, 0, 1, 0, ctypes.byref(ti)) == 0 and (ti.rows, ti.dev_rows) == (14 + 2 + 5, 14 + 10)
    # still unused: may change again, and mdp_set_act_dims makes every kind Discrete
    assert lib.mdp_set_act_dims(h, _i32(3, 5)) == 0
    assert lib.mdp_get_act_spaces(h, kk, dd) == 0 and list(kk)[:2] == [D, D] and list(dd)[:2] == [3, 5]
    assert lib.mdp_grad_variant(h, 0) == 1
    # refused once the handle has been used
    eng2 = Engine([3, 11], batch_size=8, capacity=64, act_kinds=["box", "discrete"], act_dims=[1, 5])
    assert eng2.act_kinds == ["box", "discrete"] and eng2.head_dim(0) == 2
    eng2.init_params(0)
    assert lib.mdp_set_act_spaces(eng2.h, _i32(X, D), _i32(1, 5)) < 0
    assert b"before the handle's first" in lib.mdp_last_error(eng2.h)
    with pytest.raises(_lib.MdpError, match="before the handle's first"):
        eng2.set_act_spaces(["box", "discrete"], [1, 5])
    with pytest.raises(ValueError, match="1 or 2"):
        Engine([3, 11], batch_size=8, capacity=64, act_kinds=["box", "discrete"], act_dims=[3, 5])
    with pytest.raises(ValueError, match="unknown action kind"):
        Engine([3, 11], batch_size=8, capacity=64, act_kinds=["torus", "discrete"], act_dims=[2, 5])
    with pytest.raises(ValueError, match="one entry"):
        Engine([3, 11], batch_size=8, capacity=64, act_kinds=["box"], act_dims=[2, 5])


def test_scenario_handle_rules():
    from maddpg_amd.envs import spec
    sl = spec("simple_speaker_listener")
    kw = dict(batch_size=8, capacity=64, num_envs=4, scenario="simple_speaker_listener")
    eng = Engine(sl.obs_dims, act_kinds=["discrete", "box"], **kw)           # the listener moves and is silent
    assert eng.act_kinds == ["discrete", "box"] and eng.act_dims == [3, 2]
    for kinds, dims in ((["box", "discrete"], [2, 5]),      # the speaker does not move and speaks
                        (["discrete", "box"], [3, 1]),      # the env needs both force components
                        (["discrete", "discrete"], [3, 4])):
        with pytest.raises(ValueError, match="scenario"):
            Engine(sl.obs_dims, act_kinds=kinds, act_dims=dims, **kw)
    sp = spec("simple_spread")
    eng = Engine(sp.obs_dims, batch_size=8, capacity=64, num_envs=4, scenario="simple_spread",
                 act_kinds=["box", "discrete", "box"])
    assert eng.act_dims == [2, 5, 2]
    assert eng.lib.mdp_set_act_dims(eng.h, _i32(5, 5, 5)) == 0               # back to the scenario's own
    assert eng.lib.mdp_set_act_spaces(eng.h, _i32(1, 0, 1), _i32(2, 5, 2)) == 0
    eng.env_reset()
    assert eng.lib.mdp_set_act_spaces(eng.h, _i32(1, 0, 1), _i32(2, 5, 2)) < 0   # after the first env call


def test_refused_combinations_leave_the_handle_usable():
    c, B, H = _case("d3_box2")
    eng = _engine(c, B, H)
    lib, h = eng.lib, eng.h
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=eng.device)
    eps = (ctypes.c_float * 4)(0.0, 1e-3, 1e-3, 0.0)
    calls = {
        "mdp_per_enable": lambda: lib.mdp_per_enable(h, eng._ptr(buf), buf.numel(), 0.6, 0.4, 0.001, 0.01, 1.0),
        "mdp_td3_enable": lambda: lib.mdp_td3_enable(h, eng._ptr(buf), buf.numel(), 2),
        "mdp_minimax_enable": lambda: lib.mdp_minimax_enable(h, eps),
        "mdp_approx_enable": lambda: lib.mdp_approx_enable(h, eng._ptr(buf), buf.numel(), 1e-3),
        "mdp_set_update_mode": lambda: lib.mdp_set_update_mode(h, 1),
        "mdp_update_all": lambda: lib.mdp_update_all(h, None, None, None),
        "mdp_dp_init": lambda: lib.mdp_dp_init(h, bytes(128), 2, 0),
        "mdp_dp_xgmi_open": lambda: lib.mdp_dp_xgmi_open(h, 2, 0, ctypes.create_string_buffer(64)),
        "mdp_dp_xgmi_connect": lambda: lib.mdp_dp_xgmi_connect(h, bytes(128)),
        "mdp_dp_xgmi_probe": lambda: lib.mdp_dp_xgmi_probe(h, _i32()),
        "mdp_dp_xgmi_enable": lambda: lib.mdp_dp_xgmi_enable(h),
    }
    for name, call in calls.items():
        assert call() < 0, name
        msg = lib.mdp_last_error(h)
        assert name.encode() in msg and b"Box action space" in msg, (name, msg)
    for kw in ({"prioritized": True}, {"td3": True}, {"minimax": True}, {"approx": True}):
        with pytest.raises((_lib.MdpError, ValueError), match="Box action space"):
            Engine(c["dims"], batch_size=B, capacity=L + 7, act_kinds=c["kinds"], act_dims=c["widths"], **kw)
    # the other order: the feature first, then a Box space
    e2 = Engine(c["dims"], batch_size=B, capacity=L + 7, td3=True)
    assert e2.lib.mdp_set_act_spaces(e2.h, _i32(0, 1), _i32(3, 2)) < 0
    assert b"Box action space" in e2.lib.mdp_last_error(e2.h)
    # ... and the handle goes on: one strict round against the restatement
    agents = _agents(c)
    for i in range(2):
        eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                   u_act=torch.from_numpy(c["u_act"][i]))
        want, og = ba.update(agents, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], c["spaces"])
        _check_agent(eng, i, agents, eng.stats(i), want, og)


# -------------------------------------------------------------------- env
def _oracle_scn(name, n, na):
    if name == "simple_tag":
        return mpe.SimpleTag(n_adv=na, n_good=n - na)
    return mpe.SimpleSpread(n)


@pytest.mark.parametrize("E", [16, 20])
@pytest.mark.parametrize("name,n,na,kinds", [("simple_spread", 3, 0, ["box", "box", "box"]),
                                             ("simple_tag", 4, 3, ["box", "discrete", "box", "box"])])
def test_env_step_with_box_actions(name, n, na, kinds, E):
    """mdp_env_step with given actions against oracle.mpe.step(to_mpe5(a)), at the
    tolerances of tests/test_gpu_parity.py::test_env_step_parity; a Discrete agent
    in the same env decodes the old way"""
    from maddpg_amd.envs import spec
    sp = spec(name, n, na if na else None)
    eng = Engine(sp.obs_dims, batch_size=16, capacity=1000, num_envs=E, scenario=name,
                 num_adversaries=sp.num_adversaries, max_episode_len=25, seed=3, act_kinds=kinds)
    assert eng.act_dims == [2 if k == "box" else 5 for k in kinds]
    eng.env_reset()
    sc = _oracle_scn(name, n, na)
    rng = np.random.default_rng(4)
    lay, _ = row_layout(sp.obs_dims)
    for step in range(3):
        act = np.zeros((E, n, ACT), np.float32)        # the device's slots
        ref = np.zeros((E, n, ACT), np.float64)        # what the CPU env decodes
        for j, k in enumerate(kinds):
            if k == "box":
                a = rng.normal(size=(E, 2)).astype(np.float32)
                act[:, j, :2] = a
                ref[:, j] = ba.to_mpe5(a.astype(np.float64))
            else:
                z = rng.normal(size=(E, ACT))
                act[:, j] = (np.exp(z) / np.exp(z).sum(-1, keepdims=True)).astype(np.float32)
                ref[:, j] = act[:, j]
        st = eng.env_state()
        ost = {"pos": st["pos"].astype(np.float64), "vel": st["vel"].astype(np.float64), "goal": st["goal"]}
        obs0 = sc.observation(ost)
        nst, obs1, rew = sc.step(ost, ref)
        eng.env_step(act_in=torch.from_numpy(act))
        got = eng.env_state()
        np.testing.assert_allclose(got["pos"], nst["pos"], atol=2e-5)
        np.testing.assert_allclose(got["vel"], nst["vel"], atol=2e-5)
        rows = eng.replay_rows(step * E, E).cpu().numpy()
        for j in range(n):
            lj, o = lay[j], sp.obs_dims[j]
            np.testing.assert_allclose(rows[:, lj["obs"]:lj["obs"] + o], obs0[j], atol=2e-5)
            np.testing.assert_array_equal(rows[:, lj["act"]:lj["act"] + ACT], act[:, j])
            np.testing.assert_allclose(rows[:, lj["nobs"]:lj["nobs"] + o], obs1[j], atol=2e-5)
            np.testing.assert_allclose(rows[:, lj["rew"]], rew[:, j], rtol=1e-5, atol=5e-5)


# ------------------------------------------------------------- evaluation
T = eo.T
SEED = 0x0123456789ABCDEF
EP = 32
KINDS3 = ["box", "discrete", "box"]


def _eval_engine(case, num_envs):
    return eo.make_engine(case, num_envs, SEED, act_kinds=KINDS3)


@pytest.mark.parametrize("case", ["spread3", "spread3_h128"])
def test_evaluation_is_the_step_chain_bit_for_bit(case):
    """sample-mode returns == the training step chain on the same states and noise
    (one env copy per id, 5 vector steps), with the device's own noise and with
    the same uniforms injected; one matchup cell and one evaluate_q trajectory
    equal evaluate / q_values; mean mode plays the mean"""
    a = _eval_engine(case, 4)
    n = a.n
    ids = np.arange(EP)
    start = a.eval_initial_state(EP, 0)
    u = eo.noise(SEED, n, ids)
    b = _eval_engine(case, EP)
    for i in range(n):      # (the same init seed gives the same parameters: checked, not assumed)
        for k, v in a.get_params(i, "actor").items():
            assert np.array_equal(v, b.get_params(i, "actor")[k])
    b.set_env_state(start["pos"], start["vel"], start["goal"])
    rows = []
    for t in range(T):
        b.env_step(u=torch.from_numpy(u[:, t]))
        rows.append(b.replay_rows(t * EP, EP).cpu().numpy())
    b.synchronize()
    assert b.episode_count() == EP
    want = b.episode_log(0, EP)[:, 1:].copy()
    assert np.all(np.isfinite(want)) and np.any(want != 0)
    ret = a.evaluate(EP, 0)["returns"].cpu().numpy()
    np.testing.assert_array_equal(ret, want)
    inj = a.evaluate(EP, 0, u=torch.from_numpy(u))["returns"].cpu().numpy()
    np.testing.assert_array_equal(inj, want)
    # the chain's first actions are the restatement's samples of the device's heads
    lay, _ = row_layout(a.obs_dims)
    for j, k in enumerate(KINDS3):
        lj = lay[j]
        obs = rows[0][:, lj["obs"]:lj["obs"] + a.obs_dims[j]]
        flat = a.actor_logits(j, torch.from_numpy(obs)).cpu().numpy().astype(np.float64)
        sp = ("box", 2) if k == "box" else ("discrete", 5)
        _w32, w64, tol, _d = _sample_tol(lambda: ba.sample(sp, flat.astype(trainer.F32), u[:, 0, j]))
        got = rows[0][:, lj["act"]:lj["act"] + ACT]
        assert float(np.abs(got[:, :sp[1]] - w64).max()) <= tol
        assert (got[:, sp[1]:] == 0).all()
    # one matchup cell: the handle's own actors from a bank
    bank = a.actor_bank(1)
    a.bank_snapshot(bank, 0)
    mu = a.evaluate_matchups(bank, np.zeros((1, n), np.int32), EP, 0)["returns"].cpu().numpy()
    np.testing.assert_array_equal(mu[0], want)
    # one evaluate_q trajectory: the chain's rewards, and q_values on its rows
    q = a.evaluate_q(EP, steps=T, scored=T, u=torch.from_numpy(u))
    cin = a.net_tensors(0, 1)[0][3]
    for t in range(T):
        for j in range(n):
            np.testing.assert_array_equal(q["rew"][:, t, j].cpu().numpy(), rows[t][:, lay[j]["rew"]])
            qv = a.q_values(j, torch.from_numpy(np.ascontiguousarray(rows[t][:, :cin]))).cpu().numpy()
            np.testing.assert_array_equal(q["q"][:, t, j, 0].cpu().numpy(), qv)
    # mean mode: the chain stepped with the heads' means (a Discrete agent: its softmax)
    # Host-side heads and samples are not the rollout's to the bit (another kernel,
    # numpy's libm): the yardstick of tests/test_eval_gpu.py::test_mean_mode -- the
    # same chain with act_in = the restatement's sample of mdp_actor_logits against
    # the exact sample-mode returns -- and its bound, 4 x the yardstick.
    spaces = [("box", 2) if k == "box" else ("discrete", 5) for k in KINDS3]

    def host_chain(fn):
        e = _eval_engine(case, EP)
        e.set_env_state(start["pos"], start["vel"], start["goal"])
        for t in range(T):
            e.env_step(act_in=eo.host_actions(e, lambda j, flat: fn(t, j, flat)))
        e.synchronize()
        return e.episode_log(0, EP)[:, 1:].astype(np.float64)

    yard = float(np.abs(host_chain(lambda t, j, flat: ba.sample(spaces[j], flat, u[:, t, j])) - want).max())
    want_mean = host_chain(lambda t, j, flat: flat[:, :2] if KINDS3[j] == "box" else eo.softmax64(flat))
    got_mean = a.evaluate(EP, 0, mode="mean")["returns"].cpu().numpy()
    assert np.any(got_mean != ret)
    dev = np.abs(got_mean.astype(np.float64) - want_mean)
    bound = np.maximum(4 * yard, np.spacing(np.abs(want_mean)))
    print(f"{case}: yardstick {yard:.3e}, mean-mode deviation {dev.max():.3e}")
    assert np.all(dev <= bound), (yard, float(dev.max()))


# ------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("fmt", ["npz", "tf1"])
def test_checkpoint_round_trip_stores_logical_shapes(tmp_path, fmt):
    c, B, H = _case("box1_d5_box2", seed=59)

    def one_round(eng, r):
        for i in range(3):
            k = (i + r) % 3
            eng.update(i, idx=torch.from_numpy(c["idx"][k]), u_tgt=torch.from_numpy(c["u_tgt"][k]),
                       u_act=torch.from_numpy(c["u_act"][k]))
        eng.synchronize()

    eng = _engine(c, B, H)
    one_round(eng, 0)
    (tmp_path / "ck").mkdir()
    fname = str(tmp_path / "ck" / "model")
    eng.save_state(fname, fmt)
    sd = eng.state_dict()
    cin = 5 + 7 + 4 + 1 + 5 + 2
    assert sd["agent_0/actor/W3"].shape == (64, 2) and sd["agent_0/actor/b3"].shape == (2,)
    assert sd["agent_2/tgt_actor/W3"].shape == (64, 4) and sd["agent_1/actor/W3"].shape == (64, 5)
    assert sd["agent_0/critic/W1"].shape == (cin, 64) and sd["agent_2/v_critic/W1"].shape == (cin, 64)
    if fmt == "npz":
        with np.load(eng.checkpoint_path(fname)) as z:
            assert z["agent_2/actor/W3"].shape == (64, 4) and z["agent_1/m_critic/W1"].shape == (cin, 64)
    else:
        from maddpg_amd.common import tf_checkpoint as tfc
        shapes = {tuple(v.shape) for v in tfc.read_bundle(fname).values()}
        assert {(64, 2), (2,), (64, 4), (4,), (64, 5), (cin, 64)} <= shapes
        assert (16 + 15, 64) not in shapes                  # the device block of the joint critic's W1
    eng2 = Engine(c["dims"], batch_size=B, capacity=L + 7, act_dims=c["widths"], act_kinds=c["kinds"])
    eng2.add_rows(torch.from_numpy(mw.joint_rows_w(c["data"], c["dims"])))
    eng2.load_state(fname)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)
    one_round(eng, 1)
    one_round(eng2, 1)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)
    # a Discrete checkpoint of the same observations does not fit a Box handle, nor the reverse
    disc = Engine(c["dims"], batch_size=B, capacity=L + 7)
    disc.init_params(3)
    dname = str(tmp_path / "ck" / "discrete")
    disc.save_state(dname, fmt)
    with pytest.raises(ValueError, match="does not match the handle's"):
        eng2.load_state(dname)
    with pytest.raises(ValueError, match="does not match the handle's"):
        disc.load_state(fname)


# ----------------------------------------------------------------- facade
def test_trainer_facade_takes_box_spaces():
    """the reference's loop (experiments/train.py:110-161) on the drop-in classes with
    Box entries in act_space_n, the CPU env stepped through to_mpe5"""
    import argparse

    from maddpg_amd.common import tf_util as U
    from maddpg_amd.envs import Box, Discrete
    from maddpg_amd.trainer.maddpg import MADDPGAgentTrainer
    args = argparse.Namespace(lr=1e-2, gamma=0.95, batch_size=64, num_units=64, max_episode_len=5)
    sc = mpe.make("simple_spread")
    rng = np.random.default_rng(0)
    spaces = [Box(2), Discrete(5), Box(2)]
    with pytest.raises(NotImplementedError, match="Box"):
        MADDPGAgentTrainer("x", None, [(18,)] * 3, [Box(3)] * 3, 0, args)
    with U.single_threaded_session():
        trainers = [MADDPGAgentTrainer(f"agent_{i}", None, [(18,)] * 3, spaces, i, args) for i in range(3)]
        U.initialize()
        eng = U.get_session().engine()
        assert eng.act_kinds == ["box", "discrete", "box"] and eng.act_dims == [2, 5, 2]
        st = sc.reset(rng, 1)
        obs_n = [o[0] for o in sc.observation(st)]
        trained = 0
        for t in range(1, 421):
            action_n = [a.action(o) for a, o in zip(trainers, obs_n)]
            assert [a.shape for a in action_n] == [(2,), (5,), (2,)]
            env_act = np.stack([ba.to_mpe5(a) if a.shape == (2,) else a for a in action_n])[None]
            st, new_obs_n, rew = sc.step(st, env_act.astype(np.float64))
            for i, ag in enumerate(trainers):
                ag.experience(obs_n[i], action_n[i], rew[0, i], new_obs_n[i][0], False, t % 5 == 0)
            obs_n = [o[0] for o in new_obs_n]
            if t % 5 == 0:
                st = sc.reset(rng, 1)
                obs_n = [o[0] for o in sc.observation(st)]
            for ag in trainers:
                ag.preupdate()
            for ag in trainers:
                loss = ag.update(trainers, t)
                if loss is not None:
                    trained += 1
                    assert len(loss) == 6 and all(np.isfinite(loss))
        assert trained == 3                 # the gate opens at 320 rows: t = 400
        ob = np.stack([obs_n[0]] * 7)
        assert trainers[0].p_debug["p_values"](ob).shape == (7, 4)          # flat = [mean | logstd]
        assert trainers[0].p_debug["target_act"](ob).shape == (7, 2)
        a2, a5 = np.full((7, 2), 0.2, np.float32), np.full((7, 5), 0.2, np.float32)
        q = trainers[1].q_debug["q_values"](ob, ob, ob, a2, a5, a2)
        assert q.shape == (7,) and np.all(np.isfinite(q))
        # the stored action sits at the head of its 5-wide slot, the pad entries zero
        o, a, _r, _on, _d = trainers[0].replay_buffer.sample_index([0, 1, 2])
        assert a.shape == (3, 2)
        row = eng.replay_rows(0, 1).cpu().numpy()[0]
        lay, _ = row_layout([18, 18, 18])
        assert (row[lay[0]["act"] + 2:lay[0]["act"] + 5] == 0).all() and (row[lay[0]["act"]:lay[0]["act"] + 2] != 0).all()
        assert eng.check_finite() == 0
