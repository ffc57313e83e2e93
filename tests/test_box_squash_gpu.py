"""GPU: tanh-squashed Box policies (mdp_set_act_squash) through the sampling
sites, the general gradient kernels, the env and the evaluation launch, against
the restatement of tests/box_squash.py.

The yardsticks are tests/test_box_actions_gpu.py's: gradients, stats and
parameters by tests/test_act_dims_gpu.py::_check_agent with its tolerances, Adam
m / v by _check_adam, the re-anchoring of _anchor before rounds two and three,
and the sampled action at the larger of 2e-6 and four times the float32
restatement's own deviation from the float64 one on the same case.
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
from oracle import mpe, nets, trainer  # noqa: E402
from tests import box_actions as ba  # noqa: E402
from tests import box_squash as bs  # noqa: E402
from tests import eval_oracle as eo  # noqa: E402
from tests import mixed_width as mw  # noqa: E402
from tests.helpers import row_layout  # noqa: E402
from tests.test_act_dims_gpu import _bits, _check_agent  # noqa: E402
from tests.test_box_actions_gpu import _anchor, _check_adam, _sample_tol  # noqa: E402

ACT = 5
SETS = ("actor", "critic", "tgt_actor", "tgt_critic")
BOX2, D3, D5 = ("box", 2), ("discrete", 3), ("discrete", 5)
T2, T1 = bs.BOX2T, bs.BOX1T

# name -> (dims, spaces, B, local_q, H); L = 64 rows everywhere
ROUND_CASES = {
    "t2_t2_b16": ([6, 4], [T2, T2], 16, None, 64),
    "t2_t2_b40": ([6, 4], [T2, T2], 40, None, 64),                  # a partial last tile
    "d3_t2": ([3, 11], [D3, T2], 16, None, 64),
    "box2_t2": ([6, 4], [BOX2, T2], 16, None, 64),                  # both Box forms in one critic launch's lanes
    "t1_d5_t2": ([5, 7, 4], [T1, D5, T2], 16, None, 64),
    "ddpg_critic": ([6, 4], [T2, D5], 16, [True, False], 64),
    "h128": ([6, 4], [T2, T1], 16, None, 128),
}
L = 64


def _engine(c, B, H=64, squash=True, **kw):
    eng = Engine(c["dims"], c["local_q"], num_units=H, batch_size=B, capacity=L + 7, act_dims=c["widths"],
                 act_kinds=c["kinds"], **({"act_squash": c["squash"]} if squash else {}), **kw)
    eng.add_rows(torch.from_numpy(mw.joint_rows_w(c["data"], c["dims"])))
    for i, p in enumerate(c["params"]):
        for w in SETS:
            eng.set_params(i, w, p[w])
    return eng


def _agents(c):
    return [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][i]) for i, p in enumerate(c["params"])]


def _case(name, seed=51):
    dims, spaces, B, local_q, H = ROUND_CASES[name]
    return bs.squash_case(dims, spaces, B, L, seed, local_q, H), B, H


def _round(eng, c, r=0):
    n = len(c["dims"])
    for i in range(n):
        k = (i + r) % n
        eng.update(i, idx=torch.from_numpy(c["idx"][k]), u_tgt=torch.from_numpy(c["u_tgt"][k]),
                   u_act=torch.from_numpy(c["u_act"][k]))
    eng.synchronize()


# ------------------------------------------------------------------ act
@pytest.mark.parametrize("name", list(ROUND_CASES))
def test_act_logits_and_target_act_match_the_restatement(name):
    c, B, H = _case(name)
    eng = _engine(c, B, H)
    assert eng.act_squash == c["squash"] and eng.act_kinds == c["kinds"]
    agents = _agents(c)
    worst = (0.0, 0.0)
    for j, sp in enumerate(c["spaces"]):
        obs = c["data"][j][0][:B].astype(np.float32)
        flat = eng.actor_logits(j, torch.from_numpy(obs)).cpu().numpy()
        assert flat.shape == (B, ba.head_w(sp))                    # the head is not squashed
        np.testing.assert_allclose(flat, nets.mlp_fwd(agents[j].actor, obs)[0], atol=2e-6)
        for target in (False, True):
            u = c["u_act"][j]
            got = eng.act(j, torch.from_numpy(obs), target=target, u=torch.from_numpy(u)).cpu().numpy()
            assert got.shape == (B, ba.act_w(sp))
            _w32, w64, tol, dev32 = _sample_tol(lambda: bs.act(agents[j], obs, u, sp, target))
            err = float(np.abs(got - w64).max())
            print(f"{name} agent {j} {sp} target={target}: device |a - a64| = {err:.3e}, "
                  f"float32 restatement {dev32:.3e}, tolerance {tol:.3e}")
            assert err <= tol, (j, target, err, tol)
            if bs.is_squashed(sp):
                worst = (max(worst[0], err), max(worst[1], dev32))
                assert np.abs(got).max() <= 1.0
    print(f"{name}: squashed samples, worst device deviation {worst[0]:.3e}, worst float32 restatement {worst[1]:.3e}")


# ---------------------------------------------------------- strict rounds
@pytest.mark.parametrize("name", list(ROUND_CASES))
def test_strict_round_parity(name):
    """tests/test_box_actions_gpu.py::test_strict_round_parity with the squash:
    three rounds by _check_agent and _check_adam, anchored before rounds two and
    three, the deviation taken over asserted first at 2e-4"""
    c, B, H = _case(name)
    eng = _engine(c, B, H)
    n = len(c["dims"])
    assert [eng.lib.mdp_grad_variant(eng.h, i) for i in range(n)] == [0] * n
    assert eng.act_kinds == c["kinds"] and eng.act_dims == c["widths"] and eng.act_squash == c["squash"]
    agents = _agents(c)
    for rnd in range(3):
        if rnd:
            for i in range(n):
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
            want, og = bs.update(agents, i, c["data"], c["idx"][k], c["u_tgt"][k], c["u_act"][k], c["spaces"])
            g, w = _check_agent(eng, i, agents, got, want, og)
            _check_adam(eng, i, agents)
            wg, ww = max(wg, g), max(ww, w)
        print(f"squash round {rnd + 1} {name}: worst grad |diff|/max|g| = {wg:.3e}, worst param |diff| = {ww:.3e}")
    assert eng.check_finite() == 0


def test_the_squash_changes_the_round():
    """the same case with and without the squash differs (the bit is read)"""
    c, B, H = _case("t2_t2_b16")
    res = []
    for squash in (True, False):
        eng = _engine(c, B, H, squash=squash)
        _round(eng, c)
        res.append(_bits(eng))
    assert not np.array_equal(res[0][0], res[1][0])


def test_update_round_graph_equals_eager():
    """mdp_update_round (device-drawn indices and noise) captured and eager: bit-identical"""
    c, B, H = _case("t1_d5_t2", seed=57)
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


@pytest.mark.parametrize("name", ["t1_d5_t2", "ddpg_critic"])
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
    for r in range(3):
        _round(eng, c, r)
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


def test_no_squash_is_a_plain_box_handle_bit_for_bit():
    """a handle on which mdp_set_act_squash was never called meets the plain Box
    restatement as before; one with every squash none equals it bit for bit:
    parameters and stats after a round, and an evaluate call"""
    dims, spaces, B, H = [5, 7, 4], [("box", 1), D5, BOX2], 16, 64
    c = ba.box_case(dims, spaces, B, L, 51, None, H)
    res = []
    for kw in ({}, {"act_squash": ["none", None, 0]}):
        eng = Engine(c["dims"], c["local_q"], num_units=H, batch_size=B, capacity=L + 7, act_dims=c["widths"],
                     act_kinds=c["kinds"], **kw)
        assert eng.act_squash == ["none"] * 3
        eng.add_rows(torch.from_numpy(mw.joint_rows_w(c["data"], c["dims"])))
        for i, p in enumerate(c["params"]):
            for w in SETS:
                eng.set_params(i, w, p[w])
        agents = _agents(c)
        for i in range(3):
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                       u_act=torch.from_numpy(c["u_act"][i]))
            want, og = ba.update(agents, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], c["spaces"])
            _check_agent(eng, i, agents, eng.stats(i), want, og)
        eng.synchronize()
        res.append(_bits(eng) + [np.asarray(eng.stats(i)).view(np.uint64) for i in range(3)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    ev = []
    for kw in ({}, {"act_squash": [None] * 3}):
        e = eo.make_engine("spread3", 4, SEED, act_kinds=KINDS3, **kw)
        ev.append(e.evaluate(EP, 0)["returns"].cpu().numpy())
    np.testing.assert_array_equal(ev[0], ev[1])
    assert np.all(np.isfinite(ev[0]))


# --------------------------------------------------------------- contract
def _i32(*w):
    return (ctypes.c_int32 * _lib.MAX_AGENTS)(*w)


def test_set_act_squash_contract():
    N, TH = _lib.SQUASH_NONE, _lib.SQUASH_TANH
    D, X = _lib.ACT_DISCRETE, _lib.ACT_BOX
    eng = Engine([3, 11], batch_size=8, capacity=64)
    lib, h = eng.lib, eng.h
    sq = _i32()
    assert lib.mdp_get_act_squash(h, sq) == 0 and list(sq) == [0] * 8
    # an all-Discrete handle: zeros pass, a non-zero entry is refused
    assert lib.mdp_set_act_squash(h, _i32(N, N)) == 0
    assert lib.mdp_set_act_squash(h, _i32(TH, N)) < 0 and b"only a Box agent" in lib.mdp_last_error(h)
    assert lib.mdp_set_act_spaces(h, _i32(X, D), _i32(2, 5)) == 0
    assert lib.mdp_set_act_squash(h, _i32(N, TH)) < 0 and b"only a Box agent" in lib.mdp_last_error(h)
    for bad in (2, -1, 4):
        assert lib.mdp_set_act_squash(h, _i32(bad, N)) < 0 and b"unknown squash" in lib.mdp_last_error(h)
    assert lib.mdp_set_act_squash(h, None) < 0 and b"null" in lib.mdp_last_error(h)
    assert lib.mdp_get_act_squash(h, None) < 0
    assert lib.mdp_get_act_squash(h, sq) == 0 and list(sq) == [0] * 8        # a refused call changes nothing
    # round trip; the handle stays a Box handle in everything else
    assert lib.mdp_set_act_squash(h, _i32(TH, N)) == 0
    assert lib.mdp_get_act_squash(h, sq) == 0 and list(sq) == [TH, N] + [0] * 6
    kk, dd = _i32(), _i32()
    assert lib.mdp_get_act_spaces(h, kk, dd) == 0
    assert list(kk) == [X, D] + [0] * 6 and list(dd) == [2, 5] + [0] * 6
    assert lib.mdp_get_act_dims(h, dd) == 0 and list(dd)[:2] == [2, 5]
    assert lib.mdp_grad_variant(h, 0) == 0 and lib.mdp_grad_variant(h, 1) == 0
    ti = _lib.MdpTensorInfo()
    assert lib.mdp_tensor(h, 0, 0, 4, ctypes.byref(ti)) == 0 and (ti.rows, ti.cols, ti.dev_cols) == (64, 4, 5)
    assert lib.mdp_tensor(h, 0, 1, 0, ctypes.byref(ti)) == 0 and (ti.rows, ti.dev_rows) == (14 + 2 + 5, 14 + 10)
    assert lib.mdp_set_act_squash(h, _i32(N, N)) == 0
    assert lib.mdp_get_act_squash(h, sq) == 0 and list(sq) == [0] * 8
    # mdp_set_act_spaces and mdp_set_act_dims reset it
    assert lib.mdp_set_act_squash(h, _i32(TH, N)) == 0
    assert lib.mdp_set_act_spaces(h, _i32(X, D), _i32(2, 5)) == 0
    assert lib.mdp_get_act_squash(h, sq) == 0 and list(sq) == [0] * 8
    assert lib.mdp_set_act_squash(h, _i32(TH, N)) == 0
    assert lib.mdp_set_act_dims(h, _i32(3, 5)) == 0
    assert lib.mdp_get_act_squash(h, sq) == 0 and list(sq) == [0] * 8
    assert lib.mdp_get_act_spaces(h, kk, dd) == 0 and list(kk)[:2] == [D, D] and list(dd)[:2] == [3, 5]
    # a squashed handle is a Box handle to the gate
    assert lib.mdp_set_act_spaces(h, _i32(X, X), _i32(1, 2)) == 0 and lib.mdp_set_act_squash(h, _i32(TH, TH)) == 0
    assert lib.mdp_get_act_dims(h, dd) == 0 and list(dd)[:2] == [1, 2]       # widths untouched by the bit
    assert lib.mdp_set_update_mode(h, 1) < 0 and b"Box action space" in lib.mdp_last_error(h)
    # refused once the handle has been used, with mdp_set_act_spaces' message
    eng2 = Engine([3, 11], batch_size=8, capacity=64, act_kinds=["box", "discrete"], act_dims=[1, 5],
                  act_squash=["tanh", None])
    assert eng2.act_squash == ["tanh", "none"] and eng2.act_kinds == ["box", "discrete"] and eng2.head_dim(0) == 2
    eng2.init_params(0)
    assert lib.mdp_set_act_squash(eng2.h, _i32(TH, N)) < 0
    assert b"mdp_set_act_squash: call it before the handle's first parameter write, act, update or env call" \
        in lib.mdp_last_error(eng2.h)
    with pytest.raises(_lib.MdpError, match="before the handle's first"):
        eng2.set_act_squash(["tanh", "none"])
    assert eng2.act_squash == ["tanh", "none"]
    with pytest.raises(ValueError, match="only a Box agent"):
        Engine([3, 11], batch_size=8, capacity=64, act_kinds=["box", "discrete"], act_dims=[2, 5],
               act_squash=["tanh", "tanh"])
    with pytest.raises(ValueError, match="only a Box agent"):
        Engine([3, 11], batch_size=8, capacity=64, act_squash=["tanh", None])
    with pytest.raises(ValueError, match="unknown action squash"):
        Engine([3, 11], batch_size=8, capacity=64, act_kinds=["box", "discrete"], act_dims=[2, 5],
               act_squash=["clip", None])
    with pytest.raises(ValueError, match="one entry"):
        Engine([3, 11], batch_size=8, capacity=64, act_kinds=["box", "discrete"], act_dims=[2, 5], act_squash=["tanh"])


# -------------------------------------------------------------------- env
def _oracle_scn(name, n, na):
    if name == "simple_adversary":
        return mpe.SimpleAdversary(n_good=n - na, n_adv=na)
    return mpe.SimpleSpread(n)


@pytest.mark.parametrize("E", [16, 20])
@pytest.mark.parametrize("name,n,na", [("simple_spread", 3, 0), ("simple_adversary", 3, 1)])
def test_env_step_on_a_squashed_handle(name, n, na, E):
    """mdp_env_step against oracle.mpe.step(to_mpe5(a)) at the tolerances of
    test_env_step_with_box_actions: first the device's own squashed policies (the
    stored action is inside [-1, 1] and is the force the env applied), then given
    actions at the bounds"""
    from maddpg_amd.envs import spec
    sp = spec(name, n, na if na else None)
    eng = Engine(sp.obs_dims, batch_size=16, capacity=1000, num_envs=E, scenario=name,
                 num_adversaries=sp.num_adversaries, max_episode_len=25, seed=3, act_kinds=["box"] * n,
                 act_squash=["tanh"] * n)
    assert eng.act_dims == [2] * n and eng.act_squash == ["tanh"] * n
    eng.init_params(2)
    eng.env_reset()
    sc = _oracle_scn(name, n, na)
    rng = np.random.default_rng(4)
    lay, _ = row_layout(sp.obs_dims)
    for step in range(4):
        st = eng.env_state()
        ost = {"pos": st["pos"].astype(np.float64), "vel": st["vel"].astype(np.float64), "goal": st["goal"]}
        obs0 = sc.observation(ost)
        if step < 2:
            eng.env_step()
            act = None
        else:
            act = np.zeros((E, n, ACT), np.float32)
            act[:, :, :2] = rng.choice(np.float32([-1.0, 1.0, 0.5]), size=(E, n, 2))
            eng.env_step(act_in=torch.from_numpy(act))
        rows = eng.replay_rows(step * E, E).cpu().numpy()
        stored = np.stack([rows[:, lay[j]["act"]:lay[j]["act"] + ACT] for j in range(n)], 1)
        assert np.abs(stored).max() <= 1.0 and (stored[:, :, 2:] == 0).all() and (stored[:, :, :2] != 0).all()
        if act is not None:
            np.testing.assert_array_equal(stored, act)
        nst, obs1, rew = sc.step(ost, ba.to_mpe5(stored[:, :, :2].astype(np.float64)))
        got = eng.env_state()
        np.testing.assert_allclose(got["pos"], nst["pos"], atol=2e-5)
        np.testing.assert_allclose(got["vel"], nst["vel"], atol=2e-5)
        for j in range(n):
            lj, o = lay[j], sp.obs_dims[j]
            np.testing.assert_allclose(rows[:, lj["obs"]:lj["obs"] + o], obs0[j], atol=2e-5)
            np.testing.assert_allclose(rows[:, lj["nobs"]:lj["nobs"] + o], obs1[j], atol=2e-5)
            np.testing.assert_allclose(rows[:, lj["rew"]], rew[:, j], rtol=1e-5, atol=5e-5)


# ------------------------------------------------------------- evaluation
T = eo.T
SEED = 0x0123456789ABCDEF
EP = 32
KINDS3 = ["box", "discrete", "box"]
SQUASH3 = ["tanh", None, "tanh"]
SPACES3 = [T2, D5, T2]


def _eval_engine(case, num_envs):
    return eo.make_engine(case, num_envs, SEED, act_kinds=KINDS3, act_squash=SQUASH3)


def test_evaluation_is_the_step_chain_bit_for_bit():
    """section 24's spread3 case with the squash: sample-mode returns == the training
    step chain on the same states and noise; one matchup cell and evaluate_q run on
    the squashed handle and equal it; mean mode plays tanh(mean)"""
    case = "spread3"
    a = _eval_engine(case, 4)
    n = a.n
    ids = np.arange(EP)
    start = a.eval_initial_state(EP, 0)
    u = eo.noise(SEED, n, ids)
    b = _eval_engine(case, EP)
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
    # the squash is in the chain: a plain Box handle with the same parameters scores differently
    plain = eo.make_engine(case, 4, SEED, act_kinds=KINDS3)
    assert not np.array_equal(plain.evaluate(EP, 0)["returns"].cpu().numpy(), ret)
    # the chain's first actions are the restatement's samples of the device's heads
    lay, _ = row_layout(a.obs_dims)
    for j, sp in enumerate(SPACES3):
        lj = lay[j]
        obs = rows[0][:, lj["obs"]:lj["obs"] + a.obs_dims[j]]
        flat = a.actor_logits(j, torch.from_numpy(obs)).cpu().numpy().astype(np.float64)
        _w32, w64, tol, _d = _sample_tol(lambda: bs.sample(sp, flat.astype(trainer.F32), u[:, 0, j]))
        got = rows[0][:, lj["act"]:lj["act"] + ACT]
        assert float(np.abs(got[:, :sp[1]] - w64).max()) <= tol
        assert (got[:, sp[1]:] == 0).all()
    for t in range(T):          # every stored action entry of a squashed agent is inside the bounds
        for j in (0, 2):
            assert np.abs(rows[t][:, lay[j]["act"]:lay[j]["act"] + ACT]).max() <= 1.0
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
    # mean mode: the chain stepped with tanh(mean) (a Discrete agent: its softmax), by
    # test_box_actions_gpu's yardstick -- the same host chain with the restatement's
    # sample against the exact sample-mode returns -- and its bound, 4 x the yardstick
    def host_chain(fn):
        e = _eval_engine(case, EP)
        e.set_env_state(start["pos"], start["vel"], start["goal"])
        for t in range(T):
            e.env_step(act_in=eo.host_actions(e, lambda j, flat: fn(t, j, flat)))
        e.synchronize()
        return e.episode_log(0, EP)[:, 1:].astype(np.float64)

    yard = float(np.abs(host_chain(lambda t, j, flat: bs.sample(SPACES3[j], flat, u[:, t, j])) - want).max())
    want_mean = host_chain(lambda t, j, flat: (np.tanh(flat[:, :2].astype(np.float64)).astype(np.float32)
                                               if j != 1 else eo.softmax64(flat)))
    got_mean = a.evaluate(EP, 0, mode="mean")["returns"].cpu().numpy()
    assert np.any(got_mean != ret)
    dev = np.abs(got_mean.astype(np.float64) - want_mean)
    bound = np.maximum(4 * yard, np.spacing(np.abs(want_mean)))
    print(f"{case}: yardstick {yard:.3e}, mean-mode deviation {dev.max():.3e}")
    assert np.all(dev <= bound), (yard, float(dev.max()))


# ------------------------------------------------------------ checkpoints
def test_npz_round_trip_carries_the_squash_and_a_mismatch_is_refused(tmp_path):
    c, B, H = _case("t1_d5_t2", seed=59)
    eng = _engine(c, B, H)
    _round(eng, c, 0)
    (tmp_path / "ck").mkdir()
    fname = str(tmp_path / "ck" / "model")
    eng.save_state(fname)
    with np.load(eng.checkpoint_path(fname)) as z:
        assert z["act_squash"].dtype == np.int32 and z["act_squash"].tolist() == [1, 0, 1]
        assert z["agent_0/actor/W3"].shape == (64, 2) and z["agent_2/actor/W3"].shape == (64, 4)
    eng2 = _engine(c, B, H)
    eng2.load_state(fname)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)
    _round(eng, c, 1)
    _round(eng2, c, 1)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)
    # a handle whose squash differs refuses it, either way round
    plain = _engine(c, B, H, squash=False)
    before = _bits(plain)
    with pytest.raises(ValueError, match="action squash"):
        plain.load_state(fname)
    for a, b in zip(before, _bits(plain)):
        assert np.array_equal(a, b)                     # refused before anything was written
    pname = str(tmp_path / "ck" / "plain")
    plain.save_state(pname)
    with np.load(plain.checkpoint_path(pname)) as z:
        assert "act_squash" not in z.files              # a checkpoint without the array counts as none
    with pytest.raises(ValueError, match="action squash"):
        eng2.load_state(pname)
    plain.load_state(pname)
    # agents=: only the agents restored are compared (agent 1 is Discrete in both)
    plain.load_state(fname, agents=[1])
    with pytest.raises(ValueError, match="action squash"):
        plain.load_state(fname, agents=[0])


def test_tf1_round_trip_loads(tmp_path):
    """a TF1 bundle has no place for the squash: it loads into a handle that was
    given the squash again, and continues bit for bit"""
    c, B, H = _case("t1_d5_t2", seed=59)
    eng = _engine(c, B, H)
    _round(eng, c, 0)
    (tmp_path / "ck").mkdir()
    fname = str(tmp_path / "ck" / "model")
    eng.save_state(fname, "tf1")
    eng2 = _engine(c, B, H)
    eng2.load_state(fname)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)
    _round(eng, c, 1)
    _round(eng2, c, 1)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------- facade
def test_trainer_facade_takes_action_squash():
    """the reference's loop on the drop-in classes with Box entries and
    args.action_squash = "tanh": every action a Box agent returns and stores is
    inside [-1, 1]; without the setting the same entries stay plain Gaussians"""
    import argparse

    from maddpg_amd.common import tf_util as U
    from maddpg_amd.envs import Box, Discrete
    from maddpg_amd.trainer.maddpg import MADDPGAgentTrainer
    base = dict(lr=1e-2, gamma=0.95, batch_size=64, num_units=64, max_episode_len=5)
    spaces = [Box(2), Discrete(5), Box(2)]
    with U.single_threaded_session():
        trainers = [MADDPGAgentTrainer(f"agent_{i}", None, [(18,)] * 3, spaces, i, argparse.Namespace(**base))
                    for i in range(3)]
        U.initialize()
        assert U.get_session().engine().act_squash == ["none"] * 3
    args = argparse.Namespace(action_squash="tanh", **base)
    sc = mpe.make("simple_spread")
    rng = np.random.default_rng(0)
    with U.single_threaded_session():
        trainers = [MADDPGAgentTrainer(f"agent_{i}", None, [(18,)] * 3, spaces, i, args) for i in range(3)]
        U.initialize()
        eng = U.get_session().engine()
        assert eng.act_kinds == ["box", "discrete", "box"] and eng.act_dims == [2, 5, 2]
        assert eng.act_squash == ["tanh", "none", "tanh"]
        st = sc.reset(rng, 1)
        obs_n = [o[0] for o in sc.observation(st)]
        trained = 0
        for t in range(1, 421):
            action_n = [a.action(o) for a, o in zip(trainers, obs_n)]
            assert [a.shape for a in action_n] == [(2,), (5,), (2,)]
            assert np.abs(action_n[0]).max() <= 1.0 and np.abs(action_n[2]).max() <= 1.0
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
        assert trainers[0].p_debug["p_values"](ob).shape == (7, 4)          # flat = [mean | logstd], not squashed
        ta = trainers[0].p_debug["target_act"](ob)
        assert ta.shape == (7, 2) and np.abs(ta).max() <= 1.0
        assert eng.check_finite() == 0
