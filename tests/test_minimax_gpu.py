"""GPU tests of M3DDPG (mdp_minimax_enable) against tests/minimax_oracle.py.

Trainer-only handles on injected indices and uniforms (tests/minimax_cases.py).
Tolerances are those of tests/test_gpu_parity.py: critic loss 1e-5 relative,
the other stats 2e-5, reduced gradients 1e-5 of the tensor's largest entry,
parameters 2e-4 -- at the authors' eps (1e-3 / 1e-5) and at eps = 0.3 for every
pair, on batch rows whose ReLU inputs keep a 1e-5 margin at the unperturbed and
at the perturbed critic inputs (minimax_oracle.clean_idx).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd import _lib  # noqa: E402
from maddpg_amd.engine import Engine  # noqa: E402
from tests import minimax_cases as mc  # noqa: E402
from tests import minimax_oracle as mo  # noqa: E402
from tests import mixed_width  # noqa: E402
from tests.helpers import joint_rows  # noqa: E402

UPD_CTR = 642   # Ctl::upd_ctr, in 32-bit words (mdp_topo.h)


def _engine(c, name, eps="case", **kw):
    """a handle of case `name` with c's replay and weights; eps: the case's matrix
    ("case"), None (a MADDPG handle) or a matrix"""
    k = c["spec"] if "spec" in c else mc.CASES[name]
    mixed = any(w != 5 for w in c["widths"])
    if isinstance(eps, str):
        eps = c["eps"]
    kw.setdefault("lr", c.get("lr", 1e-2))
    eng = Engine(k["dims"], c["local_q"], num_units=k["H"], batch_size=k["B"], capacity=mc.L + 7,
                 act_dims=c["widths"] if mixed else None, minimax_eps=eps, **kw)
    rows = mixed_width.joint_rows_w(c["data"], k["dims"]) if mixed else joint_rows(c["data"], k["dims"])
    eng.add_rows(torch.from_numpy(rows))
    for i, p in enumerate(c["params"]):
        for w in mc.NETS4:
            eng.set_params(i, w, p[w])
    return eng


def _general(monkeypatch, c, name, **kw):
    """a MADDPG handle forced onto the general gradient kernels"""
    monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
    eng = _engine(c, name, eps=None, **kw)
    monkeypatch.delenv("MDP_GENERAL_GRADS")
    return eng


def _update(eng, c, i):
    eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
               u_act=torch.from_numpy(c["u_act"][i]))


def _state(eng, i):
    out = {w: eng.get_params(i, w) for w in Engine.SETS}
    out["beta"] = {f"net{k}": eng.get_beta_powers(i, k) for k in (0, 1)}
    return out


def _assert_equal(a, b, tag):
    for w in a:
        for k in a[w]:
            assert np.array_equal(a[w][k], b[w][k]), (tag, w, k)


# ---- 1. eps = 0 is the MADDPG update of the general kernels, bit for bit
@pytest.mark.parametrize("name", list(mc.CASES))
def test_eps_zero_equals_maddpg_on_the_general_kernels(monkeypatch, name):
    c = mc.make_case(name, "zero")
    n = len(c["params"])
    plain = _general(monkeypatch, c, name)
    eng = _engine(c, name)
    assert not eng.minimax_info().any()
    for r in range(3):
        for i in range(n):
            _update(plain, c, i)
            _update(eng, c, i)
            if r in (0, 2):
                assert plain.stats(i) == eng.stats(i), (r, i)
                _assert_equal(_state(plain, i), _state(eng, i), (r, i))


# ---- 2. agents that see no other action are untouched by any eps
@pytest.mark.parametrize("which", ["all_local_q", "one_agent"])
def test_agents_without_other_actions_equal_maddpg(monkeypatch, which):
    if which == "all_local_q":
        name, c = "spread", mc.make_case("spread", "large")
        c["local_q"] = [True] * 3
        rng = np.random.default_rng(5)
        from oracle import nets
        for j, p in enumerate(c["params"]):     # DDPG critics: [obs_j | act_j] inputs
            p["critic"] = nets.xavier_init(rng, 18 + 5, 1, 64)
            p["tgt_critic"] = nets.xavier_init(rng, 18 + 5, 1, 64)
        plain = _general(monkeypatch, c, name)
        eng = _engine(c, name)
        n = 3
    else:
        from tests.helpers import synthetic_trainer_case
        c = synthetic_trainer_case([4], 40, mc.L, 3)
        n = 1

        def one(eps):
            e = Engine([4], batch_size=40, capacity=mc.L + 7, minimax_eps=eps)
            e.add_rows(torch.from_numpy(joint_rows(c["data"], [4])))
            for w in mc.NETS4:
                e.set_params(0, w, c["params"][0][w])
            return e
        monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
        plain = one(None)
        monkeypatch.delenv("MDP_GENERAL_GRADS")
        eng = one(np.full((1, 1), 0.3, np.float32))
    for r in range(2):
        for i in range(n):
            _update(plain, c, i)
            _update(eng, c, i)
            assert plain.stats(i) == eng.stats(i), (r, i)
            _assert_equal(_state(plain, i), _state(eng, i), (r, i))


# ---- 3 + 4. update parity and the perturbed actions against the oracle
def _adv_check(got, want_n, ss, own, widths, eps_row, tag):
    """device a^ [B, n, 5] against the oracle's logical a^; `own`: the updating agent.
    Bound per (row, agent j): 2e-6 for the unperturbed action (the stats' absolute
    tolerance; entries are probabilities) + eps_j * 2 * 1e-5 * gmax_j / |g_j[row]| --
    the gradient tolerance (1e-5 of the largest entry, here of g_j over the batch)
    through the normalisation, whose first-order error is at most 2 |dg| / |g|."""
    want = mo.pad5(want_n)
    for j, w in enumerate(widths):
        assert not got[:, j, w:].any(), (tag, j, "pad entries")
    skip = mo.ill_conditioned(ss)
    assert skip.mean() <= 0.05, (tag, skip.mean())
    worst = 0.0
    for j in range(len(widths)):
        err = np.abs(got[:, j] - want[:, j]).max(-1)[~skip]
        tol = np.full(err.shape, 2e-6)
        if j != own:
            norm = np.sqrt(np.asarray(ss[j], np.float64))
            tol = tol + float(eps_row[j]) * 2e-5 * norm.max() / norm[~skip]
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (tag, j, float(err.max()), float((err / tol).max()))
    print(f"{tag}: a^ worst error / bound {worst:.3f} over {int((~skip).sum())} rows")
    return got[:, own]


def _update_parity(eng, ags, c, i, tag):
    """agent i's update on the handle and on the oracle agents (both move), held to the
    tolerances of the module docstring; returns (device stats, oracle stats, oracle extras)"""
    _update(eng, c, i)
    got = eng.stats(i)
    want, ex = mc.oracle_update(ags, c, i)
    print(f"{tag} agent {i}: stats {got} oracle {want}")
    assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]) + 1e-7, (i, got[0], want[0])
    np.testing.assert_allclose(got[1:], want[1:], rtol=2e-5, atol=2e-6)
    for w, ref in (("g_critic", ex["grad_critic"]), ("g_actor", ex["grad_actor"])):
        dg = eng.get_params(i, w)
        for k in ref:
            r = np.asarray(ref[k], np.float64).reshape(dg[k].shape)
            scale = float(np.abs(r).max()) or 1.0
            err = float(np.abs(dg[k] - r).max()) / scale
            assert err < 1e-5, (i, w, k, err)
    sets = {"actor": ags[i].actor, "critic": ags[i].critic, "tgt_actor": ags[i].tgt_actor,
            "tgt_critic": ags[i].tgt_critic, "m_actor": ags[i].opt_actor.m, "v_actor": ags[i].opt_actor.v,
            "m_critic": ags[i].opt_critic.m, "v_critic": ags[i].opt_critic.v}
    for w, ref in sets.items():
        dev = eng.get_params(i, w)
        for k in ref:
            err = float(np.abs(dev[k] - np.asarray(ref[k]).reshape(dev[k].shape)).max())
            assert err < 2e-4, (i, w, k, err)
    return got, want, ex


@pytest.mark.parametrize("kind", mc.EPS)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_update_parity_and_perturbed_actions(name, kind):
    c = mc.make_case(name, kind)
    n = len(c["params"])
    eng = _engine(c, name)
    assert np.array_equal(eng.minimax_info(), c["eps"] * (1 - np.eye(n, dtype=np.float32)))
    adv_c, adv_a = eng.minimax_debug_adv()
    ags = mc.oracle_agents(c)
    for i in range(n):
        adv_c.zero_()
        adv_a.zero_()
        _, _, ex = _update_parity(eng, ags, c, i, f"{name} {kind}")
        gc, ga = adv_c.cpu().numpy(), adv_a.cpu().numpy()
        if c["local_q"][i]:           # today's kernels ran: nothing is written
            assert not gc.any() and not ga.any()
            continue
        own_c = _adv_check(gc, ex["adv_critic"], ex["ss_critic"], i, c["widths"], c["eps"][i],
                           (name, kind, i, "critic"))
        own_a = _adv_check(ga, ex["adv_actor"], ex["ss_actor"], i, c["widths"], c["eps"][i],
                           (name, kind, i, "actor"))
        # a^_i == a~_i bitwise: the agent's own slot is what the unperturbed step samples
        assert np.all(np.abs(own_c.sum(-1) - 1) < 1e-5) and np.all(np.abs(own_a.sum(-1) - 1) < 1e-5)
    if kind == "large":               # ... shown against a handle with eps = 0 on the same inputs
        for i in range(n):
            if c["local_q"][i]:
                continue
            pair = [_engine(c, name, eps=np.zeros((n, n), np.float32)), _engine(c, name)]
            (zc, za), (ec, ea) = [e.minimax_debug_adv() for e in pair]
            for e in pair:
                _update(e, c, i)
                e.synchronize()
            assert torch.equal(zc[:, i], ec[:, i]) and torch.equal(za[:, i], ea[:, i]), i
            assert not torch.equal(zc, ec) and not torch.equal(za, ea), i


# ---- 5. graphs, train steps, counters
def _round_engine(c, name, graphs, eps="case", monkeypatch=None):
    eng = _general(monkeypatch, c, name, seed=5) if eps is None else _engine(c, name, eps=eps, seed=5)
    eng.seed_py_random(77)
    eng.set_graphs(graphs)
    return eng


@pytest.mark.parametrize("name", ["spread", "tag"])
def test_update_round_graphs_equal_eager_and_counters_are_maddpgs(monkeypatch, name):
    c = mc.make_case(name, "large")
    n = len(c["params"])
    engs = [_round_engine(c, name, g) for g in (True, False)]
    plain = _round_engine(c, name, True, eps=None, monkeypatch=monkeypatch)
    for r in range(4):
        for e in engs + [plain]:
            e.update_round()
    for e in engs + [plain]:
        e.synchronize()
    for i in range(n):
        _assert_equal(_state(engs[0], i), _state(engs[1], i), i)
        assert engs[0].stats(i) == engs[1].stats(i)
    ctl = [e.region("ctl", torch.int32).cpu().numpy() for e in engs + [plain]]
    assert ctl[0][UPD_CTR] == ctl[1][UPD_CTR] == ctl[2][UPD_CTR] == 4 * n
    assert np.array_equal(engs[0].get_rng_state(), engs[1].get_rng_state())
    assert np.array_equal(engs[0].get_rng_state(), plain.get_rng_state())
    assert engs[0].check_finite() == 0


def _scn_engine(graphs, eps, monkeypatch=None):
    from maddpg_amd.envs import spec
    sp = spec("simple_adversary")
    kw = dict(batch_size=32, capacity=4096, num_envs=16, scenario="simple_adversary", num_adversaries=1, seed=9)
    if eps is None:
        monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
        eng = Engine(sp.obs_dims, **kw)
        monkeypatch.delenv("MDP_GENERAL_GRADS")
    else:
        eng = Engine(sp.obs_dims, minimax=True, adv_eps=eps, adv_eps_s=eps / 100, **kw)
    eng.init_params(3)
    eng.seed_py_random(4)
    eng.env_reset()
    eng.set_graphs(graphs)
    return eng


def test_train_step_graphs_equal_eager_equal_single_rounds(monkeypatch):
    """simple_adversary, 16 env copies, B = 32: train_step(2) with graphs on and off, and
    the same steps issued as env_step + two update_round calls, are bit-equal; with
    eps = 0 they are the MADDPG steps of the general kernels, noise counters included"""
    engs = [_scn_engine(g, 0.3) for g in (True, False, False)]
    zero, plain = _scn_engine(True, 0.0), _scn_engine(True, None, monkeypatch)
    for e in engs[:2] + [zero, plain]:
        for _ in range(3):
            e.train_step(2)
        e.train_steps([1, 2, 0, 1])
    for _ in range(3):
        engs[2].env_step()
        engs[2].update_round()
        engs[2].update_round()
    for k in (1, 2, 0, 1):
        engs[2].env_step()
        for _ in range(k):
            engs[2].update_round()
    for e in engs + [zero, plain]:
        e.synchronize()
    for i in range(3):
        _assert_equal(_state(engs[0], i), _state(engs[1], i), ("graphs", i))
        _assert_equal(_state(engs[0], i), _state(engs[2], i), ("single rounds", i))
        _assert_equal(_state(zero, i), _state(plain, i), ("eps 0", i))
    assert torch.equal(engs[0].region("replay"), engs[1].region("replay"))
    assert torch.equal(engs[0].region("replay"), engs[2].region("replay"))
    rng = [e.get_rng_state() for e in engs + [zero, plain]]
    assert all(np.array_equal(rng[0], r) for r in rng[1:3]) and np.array_equal(rng[3], rng[4])
    ctr = [int(e.region("ctl", torch.int32)[UPD_CTR]) for e in engs + [zero, plain]]
    assert ctr == [3 * 10] * 5, ctr                     # 10 rounds of 3 agents
    assert not torch.equal(engs[0].region("theta"), zero.region("theta"))
    assert engs[0].check_finite() == 0


# ---- 6. refusals
def test_refusals_leave_the_handle_training():
    name = "spread"
    c = mc.make_case(name, "authors")
    n = len(c["params"])
    eng = _engine(c, name)
    idx = torch.from_numpy(c["idx"][0]).to(eng.device)
    eps = np.ascontiguousarray(c["eps"])

    def refused(fn, *a, match):
        with pytest.raises(_lib.MdpError, match=match):
            fn(*a)

    buf = torch.empty(eng.lib.mdp_td3_bytes(eng.cfg), dtype=torch.uint8, device=eng.device)
    pbuf = torch.empty(eng.lib.mdp_per_bytes(eng.cfg), dtype=torch.uint8, device=eng.device)
    refused(eng._c, "mdp_minimax_enable", _lib.fptr(eps), match="mdp_minimax_enable: already enabled")
    refused(eng._c, "mdp_td3_enable", eng._ptr(buf), buf.numel(), 2, match="mdp_td3_enable: .*M3DDPG")
    refused(eng._c, "mdp_per_enable", eng._ptr(pbuf), pbuf.numel(), 0.6, 0.4, 0.001, 0.01, 1.0,
            match="mdp_per_enable: .*M3DDPG")
    refused(eng.set_update_mode, "throughput", match="mdp_set_update_mode")
    refused(eng.update_all, match="mdp_update_all")
    refused(eng.dp_init, 2, 0, b"\0" * 128, match="mdp_dp_init")
    refused(eng.dp_xgmi_open, 2, 0, match="mdp_dp_xgmi_open")
    refused(eng.critic_grad, 0, idx, match="mdp_critic_grad")
    refused(eng.actor_grad, 0, idx, match="mdp_actor_grad")
    refused(eng.reduce_grad, 0, 1, match="mdp_reduce_grad")
    refused(eng.apply_grad, 0, 1, match="mdp_apply_grad")
    host = np.zeros((mc.CASES[name]["B"], n, 5), np.float32)
    refused(eng._c, "mdp_minimax_debug_adv", host.ctypes.data, None, match="mdp_minimax_debug_adv: critic_adv_dev")
    refused(eng._c, "mdp_minimax_debug_adv", None, host.ctypes.data, match="mdp_minimax_debug_adv: actor_adv_dev")
    _update(eng, c, 0)                                  # still trains
    assert eng.check_finite() == 0

    # a MADDPG handle: enable's own argument checks, then the order rule
    plain = _engine(c, name, eps=None)
    out = np.zeros((n, n), np.float32)
    refused(plain._c, "mdp_minimax_info", _lib.fptr(out), match="mdp_minimax_info")
    refused(plain._c, "mdp_minimax_debug_adv", None, None, match="mdp_minimax_debug_adv")
    refused(plain._c, "mdp_minimax_enable", None, match="mdp_minimax_enable: eps_host")
    for bad in (-1e-3, np.nan, np.inf):
        e2 = eps.copy()
        e2[0, 1] = bad
        refused(plain._c, "mdp_minimax_enable", _lib.fptr(e2), match="mdp_minimax_enable: eps_host")
    _update(plain, c, 0)                                # a refused enable leaves a MADDPG handle
    refused(plain._c, "mdp_minimax_enable", _lib.fptr(eps), match="before the handle's first update")
    _update(plain, c, 1)

    # either order: after prioritized replay, MATD3, throughput mode; several GPUs
    k = mc.CASES[name]
    with pytest.raises(_lib.MdpError, match="minimax"):
        Engine(k["dims"], batch_size=k["B"], capacity=mc.L + 7, minimax=True, prioritized=True)
    with pytest.raises(_lib.MdpError, match="minimax"):
        Engine(k["dims"], batch_size=k["B"], capacity=mc.L + 7, minimax=True, td3=True)
    per = Engine(k["dims"], batch_size=k["B"], capacity=mc.L + 7, prioritized=True)
    refused(per._c, "mdp_minimax_enable", _lib.fptr(eps), match="prioritized replay")
    td3 = Engine(k["dims"], batch_size=k["B"], capacity=mc.L + 7, td3=True)
    refused(td3._c, "mdp_minimax_enable", _lib.fptr(eps), match="MATD3")
    tp = Engine(k["dims"], batch_size=k["B"], capacity=mc.L + 7)
    tp.set_update_mode("throughput")
    refused(tp._c, "mdp_minimax_enable", _lib.fptr(eps), match="strict update mode")
    with pytest.raises((ValueError, _lib.MdpError)):
        Engine(k["dims"], batch_size=k["B"], capacity=mc.L + 7, minimax=True, world_size=2)
