"""GPU tests of MADDPG with inferred policies (mdp_approx_enable)
against tests/approx_oracle.py.

Trainer-only handles on injected indices and uniforms: B = 40 (two full 16-row
tiles and a ragged one) unless a case says otherwise, ring L = 200.  Tolerances
are those of tests/test_gpu_parity.py and tests/test_td3_gpu.py: losses 1e-5
relative, raw gradients 1e-5 of their scale, parameter sets 2e-4, beta powers exact.
"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd import _lib  # noqa: E402
from maddpg_amd.engine import UPDATE_STAT_DTYPES, Engine  # noqa: E402
from oracle import nets, trainer  # noqa: E402
from tests import approx_oracle as ao  # noqa: E402
from tests import mixed_width  # noqa: E402
from tests.helpers import joint_rows, synthetic_trainer_case  # noqa: E402

L = 200
NETS4 = ("actor", "critic", "tgt_actor", "tgt_critic")
CTL_UPD_CTR_OFFSET = 2568  # Ctl.upd_ctr (mdp_topo.h; tests/test_gpu_parity.py)

CASES = {
    "spread_h64": dict(dims=[6, 5, 4]),
    "padded_h32": dict(dims=[6, 5, 4], H=32),
    "h128": dict(dims=[6, 5, 4], H=128),
    "h256": dict(dims=[6, 5, 4], H=256),
    "ddpg_mix": dict(dims=[6, 5, 4], local_q=[True, False, False]),
    "act_dims_3_5": dict(dims=[6, 4], widths=[3, 5]),
    "b8_ragged": dict(dims=[6, 5, 4], B=8),
    "b16": dict(dims=[6, 5, 4], B=16),
    "eight_agents": dict(dims=[4] * 8, B=16),
}


def _case(dims, seed, local_q=None, H=64, widths=None, B=40):
    if widths is None:
        c = synthetic_trainer_case(dims, B, L, seed, local_q, H)
        c["widths"] = [5] * len(dims)
    else:
        c = mixed_width.mixed_case(dims, widths, B, L, seed, local_q, H)
    c["approx"] = ao.approx_case(c, dims, seed, H)
    c["B"] = B
    return c


def _named(name, seed):
    kw = CASES[name]
    return _case(kw["dims"], seed, kw.get("local_q"), kw.get("H", 64), kw.get("widths"), kw.get("B", 40))


def _oracle_agents(c):
    ags = [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][j]) for j, p in enumerate(c["params"])]
    return ao.add_approx(ags, copy.deepcopy(c["approx"]))


def _engine(c, dims, H=64, approx=True, **kw):
    mixed = any(w != 5 for w in c["widths"])
    eng = Engine(dims, c["local_q"], num_units=H, batch_size=c["B"], capacity=L + 7, approx=approx,
                 act_dims=c["widths"] if mixed else None, **kw)
    rows = mixed_width.joint_rows_w(c["data"], dims) if mixed else joint_rows(c["data"], dims)
    eng.add_rows(torch.from_numpy(rows))
    for i, p in enumerate(c["params"]):
        for w in NETS4:
            eng.set_params(i, w, p[w])
    for i, j in eng.approx_pairs():
        eng.set_approx_params(i, j, "net", c["approx"][i][j]["net"])
        eng.set_approx_params(i, j, "tgt", c["approx"][i][j]["tgt"])
    return eng


def _named_engine(name, c, **kw):
    return _engine(c, CASES[name]["dims"], H=CASES[name].get("H", 64), **kw)


def _update(eng, c, i, idx=None, u_tgt=None, u_act=None):
    idx = c["idx"][i] if idx is None else idx
    u_tgt = c["u_tgt"][i] if u_tgt is None else u_tgt
    u_act = c["u_act"][i] if u_act is None else u_act
    eng.update(i, idx=torch.from_numpy(idx), u_tgt=torch.from_numpy(u_tgt), u_act=torch.from_numpy(u_act))


def _oracle_update(ags, c, i, idx=None, u_tgt=None, u_act=None, lam=ao.LAMBDA):
    idx = c["idx"][i] if idx is None else idx
    u_tgt = c["u_tgt"][i] if u_tgt is None else u_tgt
    u_act = c["u_act"][i] if u_act is None else u_act
    return ao.update(ags, i, c["data"], idx, u_tgt, u_act, c["widths"], lam)


def _maddpg_sets(eng):
    out = {(i, w): eng.get_params(i, w) for i in range(eng.n) for w in Engine.SETS}
    for i in range(eng.n):
        for net in (0, 1):
            out[(i, f"beta{net}")] = {"b": eng.get_beta_powers(i, net)}
    return out


def _approx_sets(eng):
    out = {(i, j, w): eng.get_approx_params(i, j, w) for i, j in eng.approx_pairs() for w in Engine.APPROX_SETS}
    for i, j in eng.approx_pairs():
        out[(i, j, "beta")] = {"b": eng.get_approx_beta_powers(i, j)}
    return out


def _same(a, b):
    return {k: all(np.array_equal(a[k][t], b[k][t]) for t in a[k]) for k in a}


def _upd_ctr(eng):
    ctl = eng.region("ctl", torch.uint8).cpu().numpy()
    return int(ctl[CTL_UPD_CTR_OFFSET:CTL_UPD_CTR_OFFSET + 4].view(np.uint32)[0])


def _close(dev, ref, tol, what):
    for k in ref:
        r = np.asarray(ref[k]).reshape(dev[k].shape)
        err = float(np.abs(dev[k] - r).max())
        assert err < tol, (what, k, err)


def _grad_close(dev, ref, what):
    for k in ref:
        r = np.asarray(ref[k], np.float64).reshape(dev[k].shape)
        scale = float(np.abs(r).max()) or 1.0
        assert float(np.abs(dev[k] - r).max()) / scale < 1e-5, (what, k)


def _rel(got, want):
    return abs(got - want) <= 1e-5 * abs(want) + 1e-7


def _check_pair(eng, ap, i, j):
    _close(eng.get_approx_params(i, j, "net"), ap.net, 2e-4, (i, j, "net"))
    _close(eng.get_approx_params(i, j, "tgt"), ap.tgt, 2e-4, (i, j, "tgt"))
    _close(eng.get_approx_params(i, j, "m"), ap.opt.m, 2e-4, (i, j, "m"))
    _close(eng.get_approx_params(i, j, "v"), ap.opt.v, 2e-4, (i, j, "v"))
    bp = eng.get_approx_beta_powers(i, j)
    assert bp[0] == ap.opt.b1p and bp[1] == ap.opt.b2p, (i, j, bp)


def _check_pads(eng, name):
    """a padded hidden width or a narrow action width: every pad entry of the
    approximator regions is an exact zero, and so is every span without an approximator"""
    for i in range(eng.n):
        if eng.local_q[i]:
            continue
        for reg_name in Engine.APPROX_REGIONS:
            reg = eng.approx_region(i, reg_name).cpu().numpy()
            covered = np.zeros(reg.shape, bool)
            for j in range(eng.n):
                if j == i:
                    continue
                for t, (off, r, cc, dr, dc) in enumerate(eng.net_tensors(j, 0)):
                    a = reg[off:off + dr * dc].reshape(dr, dc)
                    covered[off:off + dr * dc] = True
                    assert not a[:, cc:].any(), (name, reg_name, i, j, t)
                    if t:                                   # (W1's rows are the observation: not padded)
                        assert not a[r:, :].any(), (name, reg_name, i, j, t)
                    if reg_name in ("net", "grad") and t in (0, 2, 4):
                        assert a[:r, :cc].any(), (name, reg_name, i, j, t)
            assert not reg[~covered].any(), (name, reg_name, i)


@pytest.mark.parametrize("name", list(CASES))
def test_approx_grad_and_step_parity(name):
    """every pair: raw gradients after approx_grad, the pair's cross-entropy, entropy
    and loss, then net, target, m, v and beta powers after approx_step; the step leaves
    every MADDPG set and the noise counter bit-unchanged"""
    c = _named(name, seed=31)
    eng = _named_engine(name, c)
    ags = _oracle_agents(c)
    n = eng.n
    before, ctr = _maddpg_sets(eng), _upd_ctr(eng)
    for i in range(n):
        if c["local_q"][i]:
            continue
        idx = c["idx"][i]
        batch_n = [tuple(x[idx] for x in c["data"][j]) for j in range(n)]
        eng.approx_grad(i, torch.from_numpy(idx))
        want = {j: ao.approx_grads(ap.net, batch_n[j][0], batch_n[j][1]) for j, ap in ags[i].approx.items()}
        for j, (g, st) in want.items():
            _grad_close(eng.get_approx_params(i, j, "grad"), g, (i, j))
            info = eng.approx_info(i, j)
            if i == 0:
                print(f"{name} pair ({i}, {j}): device {info}, oracle {st}")
            for k in ("cross_entropy", "entropy", "loss"):
                assert _rel(info[k], st[k]), (i, j, k, info[k], st[k])
            assert info["updates"] == 0
        eng.approx_step(i, torch.from_numpy(idx))
        ao.approx_steps(ags, i, batch_n)
        for j, ap in ags[i].approx.items():
            _check_pair(eng, ap, i, j)
            _grad_close(eng.get_approx_params(i, j, "grad"), want[j][0], (i, j, "after the step"))
            assert eng.approx_info(i, j)["updates"] == 1
    assert all(_same(before, _maddpg_sets(eng)).values()) and _upd_ctr(eng) == ctr
    assert eng.check_finite() == 0
    if name in ("padded_h32", "act_dims_3_5"):
        _check_pads(eng, name)


@pytest.mark.parametrize("name", list(CASES))
def test_approx_update_parity(name):
    """one whole update per agent against the oracle: the six stats, the critic's and
    actor's raw gradients, every MADDPG set, and the agent's approximators"""
    c = _named(name, seed=32)
    eng = _named_engine(name, c)
    ags = _oracle_agents(c)
    for i in range(eng.n):
        _update(eng, c, i)
        got = eng.stats(i)
        want, ex = _oracle_update(ags, c, i)
        assert _rel(got[0], want[0]), (i, got[0], want[0])
        np.testing.assert_allclose(got[1:], want[1:], rtol=2e-5, atol=2e-6)
        _grad_close(eng.get_params(i, "g_critic"), ex["grad_critic"], (i, "critic"))
        _grad_close(eng.get_params(i, "g_actor"), ex["grad_actor"], (i, "actor"))
        ag = ags[i]
        for w, ref in (("actor", ag.actor), ("critic", ag.critic), ("tgt_actor", ag.tgt_actor),
                       ("tgt_critic", ag.tgt_critic), ("m_actor", ag.opt_actor.m), ("v_actor", ag.opt_actor.v),
                       ("m_critic", ag.opt_critic.m), ("v_critic", ag.opt_critic.v)):
            _close(eng.get_params(i, w), ref, 2e-4, (i, w))
        for net, opt in ((0, ag.opt_actor), (1, ag.opt_critic)):
            bp = eng.get_beta_powers(i, net)
            assert bp[0] == opt.b1p and bp[1] == opt.b2p, (i, net)
        for j, ap in ag.approx.items():
            _check_pair(eng, ap, i, j)
            _grad_close(eng.get_approx_params(i, j, "grad"), ex["approx"][j][0], (i, j))
            info = eng.approx_info(i, j)
            assert _rel(info["loss"], ex["approx"][j][1]["loss"]) and info["updates"] == 1
    assert _upd_ctr(eng) == eng.n and eng.check_finite() == 0


def test_approx_with_target_actor_bits_equals_maddpg_on_general_kernels(monkeypatch):
    """every target approximator := the bits of the target actor it stands for: each
    agent's first update equals a plain engine on the general kernels bit for bit in
    every MADDPG set, the beta powers and the six stats.  An engine whose target
    approximators differ does not (the pointer is read)."""
    dims = [6, 5, 4]
    c = _case(dims, seed=33)
    same = copy.deepcopy(c)
    for i in range(3):
        for j in same["approx"][i]:
            same["approx"][i][j]["tgt"] = copy.deepcopy(c["params"][j]["tgt_actor"])
    for i in range(3):          # each agent's FIRST update: fresh engines, so no earlier Polyak moved a target actor
        monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
        plain = _engine(c, dims, approx=False)
        monkeypatch.delenv("MDP_GENERAL_GRADS")
        eng, other = _engine(same, dims), _engine(c, dims)
        for e in (plain, eng, other):
            _update(e, c, i)
        assert plain.stats(i) == eng.stats(i), i
        assert plain.stats(i) != other.stats(i), i
        a, b, d = _maddpg_sets(plain), _maddpg_sets(eng), _maddpg_sets(other)
        assert all(_same(a, b).values()), (i, _same(a, b))
        assert not _same(a, d)[(i, "critic")], i
        ga, gb = plain.get_params(i, "g_critic"), eng.get_params(i, "g_critic")
        assert all(np.array_equal(ga[k], gb[k]) for k in ga)


@pytest.mark.parametrize("unfused", [False, True])
def test_approx_four_rounds(monkeypatch, unfused):
    """four consecutive rounds against the oracle, under test_td3_four_rounds_delay_two's
    tolerances.  unfused: every optimizer step as k_reduce + k_apply (MDP_UNFUSED_APPLY=1)"""
    if unfused:
        monkeypatch.setenv("MDP_UNFUSED_APPLY", "1")
    dims = [6, 5, 4]
    n, B = len(dims), 40
    c = _case(dims, seed=34)
    eng = _engine(c, dims)
    ags = _oracle_agents(c)
    rng = np.random.default_rng(73)
    for r in range(1, 5):
        idx = rng.integers(0, L, size=(n, B)).astype(np.int32)
        u_tgt = rng.uniform(1e-6, 1.0, size=(n, n, B, 5)).astype(np.float32)
        u_act = rng.uniform(1e-6, 1.0, size=(n, B, 5)).astype(np.float32)
        for i in range(n):
            _update(eng, c, i, idx[i], u_tgt[i], u_act[i])
            got = eng.stats(i)
            want, ex = _oracle_update(ags, c, i, idx[i], u_tgt[i], u_act[i])
            assert _rel(got[0], want[0]), (r, i, got[0], want[0])
            np.testing.assert_allclose(got[1:], want[1:], rtol=1e-4, atol=1e-5)
            for j in ags[i].approx:
                assert abs(eng.approx_info(i, j)["loss"] - ex["approx"][j][1]["loss"]) < 1e-4, (r, i, j)
    for i in range(n):
        ag = ags[i]
        for w, ref in (("actor", ag.actor), ("critic", ag.critic), ("tgt_actor", ag.tgt_actor),
                       ("tgt_critic", ag.tgt_critic)):
            _close(eng.get_params(i, w), ref, 1e-4, (i, w))
        for j, ap in ag.approx.items():
            _close(eng.get_approx_params(i, j, "net"), ap.net, 1e-4, (i, j, "net"))
            _close(eng.get_approx_params(i, j, "tgt"), ap.tgt, 1e-4, (i, j, "tgt"))
            bp = eng.get_approx_beta_powers(i, j)
            assert bp[0] == ap.opt.b1p and bp[1] == ap.opt.b2p
            assert eng.approx_info(i, j)["updates"] == 4
    assert _upd_ctr(eng) == 4 * n and eng.check_finite() == 0


def test_approx_update_round_graphs_equal_eager():
    dims = [6, 5, 4]
    c = _case(dims, seed=35)
    engs = []
    for graphs in (True, False):
        e = _engine(c, dims, seed=5)
        e.seed_py_random(77)
        e.set_graphs(graphs)
        engs.append(e)
    for r in range(5):
        for e in engs:
            e.update_round()
    for e in engs:
        e.synchronize()
    assert all(_same(_maddpg_sets(engs[0]), _maddpg_sets(engs[1])).values())
    sa, sb = _approx_sets(engs[0]), _approx_sets(engs[1])
    assert all(_same(sa, sb).values()), _same(sa, sb)
    for i in range(3):
        assert engs[0].stats(i) == engs[1].stats(i)
        for j in range(3):
            if j != i:
                ia = engs[0].approx_info(i, j)
                assert ia == engs[1].approx_info(i, j) and ia["updates"] == 5
    assert np.array_equal(engs[0].get_rng_state(), engs[1].get_rng_state())
    start = c["approx"][0][1]["net"]
    assert not np.array_equal(engs[0].get_approx_params(0, 1, "net")["W1"], start["W1"])   # they did train


def _scn_engine(graphs, approx=True):
    from maddpg_amd.envs import spec
    sp = spec("simple_spread")
    eng = Engine(sp.obs_dims, batch_size=32, capacity=4096, num_envs=16, scenario="simple_spread", seed=9,
                 approx=approx)
    eng.init_params(3)
    eng.seed_py_random(4)
    eng.env_reset()
    eng.set_graphs(graphs)
    return eng


def test_approx_train_step_graphs_equal_eager():
    """simple_spread N = 3, 16 env copies, B = 32: three train_step(2) calls and a
    train_steps group are bit-equal with graphs on and off, approximators included"""
    engs = [_scn_engine(g) for g in (True, False)]
    for e in engs:
        for _ in range(3):
            e.train_step(2)
        e.train_steps([1, 2, 0, 1])
        e.synchronize()
    assert all(_same(_maddpg_sets(engs[0]), _maddpg_sets(engs[1])).values())
    sa, sb = _approx_sets(engs[0]), _approx_sets(engs[1])
    assert all(_same(sa, sb).values()), _same(sa, sb)
    assert engs[0].approx_info(0, 1) == engs[1].approx_info(0, 1) and engs[0].approx_info(0, 1)["updates"] == 10
    assert torch.equal(engs[0].region("replay"), engs[1].region("replay"))
    assert np.array_equal(engs[0].get_rng_state(), engs[1].get_rng_state())
    assert engs[0].check_finite() == 0


def test_init_params_keeps_a_seeds_nets_and_copies_the_targets():
    dims = [6, 5, 4]
    plain = Engine(dims, batch_size=16, capacity=64)
    eng = Engine(dims, batch_size=16, capacity=64, approx=True)
    plain.init_params(7)
    eng.init_params(7)
    for i in range(3):
        for w in NETS4:
            a, b = plain.get_params(i, w), eng.get_params(i, w)
            assert all(np.array_equal(a[k], b[k]) for k in a), (i, w)
    for i, j in eng.approx_pairs():
        net, tgt = eng.get_approx_params(i, j, "net"), eng.get_approx_params(i, j, "tgt")
        assert all(np.array_equal(net[k], tgt[k]) for k in net) and net["W1"].any()
        assert not np.array_equal(net["W1"], eng.get_params(j, "actor")["W1"])


def test_frozen_policy_fit_on_the_device():
    """the CPU test's inputs: 100 approx_step calls of observer 0, the same one-quarter bar"""
    fc = ao.fit_case()
    want = ao.fit_run(fc)
    eng = Engine(ao.FIT_DIMS, num_units=ao.FIT_H, batch_size=ao.FIT_B, capacity=ao.FIT_L, approx=True)
    eng.add_rows(torch.from_numpy(joint_rows(fc["data"], ao.FIT_DIMS)))
    for j, p in enumerate(fc["actors"]):
        eng.set_params(j, "actor", p)
    for j, phi in fc["phi"].items():
        eng.set_approx_params(0, j, "net", phi)
        eng.set_approx_params(0, j, "tgt", phi)
    obs = {j: torch.from_numpy(fc["data"][j][0]) for j in fc["phi"]}
    kl0 = {j: eng.approx_kl(0, j, obs[j]) for j in fc["phi"]}
    idx = torch.from_numpy(fc["idx"]).to(eng.device)
    for s in range(ao.FIT_STEPS):
        eng.approx_step(0, idx[s])
    for j in fc["phi"]:
        kl1 = eng.approx_kl(0, j, obs[j])
        print(f"approximator of agent {j}: device KL {kl0[j]:.4f} -> {kl1:.4f}; "
              f"oracle {want[j][0]:.4f} -> {want[j][1]:.4f}")
        assert abs(kl0[j] - want[j][0]) < 1e-4
        assert kl1 < 0.25 * kl0[j], (j, kl0[j], kl1)
    assert eng.approx_info(0, 1)["updates"] == ao.FIT_STEPS


def test_approx_refusals_leave_the_handle_training():
    dims = [6, 5, 4]
    c = _case(dims, seed=36, local_q=[False, False, True])
    eng = _engine(c, dims)
    twin = _engine(c, dims)
    idx = torch.from_numpy(c["idx"][0]).to(eng.device)
    nb = eng.lib.mdp_approx_bytes(eng.cfg)
    buf = torch.empty(max(nb, eng.lib.mdp_td3_bytes(eng.cfg), eng.lib.mdp_per_bytes(eng.cfg)), dtype=torch.uint8,
                      device=eng.device)
    eps = np.zeros((3, 3), np.float32)
    flat = eng._flat_params(1, "actor", c["approx"][0][1]["net"])
    f2 = np.ones(2, np.float32)

    def refused(fn, *a, match):
        with pytest.raises(_lib.MdpError, match=match):
            fn(*a)

    refused(eng._c, "mdp_approx_enable", eng._ptr(buf), buf.numel(), 1e-3, match="mdp_approx_enable: already enabled")
    refused(eng._c, "mdp_per_enable", eng._ptr(buf), buf.numel(), 0.6, 0.4, 0.001, 0.01, 1.0, match="inferred policies")
    refused(eng._c, "mdp_td3_enable", eng._ptr(buf), buf.numel(), 2, match="inferred policies")
    refused(eng._c, "mdp_minimax_enable", _lib.fptr(eps), match="inferred policies")
    refused(eng.set_update_mode, "throughput", match="mdp_set_update_mode")
    refused(eng.update_all, match="mdp_update_all")
    refused(eng.dp_init, 2, 0, b"\0" * 128, match="mdp_dp_init")
    refused(eng.dp_xgmi_open, 2, 0, match="mdp_dp_xgmi_open")
    refused(eng.critic_grad, 0, idx, match="mdp_critic_grad")
    refused(eng.actor_grad, 0, idx, match="mdp_actor_grad")
    refused(eng.reduce_grad, 0, 1, match="mdp_reduce_grad")
    refused(eng.apply_grad, 0, 1, match="mdp_apply_grad")
    # observer == agent, an observer with a DDPG critic, indices out of range: every pair entry point
    for obs_i, ag_j, why in ((0, 0, "observer itself"), (2, 0, "DDPG"), (3, 0, "observer out of range"),
                             (-1, 0, "observer out of range"), (0, 3, "agent out of range"),
                             (0, -1, "agent out of range")):
        refused(eng._c, "mdp_approx_set_params", obs_i, ag_j, 0, _lib.fptr(flat), flat.size,
                match=f"mdp_approx_set_params: .*{why}")
        refused(eng._c, "mdp_approx_get_params", obs_i, ag_j, 0, _lib.fptr(flat), flat.size,
                match=f"mdp_approx_get_params: .*{why}")
        refused(eng.get_approx_beta_powers, obs_i, ag_j, match=f"mdp_approx_get_beta_powers: .*{why}")
        refused(eng.set_approx_beta_powers, obs_i, ag_j, f2, match=f"mdp_approx_set_beta_powers: .*{why}")
        refused(eng.approx_info, obs_i, ag_j, match=f"mdp_approx_info: .*{why}")
        refused(eng._c, "mdp_approx_logits", obs_i, ag_j, 0, eng._ptr(idx), eng._ptr(idx), 1,
                match=f"mdp_approx_logits: .*{why}")
    for obs_i, why in ((2, "DDPG"), (3, "observer out of range")):
        refused(eng.approx_grad, obs_i, idx, match=f"mdp_approx_grad: .*{why}")
        refused(eng.approx_step, obs_i, idx, match=f"mdp_approx_step: .*{why}")
    refused(eng._c, "mdp_approx_set_params", 0, 1, 5, _lib.fptr(flat), flat.size, match="which")
    refused(eng._c, "mdp_approx_set_params", 0, 1, 0, _lib.fptr(flat), flat.size - 1, match="parameter count")
    host = np.zeros(c["B"], np.int32)
    refused(eng._c, "mdp_approx_step", 0, host.ctypes.data, match="mdp_approx_step: idx_dev")
    refused(eng._c, "mdp_approx_grad", 0, None, match="mdp_approx_grad: idx_dev")
    with pytest.raises(ValueError, match="tf1"):
        eng.save_state("unused", fmt="tf1")
    # after all of that the handle trains, and equals a twin that was never refused anything
    for i in range(3):
        _update(eng, c, i)
        _update(twin, c, i)
    assert all(_same(_maddpg_sets(eng), _maddpg_sets(twin)).values())
    assert all(_same(_approx_sets(eng), _approx_sets(twin)).values())
    assert eng.check_finite() == 0

    # a handle without the option: every new entry point is refused; enable's own argument checks
    plain = _engine(c, dims, approx=False)
    refused(plain._c, "mdp_approx_set_params", 0, 1, 0, _lib.fptr(flat), flat.size, match="not enabled")
    refused(plain._c, "mdp_approx_get_params", 0, 1, 0, _lib.fptr(flat), flat.size, match="not enabled")
    refused(plain._c, "mdp_approx_get_beta_powers", 0, 1, _lib.fptr(f2), match="not enabled")
    refused(plain._c, "mdp_approx_set_beta_powers", 0, 1, _lib.fptr(f2), match="not enabled")
    refused(plain.approx_info, 0, 1, match="not enabled")
    refused(plain._c, "mdp_approx_logits", 0, 1, 0, plain._ptr(idx), plain._ptr(idx), 1, match="not enabled")
    refused(plain._c, "mdp_approx_grad", 0, plain._ptr(idx), match="not enabled")
    refused(plain._c, "mdp_approx_step", 0, plain._ptr(idx), match="not enabled")
    for lam in (-1e-3, float("nan"), float("inf")):
        refused(plain._c, "mdp_approx_enable", plain._ptr(buf), buf.numel(), lam, match="lambda")
    refused(plain._c, "mdp_approx_enable", None, buf.numel(), 1e-3, match="buf_dev")
    hostbuf = np.zeros(nb, np.uint8)
    refused(plain._c, "mdp_approx_enable", hostbuf.ctypes.data, nb, 1e-3, match="buf_dev")
    refused(plain._c, "mdp_approx_enable", plain._ptr(buf), nb - 1, 1e-3, match="bytes")
    _update(plain, c, 0)                                # a refused enable leaves a MADDPG handle
    refused(plain._c, "mdp_approx_enable", plain._ptr(buf), buf.numel(), 1e-3, match="before the handle's first update")
    _update(plain, c, 1)
    assert plain.check_finite() == 0

    # either order: after prioritized replay, MATD3, M3DDPG, throughput mode; lambda = 0 is accepted
    B = c["B"]
    for kw in (dict(prioritized=True), dict(td3=True), dict(minimax=True), dict(approx_lambda=-1.0)):
        with pytest.raises(_lib.MdpError):
            Engine(dims, batch_size=B, capacity=L + 7, approx=True, **kw)
    with pytest.raises((ValueError, _lib.MdpError)):
        Engine(dims, batch_size=B, capacity=L + 7, approx=True, world_size=2)
    for kw, why in ((dict(prioritized=True), "prioritized replay"), (dict(td3=True), "MATD3"),
                    (dict(minimax=True), "M3DDPG")):
        e = Engine(dims, batch_size=B, capacity=L + 7, **kw)
        refused(e._c, "mdp_approx_enable", e._ptr(buf), buf.numel(), 1e-3, match=why)
    tp = Engine(dims, batch_size=B, capacity=L + 7)
    tp.set_update_mode("throughput")
    refused(tp._c, "mdp_approx_enable", tp._ptr(buf), buf.numel(), 1e-3, match="strict update mode")
    # a handle configured for data parallelism reaches mdp_approx_enable itself (the
    # Engine argument check above never does); the xGMI enable names the option too
    dp = Engine(dims, batch_size=B, capacity=L + 7, world_size=2)
    refused(dp._c, "mdp_approx_enable", dp._ptr(buf), buf.numel(), 1e-3, match="mdp_approx_enable: .*data-parallel")
    refused(eng._c, "mdp_dp_xgmi_enable", match="mdp_dp_xgmi_enable: inferred policies")
    zero = _engine(c, dims, approx_lambda=0.0)
    _update(zero, c, 0)
    assert _rel(zero.approx_info(0, 1)["loss"], zero.approx_info(0, 1)["cross_entropy"])


def test_approx_enable_is_refused_after_a_round_and_after_a_train_step():
    """mdp_update_round and mdp_train_step count as the handle's first training call
    just as mdp_update does (test_approx_refusals_leave_the_handle_training); the
    refused handle goes on as MADDPG and equals a twin that never asked"""
    dims = [6, 5, 4]
    c = _case(dims, seed=40)
    by_round = [_engine(c, dims, approx=False) for _ in range(2)]
    by_step = [_scn_engine(True, approx=False) for _ in range(2)]
    for (asked, twin), go in ((by_round, lambda e: e.update_round()), (by_step, lambda e: e.train_step(1))):
        go(asked)
        go(twin)
        nb = asked.lib.mdp_approx_bytes(asked.cfg)
        buf = torch.empty(nb, dtype=torch.uint8, device=asked.device)
        with pytest.raises(_lib.MdpError, match="mdp_approx_enable: .*before the handle's first update, round or train"):
            asked._c("mdp_approx_enable", asked._ptr(buf), nb, 1e-3)
        with pytest.raises(_lib.MdpError, match="not enabled"):
            asked.approx_info(0, 1)
        go(asked)
        go(twin)
        asked.synchronize()
        twin.synchronize()
        assert all(_same(_maddpg_sets(asked), _maddpg_sets(twin)).values())
        assert asked.check_finite() == 0


def test_approx_enable_refuses_a_short_allocation():
    """a buffer that ends before mdp_approx_bytes, at the very end of a hipMalloc
    allocation.  Run where the runtime reports an allocation's exact extent (the
    library checks with the same hipMemGetAddressRange)."""
    import ctypes
    dims = [6, 5, 4]
    plain = Engine(dims, batch_size=40, capacity=L + 7)
    nb = plain.lib.mdp_approx_bytes(plain.cfg)
    nbytes, base = 8 << 20, ctypes.c_void_p()
    assert 256 < nb < nbytes
    assert plain.lib.hipMalloc(ctypes.byref(base), ctypes.c_size_t(nbytes)) == 0
    try:
        rb, ext = ctypes.c_void_p(), ctypes.c_size_t()
        exact = (plain.lib.hipMemGetAddressRange(ctypes.byref(rb), ctypes.byref(ext), base) == 0
                 and rb.value == base.value and ext.value == nbytes)
        if not exact:
            pytest.skip(f"runtime reports extent {ext.value} for a {nbytes}-byte allocation")
        short = ctypes.c_void_p(base.value + nbytes - (nb - 256))
        with pytest.raises(_lib.MdpError, match="mdp_approx_enable: buf_dev .*allocation too small"):
            plain._c("mdp_approx_enable", short, nb, 1e-3)
    finally:
        torch.cuda.synchronize()
        assert plain.lib.hipFree(base) == 0
    c = _case(dims, seed=39)
    for i, p in enumerate(c["params"]):
        for w in NETS4:
            plain.set_params(i, w, p[w])
    plain.add_rows(torch.from_numpy(joint_rows(c["data"], dims)))
    _update(plain, c, 0)
    assert plain.check_finite() == 0


def test_approx_checkpoint_round_trip(tmp_path):
    dims = [6, 5, 4]
    c = _case(dims, seed=37)
    eng = _engine(c, dims)
    for r in range(2):
        for i in range(3):
            _update(eng, c, i)
    sd = eng.state_dict()
    for i, j in eng.approx_pairs():
        for w in Engine.APPROX_SETS:
            assert f"agent_{i}/approx_{j}/{w}/W1" in sd
        assert f"agent_{i}/approx_{j}/beta_power" in sd
    path = eng.save_state(str(tmp_path / "ck"))
    with pytest.raises(ValueError, match="tf1"):
        eng.save_state(str(tmp_path / "ck_tf1"), fmt="tf1")
    c2 = _case(dims, seed=38)               # other weights everywhere, the same replay rows
    c2["data"] = c["data"]
    other = _engine(c2, dims)
    assert not any(_same(_approx_sets(eng), _approx_sets(other))[(0, 1, w)] for w in Engine.APPROX_SETS)
    other.load_state(path)
    assert all(_same(_maddpg_sets(eng), _maddpg_sets(other)).values())
    assert all(_same(_approx_sets(eng), _approx_sets(other)).values())
    # a MADDPG checkpoint leaves the approximators alone; a MADDPG engine ignores their keys
    keep = _approx_sets(other)
    other.load_state_dict({k: v for k, v in sd.items() if "/approx_" not in k})
    assert all(_same(keep, _approx_sets(other)).values())
    plain = _engine(c, dims, approx=False)
    plain.load_state_dict(sd)
    assert all(np.array_equal(plain.get_params(1, "critic")[k], eng.get_params(1, "critic")[k]) for k in nets.NAMES)
    # the restored engine goes on exactly as the saved one
    _update(eng, c, 0)
    _update(other, c, 0)
    assert all(_same(_approx_sets(eng), _approx_sets(other)).values()) and eng.stats(0) == other.stats(0)
    q = eng.approx_quality(torch.from_numpy(c["idx"][0]))
    assert len(q["pairs"]) == 6 and np.isfinite(q["mean_ce"]) and q["mean_kl"] >= 0


def test_approx_trainer_facade_update_returns_the_reference_list():
    """MADDPGAgentTrainer with args.approx_policies: update() past the gates returns the
    reference's list with its dtypes, and the approximators have stepped"""
    import argparse
    import random

    from maddpg_amd.common import tf_util as U
    from maddpg_amd.envs import Discrete
    from maddpg_amd.trainer.maddpg import MADDPGAgentTrainer
    args = argparse.Namespace(lr=1e-2, gamma=0.95, batch_size=16, num_units=64, max_episode_len=2,
                              approx_policies=True, approx_lambda=1e-3)
    rng = np.random.default_rng(0)
    with U.single_threaded_session():
        trainers = [MADDPGAgentTrainer(f"agent_{i}", None, [(6,)] * 2, [Discrete(5)] * 2, i, args) for i in range(2)]
        U.initialize()
        eng = U.get_session().engine()
        assert eng.approx and eng.approx_lambda == 1e-3
        random.seed(3)
        losses = []
        for t in range(1, 201):
            for ag in trainers:
                a = rng.dirichlet(np.ones(5)).astype(np.float32)
                ag.experience(rng.normal(size=6), a, float(rng.normal()), rng.normal(size=6), False, False)
            for ag in trainers:
                ag.preupdate()
            for ag in trainers:
                loss = ag.update(trainers, t)
                if loss is not None:
                    losses.append((ag.agent_index, loss))
        assert [i for i, _ in losses] == [0, 1, 0, 1]                       # t = 100, 200
        for _, loss in losses:
            assert type(loss) is list and [type(x) for x in loss] == list(UPDATE_STAT_DTYPES)
            assert all(np.isfinite(loss))
        assert eng.approx_info(0, 1)["updates"] == 2 and eng.approx_info(1, 0)["updates"] == 2
