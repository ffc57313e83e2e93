"""GPU tests of MATD3 (mdp_td3_enable) against tests/td3_oracle.py.

Trainer-only handles on injected indices and uniforms: B = 40 (two full 16-row
tiles and a ragged one), ring L = 200.  The parity fixtures add the batch median
of q1' - q2' to the second target critic's b3, so about half of every agent's
rows take each branch of the min in the first update (asserted from the oracle).
Tolerances are those of tests/test_gpu_parity.py.
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
from tests import mixed_width, td3_oracle  # noqa: E402
from tests.helpers import joint_rows, synthetic_trainer_case  # noqa: E402

B, L = 40, 200
NETS4 = ("actor", "critic", "tgt_actor", "tgt_critic")
TWIN_SETS = ("critic2", "tgt_critic2", "m_critic2", "v_critic2")


def _case(dims, seed, local_q=None, H=64, widths=None):
    if widths is None:
        c = synthetic_trainer_case(dims, B, L, seed, local_q, H)
        c["widths"] = [5] * len(dims)
    else:
        c = mixed_width.mixed_case(dims, widths, B, L, seed, local_q, H)
    c["twins"] = td3_oracle.twin_case(c, dims, seed, H)
    return c


def _oracle_agents(c):
    ags = [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][j]) for j, p in enumerate(c["params"])]
    for j, ag in enumerate(ags):
        td3_oracle.add_twin(ag, copy.deepcopy(c["twins"][j]["critic2"]), copy.deepcopy(c["twins"][j]["tgt_critic2"]))
    return ags


def _balance(c):
    td3_oracle.balanced_twin_targets(_oracle_agents(c), c["twins"], c["data"], c["idx"],
                                     [mixed_width.narrow(u, c["widths"]) for u in c["u_tgt"]])


def _engine(c, dims, H=64, d=2, td3=True, **kw):
    mixed = any(w != 5 for w in c["widths"])
    eng = Engine(dims, c["local_q"], num_units=H, batch_size=B, capacity=L + 7, td3=td3, policy_delay=d,
                 act_dims=c["widths"] if mixed else None, **kw)
    rows = mixed_width.joint_rows_w(c["data"], dims) if mixed else joint_rows(c["data"], dims)
    eng.add_rows(torch.from_numpy(rows))
    for i, p in enumerate(c["params"]):
        for w in NETS4:
            eng.set_params(i, w, p[w])
        if td3:
            eng.set_params(i, "critic2", c["twins"][i]["critic2"])
            eng.set_params(i, "tgt_critic2", c["twins"][i]["tgt_critic2"])
    return eng


def _update(eng, c, i, idx=None, u_tgt=None, u_act=None):
    idx = c["idx"][i] if idx is None else idx
    u_tgt = c["u_tgt"][i] if u_tgt is None else u_tgt
    u_act = c["u_act"][i] if u_act is None else u_act
    eng.update(i, idx=torch.from_numpy(idx), u_tgt=torch.from_numpy(u_tgt), u_act=torch.from_numpy(u_act))


def _oracle_update(ags, c, i, d, idx=None, u_tgt=None, u_act=None):
    idx = c["idx"][i] if idx is None else idx
    u_tgt = c["u_tgt"][i] if u_tgt is None else u_tgt
    u_act = c["u_act"][i] if u_act is None else u_act
    return td3_oracle.update(ags, i, c["data"], idx, mixed_width.narrow(u_tgt, c["widths"]), u_act, d=d,
                             actor_grads=mixed_width.actor_grads)


def _oracle_sets(ag):
    return {"actor": ag.actor, "critic": ag.critic, "tgt_actor": ag.tgt_actor, "tgt_critic": ag.tgt_critic,
            "m_actor": ag.opt_actor.m, "v_actor": ag.opt_actor.v, "m_critic": ag.opt_critic.m,
            "v_critic": ag.opt_critic.v, "critic2": ag.critic2, "tgt_critic2": ag.tgt_critic2,
            "m_critic2": ag.opt_critic2.m, "v_critic2": ag.opt_critic2.v}


def _all_sets(eng, i):
    out = {w: eng.get_params(i, w) for w in Engine.SETS + Engine.TD3_SETS}
    out["beta"] = {f"net{k}": eng.get_beta_powers(i, k) for k in (0, 1, 2)}
    return out


def _equal_sets(a, b):
    return {w: all(np.array_equal(a[w][k], b[w][k]) for k in a[w]) for w in a}


CASES = {
    "spread_h64": dict(dims=[6, 5, 4]),
    "padded_h32": dict(dims=[6, 5, 4], H=32),
    "h128": dict(dims=[6, 5, 4], H=128),
    "ddpg_mix": dict(dims=[6, 5, 4], local_q=[True, False, False]),
    "act_dims_3_5": dict(dims=[6, 4], widths=[3, 5]),
}


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_td3_update_parity(name, d):
    """one update per agent (k = 1: with d = 1 an actor step + Polyak of all three
    targets, with d = 2 a critic-only update) against the oracle"""
    kw = CASES[name]
    dims, H = kw["dims"], kw.get("H", 64)
    c = _case(dims, seed=11, local_q=kw.get("local_q"), H=H, widths=kw.get("widths"))
    _balance(c)
    eng = _engine(c, dims, H=H, d=d)
    ags = _oracle_agents(c)
    for i in range(len(dims)):
        before = _all_sets(eng, i)
        _update(eng, c, i)
        got = eng.stats(i)
        info = eng.td3_info(i)
        want, ex = _oracle_update(ags, c, i, d)
        share = float(ex["take_q1"].mean())
        print(f"{name} d={d} agent {i}: share of rows taking q1' = {share:.2f}; stats {got}")
        assert 0.4 <= share <= 0.6, (i, share)                       # both branches of the min, from the oracle alone
        assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]) + 1e-7, (got[0], want[0])
        np.testing.assert_allclose(got[1:], want[1:], rtol=2e-5, atol=2e-6)
        assert abs(info["q_loss2"] - ex["q_loss2"]) <= 1e-5 * abs(ex["q_loss2"]) + 1e-7, (info, ex["q_loss2"])
        assert info["q_loss"] == np.float32(got[0])
        assert (info["critic_updates"], info["actor_updates"]) == (1, 1 if d == 1 else 0)
        for w, ref in (("g_critic", ex["grad_critic"]), ("g_critic2", ex["grad_critic2"])):
            dg = eng.get_params(i, w)
            for k in ref:
                r = np.asarray(ref[k], np.float64).reshape(dg[k].shape)
                scale = float(np.abs(r).max()) or 1.0
                assert float(np.abs(dg[k] - r).max()) / scale < 1e-5, (i, w, k)
        after = _all_sets(eng, i)
        for w, ref in _oracle_sets(ags[i]).items():
            for k in ref:
                err = float(np.abs(after[w][k] - np.asarray(ref[k]).reshape(after[w][k].shape)).max())
                assert err < 2e-4, (i, w, k, err)
        for net, opt in ((0, ags[i].opt_actor), (1, ags[i].opt_critic), (2, ags[i].opt_critic2)):
            bp = eng.get_beta_powers(i, net)
            assert bp[0] == opt.b1p and bp[1] == opt.b2p, (i, net)
        if d == 2:      # critic-only: the actor, its optimizer and all three targets bit-unchanged
            same = _equal_sets(before, after)
            for w in ("actor", "m_actor", "v_actor", "tgt_actor", "tgt_critic", "tgt_critic2"):
                assert same[w], (i, w)
            assert np.array_equal(before["beta"]["net0"], after["beta"]["net0"])
    if H != eng.net_tensors(0, 1)[0][4]:
        # a padded width: the second critic's pad entries (hidden units >= num_units) are exact zeros
        for reg_name in Engine.TD3_REGIONS:
            reg = eng.td3_region(reg_name).cpu().numpy()
            for i in range(len(dims)):
                for t, (off, r, cc, dr, dc) in enumerate(eng.net_tensors(i, 1)):
                    a = reg[off:off + dr * dc].reshape(dr, dc)
                    assert not a[:, cc:].any(), (reg_name, i, t)
                    if t:                                   # (W1's rows are the critic input: not padded here)
                        assert not a[r:, :].any(), (reg_name, i, t)
                    if reg_name == "theta2" and t in (0, 2, 4):
                        assert a[:r, :cc].any()


def test_td3_degenerate_equals_maddpg_on_general_kernels(monkeypatch):
    """d = 1, critic2 := critic, tgt_critic2 := tgt_critic: min(q, q) = q, so the
    actor, critic 1, both of today's targets, their Adam slots, beta powers and
    the six stats equal a plain engine on the general kernels bit for bit"""
    dims = [6, 5, 4]
    c = _case(dims, seed=12)
    c["twins"] = [dict(critic2=p["critic"], tgt_critic2=p["tgt_critic"]) for p in c["params"]]
    monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
    plain = _engine(c, dims, td3=False)
    monkeypatch.delenv("MDP_GENERAL_GRADS")
    eng = _engine(c, dims, d=1)
    for i in range(len(dims)):
        _update(plain, c, i)
        _update(eng, c, i)
        assert plain.stats(i) == eng.stats(i), i
        for w in Engine.SETS:
            a, b = plain.get_params(i, w), eng.get_params(i, w)
            for k in a:
                assert np.array_equal(a[k], b[k]), (i, w, k)
        for net in (0, 1):
            assert np.array_equal(plain.get_beta_powers(i, net), eng.get_beta_powers(i, net))
        g1, g2 = eng.get_params(i, "g_critic"), eng.get_params(i, "g_critic2")
        for k in g1:   # critic 2 need not round like critic 1: the gradient tolerance
            scale = float(np.abs(g1[k]).max()) or 1.0
            assert float(np.abs(g1[k] - g2[k]).max()) / scale < 1e-5, (i, k)
        c1, c2 = eng.get_params(i, "critic"), eng.get_params(i, "critic2")
        for k in c1:
            assert float(np.abs(c1[k] - c2[k]).max()) < 2e-4, (i, k)


@pytest.mark.parametrize("unfused", [False, True])
def test_td3_four_rounds_delay_two(monkeypatch, unfused):
    """four consecutive rounds at d = 2 against the oracle; updates 1 and 3 leave the
    actor, its Adam slots and beta powers and all three targets bit-unchanged.
    unfused: every optimizer step as k_reduce + k_apply (MDP_UNFUSED_APPLY=1)"""
    if unfused:
        monkeypatch.setenv("MDP_UNFUSED_APPLY", "1")
    dims, d = [6, 5, 4], 2
    n = len(dims)
    c = _case(dims, seed=13)
    _balance(c)
    eng = _engine(c, dims, d=d)
    ags = _oracle_agents(c)
    rng = np.random.default_rng(72)
    frozen = ("actor", "m_actor", "v_actor", "tgt_actor", "tgt_critic", "tgt_critic2")
    for r in range(1, 5):
        if r == 1:      # the fixture's own rows and noise: the balanced min
            idx, u_tgt, u_act = c["idx"], c["u_tgt"], c["u_act"]
        else:
            idx = rng.integers(0, L, size=(n, B)).astype(np.int32)
            u_tgt = rng.uniform(1e-6, 1.0, size=(n, n, B, 5)).astype(np.float32)
            u_act = rng.uniform(1e-6, 1.0, size=(n, B, 5)).astype(np.float32)
        for i in range(n):
            before = _all_sets(eng, i)
            _update(eng, c, i, idx[i], u_tgt[i], u_act[i])
            got = eng.stats(i)
            want, ex = _oracle_update(ags, c, i, d, idx[i], u_tgt[i], u_act[i])
            share = float(ex["take_q1"].mean())
            print(f"round {r} agent {i}: share of rows taking q1' = {share:.2f}")
            assert r > 1 or 0.4 <= share <= 0.6, (i, share)
            assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]) + 1e-7, (r, i, got[0], want[0])
            np.testing.assert_allclose(got[1:], want[1:], rtol=1e-4, atol=1e-5)
            same = _equal_sets(before, _all_sets(eng, i))
            b0 = np.array_equal(before["beta"]["net0"], eng.get_beta_powers(i, 0))
            if r % 2:
                assert all(same[w] for w in frozen) and b0, (r, i, same)
            else:
                assert not any(same[w] for w in frozen) and not b0, (r, i, same)
            assert not same["critic"] and not same["critic2"]
    for i in range(n):
        info = eng.td3_info(i)
        assert (info["critic_updates"], info["actor_updates"]) == (4, 2)
        dev = _all_sets(eng, i)
        for w, ref in _oracle_sets(ags[i]).items():
            for k in ref:
                err = float(np.abs(dev[w][k] - np.asarray(ref[k]).reshape(dev[w][k].shape)).max())
                assert err < 1e-4, (i, w, k, err)
        for net, opt in ((0, ags[i].opt_actor), (1, ags[i].opt_critic), (2, ags[i].opt_critic2)):
            bp = eng.get_beta_powers(i, net)
            assert bp[0] == opt.b1p and bp[1] == opt.b2p


@pytest.mark.parametrize("unfused", [False, True])
def test_td3_critic_only_update_advances_the_noise_counter(monkeypatch, unfused):
    """device noise, d = 2: agent 0's updates 1 (critic-only) and 2 on the same rows
    draw the target actions at counters 0 and 1 -- the oracle on the pinned Philox
    uniforms of each counter reproduces both, and the two mean Q' differ (the
    targets did not move in between, only the noise)"""
    from oracle import philox
    if unfused:     # the counter then advances in critic 2's k_reduce
        monkeypatch.setenv("MDP_UNFUSED_APPLY", "1")
    dims, key = [6, 5, 4], 0xC0FFEE0123456789
    n = len(dims)
    c = _case(dims, seed=14)
    eng = _engine(c, dims, d=2, seed=key)
    ags = _oracle_agents(c)
    rows = np.arange(B)
    qn = []
    for ctr in (0, 1):
        eng.update(0, idx=torch.from_numpy(c["idx"][0]))
        got = eng.stats(0)
        u_tgt = np.stack([philox.uniforms5(key, (0 << 8) | (j + 1), ctr, rows) for j in range(n)])
        u_act = philox.uniforms5(key, (0 << 8) | 0x80, ctr, rows)
        want, _ = _oracle_update(ags, c, 0, 2, u_tgt=u_tgt, u_act=u_act)
        assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]) + 1e-7, (ctr, got[0], want[0])
        np.testing.assert_allclose(got[1:], want[1:], rtol=2e-5, atol=2e-6)
        qn.append(got[4])
    assert qn[0] != qn[1]


def _round_engine(c, dims, d, graphs):
    eng = _engine(c, dims, d=d, seed=5)
    eng.seed_py_random(77)
    eng.set_graphs(graphs)
    return eng


@pytest.mark.parametrize("d", [2, 3])
def test_td3_update_round_graphs_equal_eager(d):
    dims = [6, 5, 4]
    c = _case(dims, seed=15)
    engs = [_round_engine(c, dims, d, g) for g in (True, False)]
    for r in range(6):
        for e in engs:
            e.update_round()
    for e in engs:
        e.synchronize()
    for i in range(len(dims)):
        a, b = _all_sets(engs[0], i), _all_sets(engs[1], i)
        assert all(_equal_sets({w: a[w] for w in a}, {w: b[w] for w in b}).values()), i
        assert engs[0].stats(i) == engs[1].stats(i)
        ia, ib = engs[0].td3_info(i), engs[1].td3_info(i)
        assert ia == ib and (ia["critic_updates"], ia["actor_updates"]) == (6, 6 // d)
    assert np.array_equal(engs[0].get_rng_state(), engs[1].get_rng_state())


def _scn_engine(graphs, d=2):
    from maddpg_amd.envs import spec
    sp = spec("simple_spread")
    eng = Engine(sp.obs_dims, batch_size=32, capacity=4096, num_envs=16, scenario="simple_spread", seed=9,
                 td3=True, policy_delay=d)
    eng.init_params(3)
    eng.seed_py_random(4)
    eng.env_reset()
    eng.set_graphs(graphs)
    return eng


def test_td3_train_step_graphs_equal_eager():
    """simple_spread N = 3, 16 env copies, B = 32: three train_step(2) calls and one
    train_steps group are bit-equal with graphs on and off"""
    engs = [_scn_engine(g) for g in (True, False)]
    for e in engs:
        for _ in range(3):
            e.train_step(2)
        e.train_steps([1, 2, 0, 1])
        e.train_steps([1, 2, 0, 1])
        e.synchronize()
    for i in range(3):
        a, b = _all_sets(engs[0], i), _all_sets(engs[1], i)
        assert all(_equal_sets(a, b).values()), (i, _equal_sets(a, b))
        ia = engs[0].td3_info(i)
        assert ia == engs[1].td3_info(i) and (ia["critic_updates"], ia["actor_updates"]) == (14, 7)
    assert torch.equal(engs[0].region("replay"), engs[1].region("replay"))
    assert np.array_equal(engs[0].get_rng_state(), engs[1].get_rng_state())
    assert engs[0].check_finite() == 0


def test_td3_refusals_leave_the_handle_training():
    dims = [6, 5, 4]
    c = _case(dims, seed=16)
    eng = _engine(c, dims, d=2)
    idx = torch.from_numpy(c["idx"][0]).to(eng.device)
    buf = torch.empty(eng.lib.mdp_td3_bytes(eng.cfg), dtype=torch.uint8, device=eng.device)

    def refused(fn, *a, match):
        with pytest.raises(_lib.MdpError, match=match):
            fn(*a)

    refused(eng._c, "mdp_td3_enable", eng._ptr(buf), buf.numel(), 2, match="mdp_td3_enable: already enabled")
    refused(eng._c, "mdp_per_enable", eng._ptr(buf), buf.numel(), 0.6, 0.4, 0.001, 0.01, 1.0, match="MATD3")
    refused(eng.set_update_mode, "throughput", match="mdp_set_update_mode")
    refused(eng.update_all, match="mdp_update_all")
    refused(eng.dp_init, 2, 0, b"\0" * 128, match="mdp_dp_init")
    refused(eng.dp_xgmi_open, 2, 0, match="mdp_dp_xgmi_open")
    refused(eng.critic_grad, 0, idx, match="mdp_critic_grad")
    refused(eng.actor_grad, 0, idx, match="mdp_actor_grad")
    refused(eng.reduce_grad, 0, 1, match="mdp_reduce_grad")
    refused(eng.apply_grad, 0, 1, match="mdp_apply_grad")
    _update(eng, c, 0)                                  # still trains
    assert eng.td3_info(0)["critic_updates"] == 1 and eng.check_finite() == 0

    # a handle without TD3: the new ids are refused; enable's own argument checks
    plain = _engine(c, dims, td3=False)
    refused(plain.get_params, 0, "critic2", match="which")
    refused(plain.set_params, 0, "g_critic2", c["params"][0]["critic"], match="which")
    refused(plain.get_beta_powers, 0, 2, match="mdp_get_beta_powers: net")
    refused(plain.set_beta_powers, 0, 2, np.ones(2, np.float32), match="mdp_set_beta_powers: net")
    refused(plain.td3_info, 0, match="mdp_td3_info")
    for delay in (0, 9):
        refused(plain._c, "mdp_td3_enable", plain._ptr(buf), buf.numel(), delay, match="policy_delay")
    refused(plain._c, "mdp_td3_enable", None, buf.numel(), 2, match="buf_dev")
    host = np.zeros(buf.numel(), np.uint8)
    refused(plain._c, "mdp_td3_enable", host.ctypes.data, buf.numel(), 2, match="buf_dev")
    refused(plain._c, "mdp_td3_enable", plain._ptr(buf), buf.numel() - 1, 2, match="bytes")
    _update(plain, c, 0)                                # a refused enable leaves a MADDPG handle
    refused(plain._c, "mdp_td3_enable", plain._ptr(buf), buf.numel(), 2, match="before the handle's first update")
    _update(plain, c, 1)

    # either order: TD3 after prioritized replay, after throughput mode
    with pytest.raises(_lib.MdpError, match="prioritized"):
        Engine(dims, batch_size=B, capacity=L + 7, td3=True, prioritized=True)
    per = Engine(dims, batch_size=B, capacity=L + 7, prioritized=True)
    refused(per._c, "mdp_td3_enable", per._ptr(buf), buf.numel(), 2, match="prioritized replay")
    tp = Engine(dims, batch_size=B, capacity=L + 7)
    tp.set_update_mode("throughput")
    refused(tp._c, "mdp_td3_enable", tp._ptr(buf), buf.numel(), 2, match="strict update mode")
    with pytest.raises((ValueError, _lib.MdpError)):
        Engine(dims, batch_size=B, capacity=L + 7, td3=True, world_size=2)


def test_td3_enable_refuses_a_short_allocation():
    """a buffer that ends before mdp_td3_bytes, at the very end of a hipMalloc
    allocation.  Run where the runtime reports an allocation's exact extent (the
    library checks with the same hipMemGetAddressRange)."""
    import ctypes
    plain = Engine([6, 5, 4], batch_size=B, capacity=L + 7)
    nb = plain.lib.mdp_td3_bytes(plain.cfg)
    nbytes, base = 4 << 20, ctypes.c_void_p()
    assert 256 < nb < nbytes
    assert plain.lib.hipMalloc(ctypes.byref(base), ctypes.c_size_t(nbytes)) == 0
    try:
        rb, ext = ctypes.c_void_p(), ctypes.c_size_t()
        exact = (plain.lib.hipMemGetAddressRange(ctypes.byref(rb), ctypes.byref(ext), base) == 0
                 and rb.value == base.value and ext.value == nbytes)
        if not exact:
            pytest.skip(f"runtime reports extent {ext.value} for a {nbytes}-byte allocation")
        short = ctypes.c_void_p(base.value + nbytes - (nb - 256))
        with pytest.raises(_lib.MdpError, match="mdp_td3_enable: buf_dev .*allocation too small"):
            plain._c("mdp_td3_enable", short, nb, 2)
    finally:
        torch.cuda.synchronize()
        assert plain.lib.hipFree(base) == 0
    c = _case([6, 5, 4], seed=19)
    for i, p in enumerate(c["params"]):
        for w in NETS4:
            plain.set_params(i, w, p[w])
    plain.add_rows(torch.from_numpy(joint_rows(c["data"], [6, 5, 4])))
    _update(plain, c, 0)
    assert plain.check_finite() == 0


def test_td3_checkpoint_round_trip(tmp_path):
    dims = [6, 5, 4]
    c = _case(dims, seed=17)
    eng = _engine(c, dims, d=2)
    for r in range(2):
        for i in range(len(dims)):
            _update(eng, c, i)
    sd = eng.state_dict()
    for i in range(len(dims)):
        for w in TWIN_SETS:
            assert f"agent_{i}/{w}/W1" in sd
        assert f"agent_{i}/critic2/beta_power" in sd
    path = eng.save_state(str(tmp_path / "ck"))
    with pytest.raises(ValueError, match="tf1"):
        eng.save_state(str(tmp_path / "ck_tf1"), fmt="tf1")
    other = _engine(_case(dims, seed=18), dims, d=2)
    other.load_state(path)
    for i in range(len(dims)):
        a, b = _all_sets(eng, i), _all_sets(other, i)
        assert all(_equal_sets(a, b).values()), (i, _equal_sets(a, b))
    # a MADDPG checkpoint leaves the twin as it is; a MADDPG engine ignores the twin's keys
    keep = _all_sets(other, 0)
    other.load_state_dict({k: v for k, v in sd.items() if "critic2" not in k})
    now = _all_sets(other, 0)
    assert all(np.array_equal(keep[w][k], now[w][k]) for w in TWIN_SETS for k in keep[w])
    plain = _engine(c, dims, td3=False)
    plain.load_state_dict(sd)
    assert all(np.array_equal(plain.get_params(1, "critic")[k], eng.get_params(1, "critic")[k]) for k in nets.NAMES)
    # evaluation-side readers work unchanged on a TD3 engine
    assert eng.act(0, torch.from_numpy(c["data"][0][0][:8].astype(np.float32))).shape == (8, 5)
    st = eng.stats(0)
    assert len(UPDATE_STAT_DTYPES) == len(st) == 6


def test_td3_trainer_facade_update_returns_the_reference_list():
    """MADDPGAgentTrainer with args.td3: update() past the gates returns the reference's
    list with its dtypes; p_loss is 0 until the agent's first actor step (its second update)"""
    import argparse
    import random

    from maddpg_amd.common import tf_util as U
    from maddpg_amd.envs import Discrete
    from maddpg_amd.trainer.maddpg import MADDPGAgentTrainer
    args = argparse.Namespace(lr=1e-2, gamma=0.95, batch_size=16, num_units=64, max_episode_len=2, td3=True,
                              policy_delay=2)
    rng = np.random.default_rng(0)
    with U.single_threaded_session():
        trainers = [MADDPGAgentTrainer(f"agent_{i}", None, [(6,)] * 2, [Discrete(5)] * 2, i, args) for i in range(2)]
        U.initialize()
        eng = U.get_session().engine()
        assert eng.td3 and eng.policy_delay == 2
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
        assert losses[0][1][1] == 0 and losses[1][1][1] == 0 and losses[2][1][1] != 0 and losses[3][1][1] != 0
        assert eng.td3_info(0)["actor_updates"] == 1 and eng.td3_info(1)["critic_updates"] == 2
