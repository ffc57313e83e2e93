"""GPU: per-agent action widths (mdp_set_act_dims) through the trainer kernels,
against the mixed-width restatement of tests/mixed_width.py.

Structure and tolerances of tests/test_gpu_parity.py::_update_parity: loss 1e-5
relative, reduced gradients 1e-5 of the tensor's scale, well-conditioned
weights 1e-6, every weight 2e-4, beta powers exact.
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
from oracle import nets, philox, trainer  # noqa: E402
from tests import mixed_width as mw  # noqa: E402
from tests import per_oracle as po  # noqa: E402

ACT = 5
SETS = ("actor", "critic", "tgt_actor", "tgt_critic")


def _engine(c, B, L, H=64, **kw):
    eng = Engine(c["dims"], c["local_q"], num_units=H, batch_size=B, capacity=L + 7, act_dims=c["widths"], **kw)
    eng.add_rows(torch.from_numpy(mw.joint_rows_w(c["data"], c["dims"])))
    for i, p in enumerate(c["params"]):
        for w in SETS:
            eng.set_params(i, w, p[w])
    return eng


def _agents(c):
    return [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][i]) for i, p in enumerate(c["params"])]


def _check_agent(eng, i, agents, got, want, og):
    """one agent's update against the restatement (the checks of _update_parity)"""
    dg_all = eng.get_grads(i)
    conditioned = {}
    worst_g = 0.0
    for net, name in (("critic", "grad_critic"), ("actor", "grad_actor")):
        dg = dg_all[net]
        for k, ref in og[name].items():
            ref = np.asarray(ref, np.float64).reshape(dg[k].shape)
            scale = float(np.abs(ref).max()) or 1.0
            gerr = float(np.abs(dg[k] - ref).max()) / scale
            worst_g = max(worst_g, gerr)
            assert gerr < 1e-5, (i, name, k, gerr)
            conditioned[(net, k)] = np.abs(ref) > 1e-3 * scale
    assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]) + 1e-7, (got[0], want[0])
    np.testing.assert_allclose(got[1:], want[1:], rtol=2e-5, atol=2e-6)
    worst_w = 0.0
    for w, ref in (("actor", agents[i].actor), ("critic", agents[i].critic),
                   ("tgt_actor", agents[i].tgt_actor), ("tgt_critic", agents[i].tgt_critic)):
        dev = eng.get_params(i, w)
        for k in ref:
            assert dev[k].shape == ref[k].shape, (i, w, k, dev[k].shape, ref[k].shape)
            err = np.abs(dev[k] - ref[k])
            worst_w = max(worst_w, float(err.max()))
            if w in ("actor", "critic"):
                m = conditioned[(w, k)].reshape(err.shape)
                assert (float(err[m].max()) if m.any() else 0.0) < 1e-6, (i, w, k)
            assert err.max() < 2e-4, (i, w, k, float(err.max()))
    for net in (0, 1):
        bp = eng.get_beta_powers(i, net)
        opt = agents[i].opt_actor if net == 0 else agents[i].opt_critic
        assert bp[0] == opt.b1p and bp[1] == opt.b2p
    return worst_g, worst_w


def _strict_round(c, B, L, H=64, variant=None):
    eng = _engine(c, B, L, H)
    n = len(c["dims"])
    if variant is not None:
        assert [eng.lib.mdp_grad_variant(eng.h, i) for i in range(n)] == [variant] * n
    agents = _agents(c)
    wg = ww = 0.0
    for i in range(n):
        eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                   u_act=torch.from_numpy(c["u_act"][i]))
        got = eng.stats(i)
        want, og = mw.update(agents, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], c["widths"])
        g, w = _check_agent(eng, i, agents, got, want, og)
        wg, ww = max(wg, g), max(ww, w)
    print(f"mixed-width round dims={c['dims']} widths={c['widths']} B={B} H={H} local_q={c['local_q']}: "
          f"worst grad |diff|/max|g| = {wg:.3e}, worst param |diff| = {ww:.3e}")
    return eng


# B = 40: two full 16-row tiles plus 8 rows
def test_round_parity_fast_kernels():
    _strict_round(mw.mixed_case([3, 11], [3, 5], 40, 300, seed=31), 40, 300, variant=1)


def test_round_parity_general_kernels_h64(monkeypatch):
    monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
    _strict_round(mw.mixed_case([3, 11], [3, 5], 40, 300, seed=31), 40, 300, variant=0)


def test_round_parity_h128():
    _strict_round(mw.mixed_case([3, 11], [3, 5], 40, 300, seed=32, H=128), 40, 300, H=128, variant=0)


def test_round_parity_narrow_slot_last():
    _strict_round(mw.mixed_case([11, 3], [5, 3], 40, 300, seed=33), 40, 300)


def test_round_parity_three_agents_width_4():
    _strict_round(mw.mixed_case([6, 6, 6], [4, 4, 4], 24, 200, seed=34), 24, 200)


def test_round_parity_width_1_and_2():
    # the narrowest widths: a one-entry softmax is the constant 1 (zero gradient through it)
    _strict_round(mw.mixed_case([5, 7, 4], [1, 2, 5], 24, 200, seed=38), 24, 200)


def test_round_parity_ddpg_critic():
    _strict_round(mw.mixed_case([3, 11], [3, 5], 40, 300, seed=35, local_q=[True, False]), 40, 300)


@pytest.mark.parametrize("general", [False, True])
def test_throughput_round_parity(monkeypatch, general):
    """one mdp_update_all round (tolerances of test_throughput_mode_round_parity)"""
    if general:
        monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
    B, L = 40, 300
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=36)
    eng = _engine(c, B, L)
    eng.set_update_mode("throughput")
    agents = _agents(c)
    n = 2

    def round_grads():
        out = []
        for i in range(n):
            batch_n = [tuple(x[c["idx"][i]] for x in c["data"][j]) for j in range(n)]
            out.append({1: trainer.critic_grads(agents, i, batch_n, mw.narrow(c["u_tgt"][i], c["widths"]))[0],
                        0: mw.actor_grads(agents, i, batch_n, c["u_act"][i])[0]})
        return out

    old32 = (nets.F32, trainer.F32)
    nets.F32 = trainer.F32 = np.float64   # the fp64 restatement: what every fp32 order approximates
    try:
        og64 = round_grads()
    finally:
        nets.F32, trainer.F32 = old32
    eng.update_all(idx=torch.from_numpy(c["idx"]), u_tgt=torch.from_numpy(c["u_tgt"]),
                   u_act=torch.from_numpy(c["u_act"]))
    want, _ = mw.update_round_throughput(agents, c["data"], c["idx"], c["u_tgt"], c["u_act"], c["widths"])
    for i in range(n):
        got = eng.stats(i)
        assert abs(got[0] - want[i][0]) <= 1e-5 * abs(want[i][0]) + 1e-7, (i, got[0], want[i][0])
        np.testing.assert_allclose(got[1:], want[i][1:], rtol=2e-5, atol=2e-6)
        dg_all = eng.get_grads(i)
        conditioned = {}
        for net, name in ((0, "actor"), (1, "critic")):
            for k, r64 in og64[i][net].items():
                dg = dg_all[name][k]
                r64 = np.asarray(r64, np.float64).reshape(dg.shape)
                scale = float(np.abs(r64).max()) or 1.0
                assert float(np.abs(dg - r64).max()) / scale < 1e-5, (i, name, k)
                conditioned[(name, k)] = np.abs(r64) > 1e-3 * scale
        for w, ref in (("actor", agents[i].actor), ("critic", agents[i].critic),
                       ("tgt_actor", agents[i].tgt_actor), ("tgt_critic", agents[i].tgt_critic)):
            dev = eng.get_params(i, w)
            for k in ref:
                e = np.abs(dev[k] - ref[k])
                if w in ("actor", "critic"):
                    m = conditioned[(w, k)].reshape(e.shape)
                    assert (float(e[m].max()) if m.any() else 0.0) < 1e-6, (i, w, k)
                assert e.max() < 2e-4, (i, w, k)


def test_device_noise_uses_the_first_columns_of_the_pinned_streams():
    """no injected uniforms: agent i's strict update draws uniforms5 on the streams
    of tests/test_gpu_parity.py::_philox_case_noise and uses their first A_j columns"""
    B, L, key = 40, 300, 0x5EED5EED00C0FFEE
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=37)
    rows = np.arange(B)
    n = 2
    c["u_tgt"] = [np.stack([philox.uniforms5(key, (i << 8) | (j + 1), i, rows) for j in range(n)]) for i in range(n)]
    c["u_act"] = [philox.uniforms5(key, (i << 8) | 0x80, i, rows) for i in range(n)]
    eng = _engine(c, B, L, seed=key)
    agents = _agents(c)
    for i in range(n):
        eng.update(i, idx=torch.from_numpy(c["idx"][i]))
        got = eng.stats(i)
        want, og = mw.update(agents, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], c["widths"])
        _check_agent(eng, i, agents, got, want, og)
    # the act path: the sample of the 3-wide agent from the first 3 of its 5 pinned uniforms
    obs = c["data"][0][0][:B].astype(np.float32)
    got = eng.act(0, torch.from_numpy(obs)).cpu().numpy()
    assert got.shape == (B, 3)
    u = philox.uniforms5(key, 0x40000 | (0 << 1) | 0, 0, np.arange(B))[:, :3]
    np.testing.assert_allclose(got, trainer.act(agents[0], obs, u), atol=2e-6)


def _pad_masks(eng, c):
    """boolean mask over one param-space region: True at every action-width pad entry"""
    mask = np.zeros(eng.param_floats, bool)
    for i in range(eng.n):
        off, _r, _c, dr, dc = eng.net_tensors(i, 0)[4]          # actor W3 [H][5]
        m = np.zeros((dr, dc), bool)
        m[:, c["widths"][i]:] = True
        mask[off:off + dr * dc] = m.ravel()
        off, _r, _c, dr, dc = eng.net_tensors(i, 0)[5]          # actor b3 [5]
        mask[off + c["widths"][i]:off + dc] = True
        off, _r, _c, dr, dc = eng.net_tensors(i, 1)[0]          # critic W1 [cin][H]
        m = np.zeros((dr, dc), bool)
        m[mw.pad_columns(c["dims"], c["widths"], c["local_q"][i], i), :] = True
        mask[off:off + dr * dc] = m.ravel()
    return mask


@pytest.mark.parametrize("local_q", [None, [True, False]])
def test_pad_entries_stay_exactly_zero(local_q):
    B, L = 40, 300
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=41, local_q=local_q)
    eng = _engine(c, B, L)
    mask = _pad_masks(eng, c)
    # agent 0's actor: 2 pad columns of W3 [64][5] and of b3; each critic's W1: 2 pad rows of 64
    assert mask.sum() == 2 * 64 + 2 + 2 * (2 * 64)
    for _ in range(3):
        for i in range(2):
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                       u_act=torch.from_numpy(c["u_act"][i]))
    eng.synchronize()
    for name in ("theta", "target", "adam_m", "adam_v", "grad"):
        r = eng.region(name).cpu().numpy()[:eng.param_floats]
        assert np.isfinite(r).all()
        assert (r[mask] == 0.0).all(), name
        assert (r[~mask] != 0.0).any(), name


def _bits(eng):
    return [eng.region(name).cpu().numpy().view(np.uint32).copy() for name in ("theta", "target", "adam_m", "adam_v")]


def test_nan_in_pad_uniforms_changes_nothing():
    B, L = 40, 300
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=42)
    out = []
    for fill in (0.0, np.nan):
        u_tgt, u_act = c["u_tgt"].copy(), c["u_act"].copy()
        u_tgt[:, 0, :, 3:] = fill           # agent 0 is 3 wide: columns 3, 4 of its uniforms are pad
        u_act[0, :, 3:] = fill
        eng = _engine(c, B, L)
        for i in range(2):
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(u_tgt[i]),
                       u_act=torch.from_numpy(u_act[i]))
        eng.synchronize()
        out.append((_bits(eng), [np.asarray(eng.stats(i)).view(np.uint64) for i in range(2)]))
        u = torch.full((B, 5), float(fill))
        u[:, :3] = torch.from_numpy(c["u_act"][0][:, :3])
        out[-1][1].append(eng.act(0, torch.from_numpy(c["data"][0][0][:B].astype(np.float32)), u=u)
                          .cpu().numpy().view(np.uint32))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert np.array_equal(a, b)


def test_all_5_given_explicitly_is_the_default_bit_for_bit():
    from tests.helpers import joint_rows, synthetic_trainer_case
    dims, B, L = [18, 18, 18], 48, 300
    c = synthetic_trainer_case(dims, B, L, seed=43)
    res = []
    for kw in ({}, {"act_dims": [5, 5, 5]}):
        eng = Engine(dims, batch_size=B, capacity=L + 7, **kw)
        assert eng.act_dims == [5, 5, 5]
        eng.add_rows(torch.from_numpy(joint_rows(c["data"], dims)))
        for i, p in enumerate(c["params"]):
            for w in SETS:
                eng.set_params(i, w, p[w])
        for i in range(3):
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                       u_act=torch.from_numpy(c["u_act"][i]))
        eng.synchronize()
        res.append(_bits(eng) + [np.asarray(eng.stats(i)).view(np.uint64) for i in range(3)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def _dims(*w):
    return (ctypes.c_int32 * _lib.MAX_AGENTS)(*w)


def test_set_act_dims_contract():
    eng = Engine([3, 11], batch_size=8, capacity=64)
    lib, h = eng.lib, eng.h
    for bad in ((0, 5), (3, 6), (-1, 5)):
        assert lib.mdp_set_act_dims(h, _dims(*bad)) < 0
        assert b"1..5" in lib.mdp_last_error(h)
    assert lib.mdp_set_act_dims(h, None) < 0
    assert eng.act_dims == [5, 5]
    assert lib.mdp_set_act_dims(h, _dims(3, 5)) == 0
    got = _dims()
    assert lib.mdp_get_act_dims(h, got) == 0 and list(got) == [3, 5, 0, 0, 0, 0, 0, 0]
    assert lib.mdp_set_act_dims(h, _dims(2, 4)) == 0           # still unused: may change again
    # refused after the first parameter write ...
    eng2 = Engine([3, 11], batch_size=8, capacity=64, act_dims=[3, 5])
    eng2.init_params(0)
    assert lib.mdp_set_act_dims(eng2.h, _dims(3, 5)) < 0
    assert b"before the handle's first" in lib.mdp_last_error(eng2.h)
    # ... after the first act ...
    eng3 = Engine([3, 11], batch_size=8, capacity=64)
    eng3.act(0, torch.zeros(4, 3))
    assert lib.mdp_set_act_dims(eng3.h, _dims(3, 5)) < 0
    # ... and after the first update
    c = mw.mixed_case([3, 11], [3, 5], 8, 40, seed=1)
    eng4 = Engine([3, 11], batch_size=8, capacity=64)
    eng4.add_rows(torch.from_numpy(mw.joint_rows_w(c["data"], c["dims"])))
    eng4.update(0, idx=torch.from_numpy(c["idx"][0]))
    assert lib.mdp_set_act_dims(eng4.h, _dims(3, 5)) < 0
    with pytest.raises(_lib.MdpError, match="before the handle's first"):
        eng4.set_act_dims([3, 5])
    with pytest.raises(ValueError, match="1..5"):
        Engine([3, 11], batch_size=8, capacity=64, act_dims=[3, 6])
    with pytest.raises(ValueError, match="entries"):
        Engine([3, 11], batch_size=8, capacity=64, act_dims=[3])


def test_scenario_handle_keeps_its_own_widths():
    from maddpg_amd.envs import spec
    sp = spec("simple_spread")
    with pytest.raises(ValueError, match="scenario"):
        Engine(sp.obs_dims, batch_size=8, capacity=64, num_envs=4, scenario="simple_spread", act_dims=[5, 3, 5])
    eng = Engine(sp.obs_dims, batch_size=8, capacity=64, num_envs=4, scenario="simple_spread", act_dims=[5, 5, 5])
    assert eng.act_dims == [5, 5, 5]
    eng.env_reset()
    assert eng.lib.mdp_set_act_dims(eng.h, _dims(5, 5, 5)) < 0      # after the first env call


@pytest.mark.parametrize("dims,widths,local_q,H,units", [
    ([3, 11], [3, 5], None, 64, 64), ([11, 3, 4], [5, 3, 2], [False, True, False], 64, 50),
    ([3, 11], [3, 5], None, 128, 128)])
def test_logical_shapes_and_param_round_trip(dims, widths, local_q, H, units):
    n, S = len(dims), sum(dims)
    eng = Engine(dims, local_q, num_units=units, batch_size=8, capacity=64, act_dims=widths)
    lq = eng.local_q
    rng = np.random.default_rng(3)
    for i in range(n):
        cin = dims[i] + widths[i] if lq[i] else S + sum(widths)
        want = {0: [(dims[i], units), (1, units), (units, units), (1, units), (units, widths[i]), (1, widths[i])],
                1: [(cin, units), (1, units), (units, units), (1, units), (units, 1), (1, 1)]}
        for net in (0, 1):
            got = [(r, c_) for (_o, r, c_, _dr, _dc) in eng.net_tensors(i, net)]
            assert got == want[net], (i, net, got)
        dev = eng.net_tensors(i, 1)[0]
        assert (dev[3], dev[4]) == ((dims[i] + 5) if lq[i] else S + 5 * n, H)
        for which in ("actor", "critic", "tgt_critic", "m_critic", "g_actor"):
            net = 1 if "critic" in which else 0
            x = {k: rng.normal(size=(r, c_) if k.startswith("W") else (c_,)).astype(np.float32)
                 for k, (r, c_) in zip(nets.NAMES, want[net])}
            eng.set_params(i, which, x)
            back = eng.get_params(i, which)
            for k in x:
                assert np.array_equal(back[k], x[k]), (i, which, k)
    # the raw device block: logical rows at their slots, interior pad rows zero
    i = 0
    off, r, c_, dr, dc = eng.net_tensors(i, 1)[0]
    blk = eng.region("theta").cpu().numpy()[off:off + dr * dc].reshape(dr, dc)
    w1 = eng.get_params(i, "critic")["W1"]
    cols = eng.cin_columns(i)
    assert np.array_equal(blk[cols][:, :units], w1)
    pad = sorted(set(range(dr)) - set(cols))
    assert len(pad) == dr - r and (blk[pad] == 0).all() and (blk[:, units:] == 0).all()
    # init_params: Xavier limits from the logical shapes (fan-in = the logical cin)
    eng.init_params(1)
    for i in range(n):
        p = eng.get_params(i, "critic")
        lim = np.sqrt(6.0 / (p["W1"].shape[0] + units))
        assert np.abs(p["W1"]).max() <= lim and np.abs(p["W1"]).max() > 0.9 * lim
        p = eng.get_params(i, "actor")
        lim = np.sqrt(6.0 / (units + widths[i]))
        assert p["W3"].shape == (units, widths[i]) and np.abs(p["W3"]).max() <= lim


def test_act_logits_and_q_values_take_logical_widths():
    B, L = 40, 300
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=44)
    eng = _engine(c, B, L)
    agents = _agents(c)
    obs = [c["data"][j][0][:B].astype(np.float32) for j in range(2)]
    act = [c["data"][j][1][:B] for j in range(2)]
    lg = eng.actor_logits(0, torch.from_numpy(obs[0])).cpu().numpy()
    assert lg.shape == (B, 3)
    np.testing.assert_allclose(lg, nets.mlp_fwd(agents[0].actor, obs[0])[0], atol=2e-6)
    u = c["u_act"][0][:, :3]
    a = eng.act(0, torch.from_numpy(obs[0]), target=True, u=torch.from_numpy(u)).cpu().numpy()
    assert a.shape == (B, 3)
    np.testing.assert_allclose(a, trainer.target_act(agents[0], obs[0], u), atol=2e-6)
    np.testing.assert_allclose(a.sum(1), 1.0, atol=1e-6)
    x = np.concatenate(obs + act, 1)                             # logical width 3 + 11 + 3 + 5
    q = eng.q_values(1, torch.from_numpy(x)).cpu().numpy()
    np.testing.assert_allclose(q, nets.mlp_fwd(agents[1].critic, x)[0][:, 0], rtol=1e-5, atol=2e-6)
    with pytest.raises(ValueError):
        eng.q_values(1, torch.zeros(4, 21))


@pytest.mark.parametrize("fmt", ["npz", "tf1"])
def test_checkpoint_round_trip_stores_logical_shapes(tmp_path, fmt):
    B, L = 40, 300
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=45)

    def one_round(eng, r):
        for i in range(2):
            eng.update(i, idx=torch.from_numpy(c["idx"][(i + r) % 2]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                       u_act=torch.from_numpy(c["u_act"][i]))
        eng.synchronize()

    eng = _engine(c, B, L)
    one_round(eng, 0)
    fname = str(tmp_path / "ck" / "model")
    (tmp_path / "ck").mkdir()
    eng.save_state(fname, fmt)
    sd = eng.state_dict()
    assert sd["agent_0/actor/W3"].shape == (64, 3) and sd["agent_0/actor/b3"].shape == (3,)
    assert sd["agent_0/critic/W1"].shape == (3 + 11 + 3 + 5, 64) and sd["agent_1/v_critic/W1"].shape == (22, 64)
    if fmt == "npz":
        with np.load(eng.checkpoint_path(fname)) as z:
            assert z["agent_0/tgt_actor/W3"].shape == (64, 3) and z["agent_1/m_critic/W1"].shape == (22, 64)
    else:
        from maddpg_amd.common import tf_checkpoint as tfc
        shapes = {tuple(v.shape) for v in tfc.read_bundle(fname).values()}
        assert {(64, 3), (3,), (64, 5), (5,), (22, 64)} <= shapes
        assert (24, 64) not in shapes                            # the device block of the joint critic's W1
    eng2 = Engine(c["dims"], batch_size=B, capacity=L + 7, act_dims=c["widths"])
    eng2.add_rows(torch.from_numpy(mw.joint_rows_w(c["data"], c["dims"])))
    eng2.load_state(fname)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)
    one_round(eng, 1)
    one_round(eng2, 1)
    for a, b in zip(_bits(eng), _bits(eng2)):
        assert np.array_equal(a, b)
    assert [eng.stats(i) for i in range(2)] == [eng2.stats(i) for i in range(2)]


def test_prioritized_round_matches_the_weighted_restatement():
    """tests/test_per_gpu.py::test_weighted_update_parity on the [3, 5] case"""
    B, L = 40, 300
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=46)
    eng = _engine(c, B, L, prioritized=True)
    P = po.tree_leaves(L + 7)
    rng = np.random.default_rng(8)
    agents = _agents(c)
    for i in range(2):
        prio = rng.uniform(0.05, 1.0, L).astype(np.float32)
        eng.per_set_priorities(i, torch.arange(L, dtype=torch.int32), torch.from_numpy(prio))
        idx = c["idx"][i]
        w = po.weights(po.build(prio, P), idx, po.beta_after(1))
        eng.update(i, idx=torch.from_numpy(idx), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                   u_act=torch.from_numpy(c["u_act"][i]))
        got = eng.stats(i)
        s_idx, s_w, s_td = (x.cpu().numpy() for x in eng.per_slots(i))
        assert (s_idx == idx).all()
        np.testing.assert_allclose(s_w, w, rtol=2e-6)
        batch_n = [tuple(x[idx] for x in c["data"][j]) for j in range(2)]
        ag = agents[i]
        gq, st = po.critic_grads(agents, i, batch_n, mw.narrow(c["u_tgt"][i], c["widths"]), w)
        trainer.apply_grads(ag.opt_critic, ag.critic, gq)
        gp, p_loss = mw.actor_grads(agents, i, batch_n, c["u_act"][i])
        trainer.apply_grads(ag.opt_actor, ag.actor, gp)
        nets.polyak(ag.tgt_actor, ag.actor)
        nets.polyak(ag.tgt_critic, ag.critic)
        want = trainer.reference_stats(st, p_loss)
        _check_agent(eng, i, agents, got, want, {"grad_critic": gq, "grad_actor": gp})
        tol = 1e-5 * np.maximum(np.maximum(np.abs(st["q"]), np.abs(st["y"])), 1.0)
        assert (np.abs(s_td - st["td"]) <= tol).all()


def test_update_round_graph_equals_eager():
    """mdp_update_round (device-drawn indices and noise) captured and eager: bit-identical"""
    B, L = 40, 300
    c = mw.mixed_case([3, 11], [3, 5], B, L, seed=47)
    res = []
    for graphs in (True, False):
        eng = _engine(c, B, L, seed=9)
        eng.seed_py_random(5)
        eng.set_graphs(graphs)
        for _ in range(3):
            eng.update_round()
        eng.synchronize()
        res.append(_bits(eng))
        assert eng.check_finite() == 0
    for a, b in zip(*res):
        assert np.array_equal(a, b)
