"""CPU: the Box restatement of tests/box_actions.py against an independent
derivation (torch.autograd in float64), the Box-Muller normals' moments and
edges, the env mapping through the unchanged CPU env, the CLI refusals and
the logical shapes.
"""
import argparse

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import mpe, nets, philox, trainer  # noqa: E402
from tests import box_actions as ba  # noqa: E402
from tests.test_oracle_autograd import F64, _cin, _gsm, _mlp, _t, fp64_oracle  # noqa: E402

BOX2, BOX1, D3, D5 = ("box", 2), ("box", 1), ("discrete", 3), ("discrete", 5)
CASES = [([6, 4], [BOX2, BOX2], 16, None, 64), ([3, 11], [D3, BOX2], 16, None, 64),
         ([5, 7, 4], [BOX1, D5, BOX2], 24, [False, True, False], 64), ([6, 4], [BOX2, BOX1], 16, None, 128)]


def _normals(u):
    r = torch.sqrt(-2.0 * torch.log(1.0 - u[:, 0]))
    return torch.stack([r * torch.cos(2 * np.pi * u[:, 1]), r * torch.sin(2 * np.pi * u[:, 1])], 1)


def _sample(space, head, u):
    if ba.is_box(space):
        d = space[1]
        return head[:, :d] + torch.exp(head[:, d:2 * d]) * _normals(u)[:, :d]
    return _gsm(head, u[:, :space[1]])


def _setup(dims, spaces, B, local_q, H, seed):
    c = ba.box_case(dims, spaces, B, 4 * B, seed, local_q, H)
    n = len(dims)
    idx = c["idx"][0]
    batch_n = [tuple(np.asarray(x[idx], np.float64) for x in c["data"][j]) for j in range(n)]
    params = [{w: {k: np.asarray(v, np.float64) for k, v in p[w].items()} for w in p} for p in c["params"]]
    return c, n, batch_n, params


def _agents(params, lq):
    return [trainer.AgentParams(**{w: dict(p[w]) for w in p}, local_q=lq[j]) for j, p in enumerate(params)]


@pytest.mark.parametrize("dims,spaces,B,local_q,H", CASES)
def test_critic_grads_match_autograd(dims, spaces, B, local_q, H):
    gamma = 0.95
    c, n, batch_n, params = _setup(dims, spaces, B, local_q, H, seed=101)
    lq = c["local_q"]
    for i in range(n):
        u_tgt = np.asarray(c["u_tgt"][i], np.float64)
        with fp64_oracle():
            g, st = ba.critic_grads(_agents(params, lq), i, batch_n, u_tgt, spaces, gamma)
        obs_n = [torch.tensor(b[0], dtype=F64) for b in batch_n]
        act_n = [torch.tensor(b[1], dtype=F64) for b in batch_n]
        obs2_n = [torch.tensor(b[3], dtype=F64) for b in batch_n]
        rew, done = torch.tensor(batch_n[i][2], dtype=F64), torch.tensor(batch_n[i][4], dtype=F64)
        with torch.no_grad():
            tgt_act = [_sample(spaces[j], _mlp(_t(params[j]["tgt_actor"]), obs2_n[j]), torch.tensor(u_tgt[j], dtype=F64))
                       for j in range(n)]
            y = rew + gamma * (1.0 - done) * _mlp(_t(params[i]["tgt_critic"]), _cin(obs2_n, tgt_act, i, lq[i]))[:, 0]
        cp = _t(params[i]["critic"], grad=True)
        q = _mlp(cp, _cin(obs_n, act_n, i, lq[i]))[:, 0]
        loss = torch.mean((q - y) ** 2)
        gt = dict(zip(cp, torch.autograd.grad(loss, list(cp.values()))))
        assert abs(st["q_loss"] - loss.item()) <= 1e-12 * abs(loss.item())
        np.testing.assert_allclose(st["target_q"], y.numpy(), rtol=1e-12, atol=1e-12)
        for k in nets.NAMES:
            want = gt[k].numpy().reshape(np.shape(g[k]))
            np.testing.assert_allclose(g[k], want, rtol=1e-10, atol=1e-14 * max(1.0, np.abs(want).max()),
                                       err_msg=f"agent {i} critic {k}")


@pytest.mark.parametrize("dims,spaces,B,local_q,H", CASES)
def test_actor_grads_match_autograd(dims, spaces, B, local_q, H):
    reg = 1e-3
    c, n, batch_n, params = _setup(dims, spaces, B, local_q, H, seed=202)
    lq = c["local_q"]
    for i in range(n):
        u_act = np.asarray(c["u_act"][i], np.float64)
        with fp64_oracle():
            g, p_loss = ba.actor_grads(_agents(params, lq), i, batch_n, u_act, spaces, actor_reg=reg)
        obs_n = [torch.tensor(b[0], dtype=F64) for b in batch_n]
        act_n = [torch.tensor(b[1], dtype=F64) for b in batch_n]
        ap = _t(params[i]["actor"], grad=True)
        head = _mlp(ap, obs_n[i])
        assert head.shape[1] == ba.head_w(spaces[i])
        act_in = list(act_n)
        act_in[i] = _sample(spaces[i], head, torch.tensor(u_act, dtype=F64))
        q = _mlp(_t(params[i]["critic"]), _cin(obs_n, act_in, i, lq[i]))[:, 0]
        loss = -torch.mean(q) + reg * torch.mean(head ** 2)       # p_reg over B * 2 d entries
        gt = dict(zip(ap, torch.autograd.grad(loss, list(ap.values()))))
        assert abs(p_loss - loss.item()) <= 1e-12 * abs(loss.item())
        for k in nets.NAMES:
            want = gt[k].numpy().reshape(np.shape(g[k]))
            np.testing.assert_allclose(g[k], want, rtol=1e-10, atol=1e-14 * max(1.0, np.abs(want).max()),
                                       err_msg=f"agent {i} actor {k}")
            if k in ("W3", "b3"):
                assert np.abs(want).max(axis=0).min() > 0      # every head column, logstd included, is trained


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_muller_moments_over_a_million_philox_uniforms(dtype):
    N = 1_000_000
    u = philox.uniforms5(0x5EED5EED00C0FFEE, 0x40000, 3, np.arange(N))
    assert u.shape == (N, 5) and u.min() >= 0.0 and u.max() < 1.0
    eps = ba.box_muller(u, dtype).astype(np.float64)
    assert eps.shape == (N, 2) and np.isfinite(eps).all() and np.abs(eps).max() < 5.7
    for k in range(2):
        assert abs(eps[:, k].mean()) < 5 * 1.0 / np.sqrt(N)                     # SE of the mean of N(0, 1)
        assert abs(eps[:, k].var() - 1.0) < 5 * np.sqrt(2.0 / N)                # SE of its variance
    assert abs(np.mean(eps[:, 0] * eps[:, 1])) < 5 * 1.0 / np.sqrt(N)           # SE of the cross moment
    # a NaN in the unread uniforms changes no bit
    v = u[:4096].copy()
    v[:, 2:] = np.nan
    assert np.array_equal(ba.box_muller(v, dtype), ba.box_muller(u[:4096], dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_output_is_finite_at_the_edges(dtype):
    below1 = np.nextafter(np.float32(1), np.float32(0))
    u0, u1 = [0.0, below1], [0.0, 0.25, 0.5, below1]
    u = np.array([[a, b, np.nan, np.nan, np.nan] for a in u0 for b in u1], np.float32)
    eps = ba.box_muller(u, dtype)
    assert np.isfinite(eps).all()
    assert np.all(eps[:4] == 0)                                  # u0 = 0: r = sqrt(-2 ln 1) = 0
    r = np.sqrt(-2 * np.log(1 - np.float64(below1)))
    # (1 - 2^-24; the device's own uniforms end at 1 - 2^-23, where r is about 5.65)
    assert 5.76 < r < 5.78 and np.abs(eps).max() <= r * (1 + 1e-6)
    for logstd in (-20.0, 0.0, 5.0):
        for d in (1, 2):
            flat = np.concatenate([np.full((len(u), d), 0.3), np.full((len(u), d), logstd)], 1).astype(dtype)
            a, se = ba.gaussian_sample(flat, u, d, dtype)
            da = np.full((len(u), d), -1.0 / 16, dtype)
            g = ba.gaussian_bwd(flat, da, se, d, 2e-3 / (16 * 2 * d), dtype)
            assert a.shape == (len(u), d) and g.shape == (len(u), 2 * d)
            assert a.dtype == dtype and g.dtype == dtype
            assert np.isfinite(a).all() and np.isfinite(se).all() and np.isfinite(g).all()


def test_to_mpe5_through_the_cpu_env_is_the_direct_force():
    rng = np.random.default_rng(0)
    E, n = 7, 3
    sc = mpe.SimpleSpread(n)
    ne = 2 * n
    st = {"pos": rng.uniform(-1, 1, (E, ne, 2)), "vel": rng.normal(size=(E, ne, 2)) * 0.1,
          "goal": np.zeros(E, np.int32)}
    st["vel"][:, n:] = 0
    a = rng.normal(size=(E, n, 2))
    a5 = ba.to_mpe5(a)
    assert a5.shape == (E, n, 5) and np.all(a5[..., [0, 2, 4]] == 0)
    nst, _obs, _rew = sc.step({k: v.copy() for k, v in st.items()}, a5)
    # the same world with no action at all, then the force (ux, uy) * sensitivity added by hand:
    # v' = v (1 - damping) + (f_contact + f_action) / mass * dt, so the difference is f_action * dt
    zst, _o, _r = sc.step({k: v.copy() for k, v in st.items()}, np.zeros((E, n, 5)))
    dv = nst["vel"][:, :n] - zst["vel"][:, :n]
    np.testing.assert_allclose(dv, a * 5.0 * 0.1, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(nst["vel"][:, n:], 0)


def _args(**kw):
    base = dict(continuous_actions=True, prioritized_replay=False, td3=False, minimax=False, approx_policies=False,
                update_mode="strict", num_gpus=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_continuous_flags_refusals():
    from experiments.train import continuous_flags, parse_args
    continuous_flags(_args())                                     # passes
    continuous_flags(_args(continuous_actions=False, td3=True))   # not asked for: nothing to refuse
    for kw, msg in ((dict(prioritized_replay=True), "--prioritized-replay"), (dict(td3=True), "--td3"),
                    (dict(minimax=True), "--minimax"), (dict(approx_policies=True), "--approx-policies"),
                    (dict(update_mode="throughput"), "--update-mode strict"), (dict(num_gpus=2), "one GPU")):
        with pytest.raises(SystemExit, match=msg):
            continuous_flags(_args(**kw))
    with pytest.raises(SystemExit, match="one GPU"):
        continuous_flags(_args(), world=2)
    a = parse_args(["--scenario", "simple", "--continuous-actions"])
    assert a.continuous_actions is True and parse_args([]).continuous_actions is False


def test_logical_shapes_and_spaces():
    from maddpg_amd.envs import Box, Discrete, spec
    c = ba.box_case([5, 7, 4], [BOX1, D5, BOX2], 16, 64, seed=3, local_q=[False, True, False])
    assert c["widths"] == [1, 5, 2] and c["heads"] == [2, 5, 4] and c["kinds"] == ["box", "discrete", "box"]
    assert [p["actor"]["W3"].shape for p in c["params"]] == [(64, 2), (64, 5), (64, 4)]
    assert [p["critic"]["W1"].shape[0] for p in c["params"]] == [16 + 8, 7 + 5, 16 + 8]
    assert [d[1].shape[1] for d in c["data"]] == [1, 5, 2]
    assert np.abs(c["data"][2][1]).max() > 1.5                    # N(0, 1)-scale floats, not probabilities
    sp = spec("simple_spread", continuous=True)
    assert sp.act_kinds == ["box"] * 3 and sp.act_dims == [2, 2, 2]
    assert all(isinstance(s, Box) and s.shape == (2,) and not hasattr(s, "n") for s in sp.action_space)
    sl = spec("simple_speaker_listener", continuous=True)
    assert sl.act_kinds == ["discrete", "box"] and sl.act_dims == [3, 2]
    assert isinstance(sl.action_space[0], Discrete) and sl.action_space[0].n == 3
    assert spec("simple_tag").act_kinds == ["discrete"] * 4 and spec("simple_tag").act_dims == [5] * 4
