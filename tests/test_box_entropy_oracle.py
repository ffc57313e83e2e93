"""CPU: the entropy restatement of tests/box_entropy.py against independent
derivations (torch.autograd and torch.distributions in float64), its edges, its
zero-coefficient identity with tests/box_squash.py, the entropy of the plain
Gaussian by Monte Carlo, and the CLI refusals.
"""
import argparse

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import nets, philox, trainer  # noqa: E402
from tests import box_actions as ba  # noqa: E402
from tests import box_entropy as be  # noqa: E402
from tests import box_squash as bs  # noqa: E402
from tests.test_box_actions_oracle import _agents, _normals  # noqa: E402
from tests.test_box_squash_oracle import CASES, IDS, _sample, _setup, _u_for_eps0  # noqa: E402
from tests.test_oracle_autograd import F64, _cin, _mlp, _t, fp64_oracle  # noqa: E402

# tests/test_box_squash_oracle.py's cases (d = 1 and 2, plain and tanh, MADDPG and DDPG critics, 64 and 128 units)
ALPHA = 0.2


def _alphas(spaces):
    """a coefficient on every Box agent, each its own"""
    return [ALPHA * (1 + j) if ba.is_box(s) else 0.0 for j, s in enumerate(spaces)]


def _torch_lp(space, head, u):
    """log pi of the reparameterised sample by torch.distributions: Normal.log_prob of
    the pre-squash value minus TanhTransform's log |det J|"""
    from torch.distributions import Normal
    from torch.distributions.transforms import TanhTransform
    d = space[1]
    mean, logstd = head[:, :d], head[:, d:2 * d]
    z = mean + torch.exp(logstd) * _normals(u)[:, :d]
    lp = Normal(mean, torch.exp(logstd)).log_prob(z)
    if bs.is_squashed(space):
        a = torch.tanh(z)
        lp = lp - TanhTransform().log_abs_det_jacobian(z, a)
    return lp.sum(1)


@pytest.mark.parametrize("dims,spaces,B,local_q,H", CASES, ids=IDS)
def test_log_probability_matches_torch_distributions(dims, spaces, B, local_q, H):
    rng = np.random.default_rng(7)
    for sp in spaces:
        if not ba.is_box(sp):
            continue
        d = sp[1]
        flat = rng.normal(size=(B, 2 * d))
        u = rng.uniform(0, 1, (B, 5))
        want = _torch_lp(sp, torch.tensor(flat, dtype=F64), torch.tensor(u, dtype=F64)).numpy()
        a, se, lp, z, eps = be.sample_lp(flat, u, d, bs.is_squashed(sp), np.float64)
        np.testing.assert_allclose(lp, want, rtol=1e-12, atol=1e-12)
        a32, _se, lp32, _z, _e = be.sample_lp(flat.astype(np.float32), u.astype(np.float32), d, bs.is_squashed(sp),
                                              np.float32)
        assert lp32.dtype == np.float32 and a32.dtype == np.float32
        # the sample itself is box_squash's, bit for bit
        fn = bs.squashed_sample if bs.is_squashed(sp) else ba.gaussian_sample
        ref_a, ref_se = fn(flat.astype(np.float32), u.astype(np.float32), d, np.float32)
        assert np.array_equal(a32, ref_a) and np.array_equal(_se, ref_se)


@pytest.mark.parametrize("dims,spaces,B,local_q,H", CASES, ids=IDS)
def test_critic_grads_match_autograd(dims, spaces, B, local_q, H):
    """the soft target: y = r + gamma (1 - done) (q' - alpha_i lp'_i), agent i's own entropy alone"""
    gamma = 0.95
    c, n, batch_n, params = _setup(dims, spaces, B, local_q, H, seed=111)
    lq = c["local_q"]
    alphas = _alphas(spaces)
    for i in range(n):
        u_tgt = np.asarray(c["u_tgt"][i], np.float64)
        with fp64_oracle():
            g, st, lp_t = be.critic_grads(_agents(params, lq), i, batch_n, u_tgt, spaces, alphas, gamma)
        obs_n = [torch.tensor(b[0], dtype=F64) for b in batch_n]
        act_n = [torch.tensor(b[1], dtype=F64) for b in batch_n]
        obs2_n = [torch.tensor(b[3], dtype=F64) for b in batch_n]
        rew, done = torch.tensor(batch_n[i][2], dtype=F64), torch.tensor(batch_n[i][4], dtype=F64)
        with torch.no_grad():
            heads = [_mlp(_t(params[j]["tgt_actor"]), obs2_n[j]) for j in range(n)]
            tgt_act = [_sample(spaces[j], heads[j], torch.tensor(u_tgt[j], dtype=F64)) for j in range(n)]
            qn = _mlp(_t(params[i]["tgt_critic"]), _cin(obs2_n, tgt_act, i, lq[i]))[:, 0]
            if alphas[i]:
                lp = _torch_lp(spaces[i], heads[i], torch.tensor(u_tgt[i], dtype=F64))
                qn = qn - alphas[i] * lp
                assert abs(lp_t - lp.mean().item()) <= 1e-12 * max(1.0, abs(lp_t))
            y = rew + gamma * (1.0 - done) * qn
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


@pytest.mark.parametrize("dims,spaces,B,local_q,H", CASES, ids=IDS)
def test_actor_grads_match_autograd(dims, spaces, B, local_q, H):
    """the gradient of alpha * mean(lp) - mean(Q) + the regulariser through the reparameterised sample"""
    reg = 1e-3
    c, n, batch_n, params = _setup(dims, spaces, B, local_q, H, seed=212)
    lq = c["local_q"]
    alphas = _alphas(spaces)
    for i in range(n):
        u_act = np.asarray(c["u_act"][i], np.float64)
        with fp64_oracle():
            g, p_loss, mean_lp = be.actor_grads(_agents(params, lq), i, batch_n, u_act, spaces, alphas, actor_reg=reg)
        obs_n = [torch.tensor(b[0], dtype=F64) for b in batch_n]
        act_n = [torch.tensor(b[1], dtype=F64) for b in batch_n]
        ap = _t(params[i]["actor"], grad=True)
        head = _mlp(ap, obs_n[i])
        ut = torch.tensor(u_act, dtype=F64)
        act_in = list(act_n)
        act_in[i] = _sample(spaces[i], head, ut)
        q = _mlp(_t(params[i]["critic"]), _cin(obs_n, act_in, i, lq[i]))[:, 0]
        loss = -torch.mean(q) + reg * torch.mean(head ** 2)
        if alphas[i]:
            lp = _torch_lp(spaces[i], head, ut)
            loss = loss + alphas[i] * torch.mean(lp)
            assert abs(mean_lp - lp.mean().item()) <= 1e-12 * max(1.0, abs(mean_lp))
        gt = dict(zip(ap, torch.autograd.grad(loss, list(ap.values()))))
        assert abs(p_loss - loss.item()) <= 1e-12 * abs(loss.item())
        for k in nets.NAMES:
            want = gt[k].numpy().reshape(np.shape(g[k]))
            np.testing.assert_allclose(g[k], want, rtol=1e-10, atol=1e-14 * max(1.0, np.abs(want).max()),
                                       err_msg=f"agent {i} actor {k}")


@pytest.mark.parametrize("dims,spaces,B,local_q,H", CASES, ids=IDS)
def test_zero_coefficient_is_the_squash_restatement_bit_for_bit(dims, spaces, B, local_q, H):
    c = bs.squash_case(dims, spaces, B, 4 * B, 303, local_q, H)
    n = len(dims)

    def agents():
        return [trainer.AgentParams(**{w: {k: v.copy() for k, v in p[w].items()} for w in p}, local_q=c["local_q"][j])
                for j, p in enumerate(c["params"])]
    A, Z = agents(), agents()
    for i in range(n):
        want, og = bs.update(A, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], spaces)
        got, gg, ent = be.update(Z, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], spaces, [0.0] * n)
        assert np.array_equal(np.asarray(want).view(np.uint64), np.asarray(got).view(np.uint64))
        assert ent["lp"] == 0.0 and ent["lp_t"] == 0.0
        for net in ("grad_critic", "grad_actor"):
            for k in og[net]:
                assert np.array_equal(og[net][k].view(np.uint32), gg[net][k].view(np.uint32)), (i, net, k)
        for w in ("actor", "critic", "tgt_actor", "tgt_critic"):
            for k, v in getattr(A[i], w).items():
                assert np.array_equal(v.view(np.uint32), getattr(Z[i], w)[k].view(np.uint32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2])
def test_edges(dtype, d):
    B = 4
    reg = 2e-3 / (B * 2 * d)
    ab = dtype(np.float32(0.2) / np.float32(B))
    da = np.full((B, d), -0.25, dtype)
    u0 = _u_for_eps0(B, 0)
    for z in (20.0, -20.0):
        # saturated: a = +-1 exactly where ln(1 - a^2) is -inf; lp finite, the entropy gradient exactly 2 a
        flat = np.concatenate([np.full((B, d), z), np.full((B, d), 0.1)], 1).astype(dtype)
        a, se, lp, zz, eps = be.sample_lp(flat, u0, d, True, dtype)
        assert a.dtype == dtype and np.array_equal(a, np.full((B, d), np.sign(z), dtype))
        assert np.isfinite(lp).all() and lp.dtype == dtype
        with np.errstate(divide="ignore"):
            assert np.isneginf(np.log(dtype(1) - a * a)).all()
        # ln(1 - tanh^2 20) = 2 (ln 2 - 20) to every digit: log1p(exp(-40)) is 4e-18
        want = d * (-0.1 - be.HALF_LN_2PI - 2.0 * (be.LN_2 - 20.0))
        assert np.abs(lp - want).max() <= 4 * np.finfo(dtype).eps * abs(want)
        g = be.entropy_bwd(flat, da, se, a, d, True, 0.0, ab, dtype)
        assert np.array_equal(g[:, :d], (ab * (dtype(2) * a)).astype(dtype))            # (alpha / B) * 2 a
        assert np.array_equal(g[:, :d] / ab, 2 * a)
        assert np.array_equal(g[:, d:], np.full((B, d), -ab, dtype))                    # se = 0: 2 a se - 1 = -1
        g = be.entropy_bwd(flat, da, se, a, d, True, reg, ab, dtype)
        assert np.isfinite(g).all()
    # z = 0: a = 0, lp is the plain Gaussian's at eps = 0, no mean gradient from the entropy
    flat = np.concatenate([np.zeros((B, d)), np.full((B, d), 0.3)], 1).astype(dtype)
    a, se, lp, zz, eps = be.sample_lp(flat, u0, d, True, dtype)
    assert np.array_equal(a, np.zeros((B, d), dtype)) and np.all(eps == 0)
    _a, _s, lp_plain, _z, _e = be.sample_lp(flat, u0, d, False, dtype)
    assert np.abs(lp - lp_plain).max() <= 8 * np.finfo(dtype).eps                       # 2 (ln 2 - log1p(1)) = 0
    assert np.abs(lp_plain - d * (-dtype(0.3) - be.HALF_LN_2PI)).max() <= 8 * np.finfo(dtype).eps
    g = be.entropy_bwd(flat, da, se, a, d, True, reg, ab, dtype)
    base = bs.squashed_bwd(flat, da, se, a, d, reg, dtype)
    assert np.array_equal(g[:, :d], base[:, :d]) and np.array_equal(g[:, d:], (base[:, d:] + (-ab)).astype(dtype))
    # the plain form: dmean gains nothing, dlogstd gains -alpha / B
    g = be.entropy_bwd(flat, da, se, a, d, False, reg, ab, dtype)
    base = ba.gaussian_bwd(flat, da, se, d, reg, dtype)
    assert np.array_equal(g[:, :d], base[:, :d]) and np.array_equal(g[:, d:], (base[:, d:] + (-ab)).astype(dtype))
    # logstd = -100: std underflows, lp = 100 d + ... stays finite
    u = _u_for_eps0(B, 1.5)
    flat = np.concatenate([np.full((B, d), 0.4), np.full((B, d), -100.0)], 1).astype(dtype)
    for squash in (False, True):
        a, se, lp, zz, eps = be.sample_lp(flat, u, d, squash, dtype)
        assert np.isfinite(lp).all() and (lp > 90 * d).all() and np.abs(se).max() < 1e-40
        assert np.isfinite(be.entropy_bwd(flat, da, se, a, d, squash, reg, ab, dtype)).all()
    # u0 = 0: eps = 0 whatever std is
    flat = np.concatenate([np.full((B, d), -0.7), np.full((B, d), 3.0)], 1).astype(dtype)
    a, se, lp, zz, eps = be.sample_lp(flat, u0, d, True, dtype)
    assert np.all(eps == 0) and np.all(se == 0) and np.isfinite(lp).all()
    # NaN in u[2..4] changes no bit
    rng = np.random.default_rng(5)
    v = rng.uniform(0, 1, (64, 5)).astype(np.float32)
    w = v.copy()
    w[:, 2:] = np.nan
    flat = rng.normal(size=(64, 2 * d)).astype(dtype)
    for squash in (False, True):
        for x, y in zip(be.sample_lp(flat, v, d, squash, dtype), be.sample_lp(flat, w, d, squash, dtype)):
            assert np.array_equal(x, y) and np.isfinite(x).all()


@pytest.mark.parametrize("d", [1, 2])
def test_plain_gaussian_entropy_by_monte_carlo(d):
    """mean(-lp) over N samples of Philox-derived normals (the device's uniforms5 and
    Box-Muller) = d * 0.5 ln(2 pi e) + sum logstd within 4 standard errors: -lp = sum_k
    (0.5 eps_k^2 + logstd_k + 0.5 ln 2 pi), the variance of 0.5 eps^2 is 0.5 per
    dimension, so the standard error is sqrt(0.5 d / N)"""
    N = 10 ** 6
    logstd = np.array([-0.3, 0.4][:d], np.float32)
    u = philox.uniforms5(0x9E3779B97F4A7C15, 0x8001, 3, np.arange(N))
    flat = np.concatenate([np.zeros((N, d), np.float32), np.tile(logstd, (N, 1))], 1)
    _a, _se, lp, _z, eps = be.sample_lp(flat, u, d, False, np.float32)
    got = float(np.mean(-lp.astype(np.float64)))
    want = d * 0.5 * np.log(2 * np.pi * np.e) + float(logstd.astype(np.float64).sum())
    se = np.sqrt(0.5 * d / N)
    print(f"d = {d}: mean -lp {got:.6f}, closed form {want:.6f}, difference {(got - want) / se:+.2f} standard errors")
    assert abs(got - want) <= 4 * se


# ------------------------------------------------------------------- CLI
def _args(**kw):
    base = dict(continuous_actions=True, action_squash="tanh", entropy_alpha=0.2, prioritized_replay=False, td3=False,
                minimax=False, approx_policies=False, update_mode="strict", num_gpus=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_entropy_alpha_flag_refusals():
    from experiments.train import continuous_flags, parse_args
    continuous_flags(_args())                                          # passes
    continuous_flags(_args(action_squash="none"))                      # a plain Gaussian may carry it too
    continuous_flags(_args(continuous_actions=False, action_squash="none", entropy_alpha=0.0))
    with pytest.raises(SystemExit, match="--entropy-alpha needs --continuous-actions"):
        continuous_flags(_args(continuous_actions=False, action_squash="none"))
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(SystemExit, match="--entropy-alpha must be finite and >= 0"):
            continuous_flags(_args(entropy_alpha=bad))
    # a handle with a coefficient is a Box handle: --continuous-actions' own refusals hold
    for kw, msg in ((dict(prioritized_replay=True), "--prioritized-replay"), (dict(td3=True), "--td3"),
                    (dict(update_mode="throughput"), "--update-mode strict"), (dict(num_gpus=2), "one GPU")):
        with pytest.raises(SystemExit, match=msg):
            continuous_flags(_args(**kw))
    a = parse_args(["--scenario", "simple_spread", "--continuous-actions", "--entropy-alpha", "0.05"])
    assert a.entropy_alpha == 0.05 and parse_args([]).entropy_alpha == 0.0


def test_runner_and_facade_settings_are_checked_before_a_device_is_needed():
    from maddpg_amd.common import tf_util as U
    from maddpg_amd.envs import Box, Discrete
    from maddpg_amd.runner import VecRunner
    from maddpg_amd.trainer.maddpg import MADDPGAgentTrainer
    with pytest.raises(ValueError, match="--entropy-alpha needs --continuous-actions"):
        VecRunner("simple_spread", 4, entropy_alpha=0.2)
    with pytest.raises(ValueError, match="--entropy-alpha must be finite"):
        VecRunner("simple_spread", 4, continuous=True, entropy_alpha=-1.0)
    base = dict(lr=1e-2, gamma=0.95, batch_size=64, num_units=64, max_episode_len=5)
    with U.single_threaded_session():
        t = MADDPGAgentTrainer("a", None, [(18,)] * 2, [Box(2), Discrete(5)], 0,
                               argparse.Namespace(entropy_alpha=0.2, **base))
        assert t.act_entropy == [0.2, 0.0] and t.act_squash == ["none", "none"]
    with U.single_threaded_session():
        t = MADDPGAgentTrainer("a", None, [(18,)] * 2, [Box(2), Discrete(5)], 0, argparse.Namespace(**base))
        assert t.act_entropy == [0.0, 0.0]
        with pytest.raises(ValueError, match="entropy_alpha"):
            MADDPGAgentTrainer("b", None, [(18,)] * 2, [Box(2), Discrete(5)], 1,
                               argparse.Namespace(entropy_alpha=-0.5, **base))
