"""CPU tests of MADDPG with inferred policies: the numpy oracle
(tests/approx_oracle.py) against a float64 autograd derivation, its reduction to
MADDPG, the frozen-policy fit, the CLI's refusals and the library's new entry points.
"""
import argparse
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import nets, trainer
from tests import approx_oracle as ao
from tests import mixed_width
from tests.helpers import synthetic_trainer_case

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd(phi, obs, act, lam):
    """loss and gradients of the approximator loss in float64 by torch.autograd,
    written from the definition: log-probability of the relaxed sample = cross-entropy"""
    P = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in phi.items()}
    x, a = torch.tensor(obs.astype(np.float64)), torch.tensor(act.astype(np.float64))
    h1 = torch.relu(x @ P["W1"] + P["b1"])
    h2 = torch.relu(h1 @ P["W2"] + P["b2"])
    logits = h2 @ P["W3"] + P["b3"]
    logits.retain_grad()
    lp = torch.log_softmax(logits, -1)
    ce = -(a * lp).sum(-1)
    ent = -(lp.exp() * lp).sum(-1)
    loss = (ce - lam * ent).mean()
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in P.items()}
    return float(loss.detach()), grads, logits.grad.numpy(), float(ce.mean().detach()), float(ent.mean().detach())


@pytest.mark.parametrize("lam", [1e-3, 0.0])
@pytest.mark.parametrize("A", [5, 3])
def test_loss_and_gradient_against_float64_autograd(A, lam):
    rng = np.random.default_rng(3 + A)
    B, o, H = 40, 6, 64
    phi = nets.xavier_init(rng, o, A, H)
    phi = {k: (v * np.float32(2)).astype(np.float32) for k, v in phi.items()}
    obs = rng.normal(size=(B, o)).astype(np.float32)
    act = rng.dirichlet(np.ones(A) * 0.3, size=B).astype(np.float32)       # points of the simplex, some near a vertex
    g, st = ao.approx_grads(phi, obs, act, lam)
    loss, g64, seed64, ce64, ent64 = _autograd(phi, obs, act, lam)
    # the seed is a handful of fp32 roundings (6e-8 each) on values no larger than its scale
    logits = nets.mlp_fwd(phi, obs)[0]
    seed = ao.head(logits, act, lam, B)[2]
    s = float(np.abs(seed64).max())
    print(f"A={A} lambda={lam}: seed error / scale {np.abs(seed - seed64).max() / s:.2e}")
    assert np.abs(seed - seed64).max() / s < 2e-6
    for k in g:                                                             # the repository's raw-gradient tolerance
        scale = float(np.abs(g64[k]).max()) or 1.0
        err = float(np.abs(g[k].astype(np.float64) - g64[k].reshape(g[k].shape)).max()) / scale
        assert err < 1e-5, (k, err)
    assert abs(st["loss"] - loss) < 1e-5 * abs(loss) + 1e-7
    assert abs(st["cross_entropy"] - ce64) < 1e-5 * abs(ce64) + 1e-7
    assert abs(st["entropy"] - ent64) < 1e-5 * abs(ent64) + 1e-7


def test_vanished_probability_gives_finite_terms_and_exact_zero_pads():
    """a logit 200 below the max: p underflows to 0, log p stays finite (log-softmax);
    a replayed action with exact-zero entries gives exact-zero cross-entropy terms there"""
    logits = np.array([[0.0, -200.0, 1.0, 0.5, -3.0]], np.float32)
    act = np.array([[0.25, 0.0, 0.5, 0.25, 0.0]], np.float32)
    ce, en, seed = ao.head(logits, act, 1e-3, 1)
    assert np.isfinite(ce).all() and np.isfinite(en).all() and np.isfinite(seed).all()
    assert seed[0, 1] == 0.0


def _agents(c, approx):
    ags = [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][j]) for j, p in enumerate(c["params"])]
    return ao.add_approx(ags, copy.deepcopy(approx))


def test_target_actor_bits_reduce_the_critic_step_to_maddpg():
    dims, B, L = [6, 5, 4], 40, 200
    c = synthetic_trainer_case(dims, B, L, seed=21)
    approx = ao.approx_case(c, dims, 21)
    for i in range(3):
        for j in approx[i]:
            approx[i][j]["tgt"] = copy.deepcopy(c["params"][j]["tgt_actor"])
    ags = _agents(c, approx)
    plain = [trainer.AgentParams(**copy.deepcopy(p)) for p in c["params"]]
    other = _agents(c, ao.approx_case(c, dims, 21))                     # targets that differ
    for i in range(3):
        batch_n = [tuple(x[c["idx"][i]] for x in c["data"][j]) for j in range(3)]
        g, st = ao.critic_grads(ags, i, batch_n, c["u_tgt"][i])
        g0, st0 = trainer.critic_grads(plain, i, batch_n, c["u_tgt"][i])
        assert all(np.array_equal(g[k], g0[k]) for k in g)
        assert st["q_loss"] == st0["q_loss"] and np.array_equal(st["target_q"], st0["target_q"])
        g1, _ = ao.critic_grads(other, i, batch_n, c["u_tgt"][i])
        assert not all(np.array_equal(g1[k], g0[k]) for k in g)


def test_ddpg_critic_agent_is_untouched():
    dims, B, L = [6, 5, 4], 40, 200
    lq = [True, False, False]
    c = synthetic_trainer_case(dims, B, L, seed=22, local_q=lq)
    ags = _agents(c, ao.approx_case(c, dims, 22))
    plain = [trainer.AgentParams(**copy.deepcopy(p), local_q=lq[j]) for j, p in enumerate(c["params"])]
    assert ags[0].approx == {} and sorted(ags[1].approx) == [0, 2]
    want, _ = mixed_width.update(plain, 0, c["data"], c["idx"][0], c["u_tgt"][0], c["u_act"][0], [5] * 3)
    got, ex = ao.update(ags, 0, c["data"], c["idx"][0], c["u_tgt"][0], c["u_act"][0], [5] * 3)
    assert got == want and ex["approx"] == {}
    for w in ("actor", "critic", "tgt_actor", "tgt_critic"):
        assert all(np.array_equal(getattr(ags[0], w)[k], getattr(plain[0], w)[k]) for k in nets.NAMES)


def test_frozen_policy_fit_quarters_the_kl():
    """100 approximator steps on actions sampled from fixed, far-from-uniform
    policies: the mean KL(true || approximator) over the ring falls below a quarter
    of its starting value"""
    res = ao.fit_run(ao.fit_case())
    for j, (kl0, kl1) in res.items():
        print(f"approximator of agent {j}: mean KL {kl0:.3f} -> {kl1:.3f} in {ao.FIT_STEPS} steps")
        assert kl0 > 0.2, (j, kl0)                      # the policies are far from the untrained approximator
        assert kl1 < 0.25 * kl0, (j, kl0, kl1)


def _cli_args(**kw):
    base = dict(approx_policies=True, approx_lambda=1e-3, prioritized_replay=False, td3=False, minimax=False,
                update_mode="strict", num_gpus=None, save_format="npz")
    base.update(kw)
    return argparse.Namespace(**base)


def test_approx_flags_refuse_each_combination():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mdp_train_cli", os.path.join(ROOT, "experiments", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    train.approx_flags(_cli_args())                                      # accepted
    train.approx_flags(_cli_args(approx_lambda=0.0))
    train.approx_flags(_cli_args(approx_policies=False, td3=True))       # not asked for: nothing to refuse
    for bad in (dict(prioritized_replay=True), dict(td3=True), dict(minimax=True), dict(update_mode="throughput"),
                dict(num_gpus=2), dict(save_format="tf1"), dict(approx_lambda=-1.0), dict(approx_lambda=float("nan"))):
        with pytest.raises(SystemExit):
            train.approx_flags(_cli_args(**bad))
    a = train.parse_args(["--approx-policies", "--approx-lambda", "0.01"])
    assert a.approx_policies and a.approx_lambda == 0.01
    assert not train.parse_args([]).approx_policies


NEW = ("mdp_approx_bytes", "mdp_approx_enable", "mdp_approx_set_params", "mdp_approx_get_params",
       "mdp_approx_get_beta_powers", "mdp_approx_set_beta_powers", "mdp_approx_info", "mdp_approx_logits",
       "mdp_approx_grad", "mdp_approx_step")


def _cfg(n=3, H=64, B=1024, obs=6):
    from maddpg_amd._lib import MdpConfig
    cfg = MdpConfig()
    cfg.n_agents = n
    for i in range(n):
        cfg.obs_dim[i] = obs
    cfg.act_dim, cfg.num_units, cfg.batch_size, cfg.max_episode_len = 5, H, B, 25
    cfg.capacity, cfg.world_size = 4096, 1
    cfg.lr, cfg.tau, cfg.grad_clip, cfg.actor_reg = 1e-2, 1e-2, 0.5, 1e-3
    cfg.adam_b1, cfg.adam_b2, cfg.adam_eps, cfg.gamma = 0.9, 0.999, 1e-8, 0.95
    return cfg


def test_library_exports_the_approx_entry_points_and_refuses_null():
    from maddpg_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols(), name
    assert lib.mdp_abi_version() == _lib.ABI_VERSION == 5
    assert re.search(r"MDP_K_COUNT = 13\b", open(_lib.HEADER).read())
    f2, d4, f8 = (ctypes.c_float * 2)(), (ctypes.c_double * 4)(), (ctypes.c_float * 8)()
    assert lib.mdp_approx_bytes(None) < 0
    assert lib.mdp_approx_enable(None, None, 0, 1e-3) < 0
    assert lib.mdp_approx_set_params(None, 0, 1, 0, f8, 8) < 0
    assert lib.mdp_approx_get_params(None, 0, 1, 0, f8, 8) < 0
    assert lib.mdp_approx_get_beta_powers(None, 0, 1, f2) < 0
    assert lib.mdp_approx_set_beta_powers(None, 0, 1, f2) < 0
    assert lib.mdp_approx_info(None, 0, 1, d4) < 0
    assert lib.mdp_approx_logits(None, 0, 1, 0, None, None, 4) < 0
    assert lib.mdp_approx_grad(None, 0, None) < 0
    assert lib.mdp_approx_step(None, 0, None) < 0


def test_every_approx_entry_point_refuses_a_failed_handle():
    """mdp_create on a 16-byte host arena fails and still returns a handle (it
    carries the message): no entry point may look into it"""
    from maddpg_amd import _lib
    lib = _lib.load()
    f2, d4, f8 = (ctypes.c_float * 2)(), (ctypes.c_double * 4)(), (ctypes.c_float * 8)()
    h, arena = ctypes.c_void_p(), ctypes.create_string_buffer(16)
    assert lib.mdp_create(None, ctypes.cast(arena, ctypes.c_void_p), 16, None, ctypes.byref(h)) < 0
    assert h.value
    try:
        assert lib.mdp_approx_enable(h, ctypes.cast(arena, ctypes.c_void_p), 16, 1e-3) < 0
        assert lib.mdp_approx_enable(h, None, 0, 1e-3) < 0
        assert lib.mdp_approx_set_params(h, 0, 1, 0, f8, 8) < 0
        assert lib.mdp_approx_get_params(h, 0, 1, 0, f8, 8) < 0
        assert lib.mdp_approx_get_beta_powers(h, 0, 1, f2) < 0
        assert lib.mdp_approx_set_beta_powers(h, 0, 1, f2) < 0
        assert lib.mdp_approx_info(h, 0, 1, d4) < 0
        assert lib.mdp_approx_logits(h, 0, 1, 0, None, None, 4) < 0
        assert lib.mdp_approx_grad(h, 0, None) < 0
        assert lib.mdp_approx_step(h, 0, None) < 0
        assert list(d4) == [0.0] * 4 and list(f2) == [0.0] * 2 and list(f8) == [0.0] * 8   # nothing was written
    finally:
        assert lib.mdp_destroy(h) == 0


def test_approx_bytes_grows_with_agents_and_width():
    from maddpg_amd import _lib
    lib = _lib.load()
    size = lambda **kw: lib.mdp_approx_bytes(ctypes.byref(_cfg(**kw)))   # noqa: E731
    base = size()
    assert base > 0
    assert size(n=4) > base and size(n=6) > size(n=4)
    assert size(H=128) > base and size(H=256) > size(H=128)
    bad = _cfg()
    bad.n_agents = 0
    assert lib.mdp_approx_bytes(ctypes.byref(bad)) < 0
    bad = _cfg()
    bad.obs_dim[1] = 0
    assert lib.mdp_approx_bytes(ctypes.byref(bad)) < 0
