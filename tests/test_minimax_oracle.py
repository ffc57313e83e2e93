"""CPU tests of the M3DDPG oracle (tests/minimax_oracle.py) and of the
host surface of mdp_minimax_enable.  The GPU tests (tests/test_minimax_gpu.py) check
the device against the fp32 restatement; here the restatement itself is checked:
against oracle.trainer at eps = 0, against a torch.autograd float64 derivation,
and against a wrong sign of the perturbation."""
import copy
import ctypes

import numpy as np
import pytest

from oracle import nets, trainer
from tests import minimax_cases as mc
from tests import minimax_oracle as mo
from tests import mixed_width

F32, F64 = np.float32, np.float64


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ["spread", "adversary", "speaker_listener"])
def test_eps_zero_is_the_trainer_oracle_exactly(name):
    c = mc.make_case(name, "zero")
    n = len(c["params"])
    a, b = mc.oracle_agents(c), mc.oracle_agents(c)
    for r in range(2):
        for i in range(n):
            got, gx = mc.oracle_update(a, c, i)
            want, wx = mixed_width.update(b, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], c["widths"])
            assert [type(x) for x in got] == [type(x) for x in want]
            assert got == want, (r, i)
            assert _same(gx["grad_critic"], wx["grad_critic"]) and _same(gx["grad_actor"], wx["grad_actor"])
            for w in mc.NETS4:
                assert _same(getattr(a[i], w), getattr(b[i], w)), (r, i, w)
            assert _same(a[i].opt_actor.m, b[i].opt_actor.m) and _same(a[i].opt_critic.v, b[i].opt_critic.v)
    if name == "spread":    # the all-5 oracle itself
        d = mc.oracle_agents(c)
        e = mc.oracle_agents(c)
        got, _ = mc.oracle_update(d, c, 0)
        want, _ = trainer.update(e, 0, c["data"], c["idx"][0], c["u_tgt"][0], c["u_act"][0])
        assert got == want and _same(d[0].actor, e[0].actor) and _same(d[0].tgt_critic, e[0].tgt_critic)


def _rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("kind", mc.EPS)
@pytest.mark.parametrize("name", ["spread", "tag", "speaker_listener", "adversary"])
def test_float64_restatement_matches_autograd(name, kind):
    """the hand-written perturbation, both losses and every gradient against
    torch.autograd in float64 (1e-10 relative to each tensor's largest entry)"""
    pytest.importorskip("torch")
    c = mc.make_case(name, kind)
    ags = mc.oracle_agents(c)
    for i in range(len(ags)):
        bn = mc.batches(c, i)
        u_t = mixed_width.narrow(c["u_tgt"][i], c["widths"])
        gq, st = mo.critic_grads(ags, i, bn, u_t, c["eps"][i], dt=F64)
        gp, p_loss, ex = mo.actor_grads(ags, i, bn, c["u_act"][i], c["eps"][i], dt=F64)
        t = mo.torch_step(ags, i, bn, u_t, c["u_act"][i], c["eps"][i])
        assert abs(st["q_loss"] - t["q_loss"]) <= 1e-10 * abs(t["q_loss"])
        assert abs(p_loss - t["p_loss"]) <= 1e-10 * abs(t["p_loss"])
        assert _rel(st["target_q_next"], t["target_q_next"]) < 1e-10
        for k in nets.NAMES:
            assert _rel(gq[k].reshape(t["grad_critic"][k].shape), t["grad_critic"][k]) < 1e-10, (i, k)
            assert _rel(gp[k].reshape(t["grad_actor"][k].shape), t["grad_actor"][k]) < 1e-10, (i, k)
        if not ags[i].local_q:
            S = sum(c["params"][j]["actor"]["W1"].shape[0] for j in range(len(ags)))
            assert _rel(np.concatenate(st["adv"], 1), t["adv_critic"][:, S:]) < 1e-10
            assert _rel(np.concatenate(ex["adv"], 1), t["adv_actor"][:, S:]) < 1e-10


def test_stop_gradient_is_not_observable_with_relu_critics():
    """The perturbation is a constant of the actor step's backward.  Its direction
    ghat is W1^T diag(h1 > 0) W2^T diag(h2 > 0) W3, normalised: piecewise CONSTANT in
    the critic's input, so differentiating through it adds exactly nothing wherever
    no ReLU input is zero -- the detached and the non-detached actor gradients are
    the same tensor (autograd, float64, eps = 0.3).  Stated here because the
    opposite was expected when the feature was specified; what makes a wrong
    treatment of the perturbation visible is its sign and size (next test)."""
    pytest.importorskip("torch")
    c = mc.make_case("spread", "large")
    ags = mc.oracle_agents(c)
    bn = mc.batches(c, 1)
    u_t = mixed_width.narrow(c["u_tgt"][1], c["widths"])
    det = mo.torch_step(ags, 1, bn, u_t, c["u_act"][1], c["eps"][1], detach=True)
    live = mo.torch_step(ags, 1, bn, u_t, c["u_act"][1], c["eps"][1], detach=False)
    for k in nets.NAMES:
        assert _rel(live["grad_actor"][k], det["grad_actor"][k]) < 1e-12, k


@pytest.mark.parametrize("name", ["spread", "tag"])
def test_a_flipped_sign_is_far_outside_the_gpu_tolerances(name):
    """eps = 0.3: the update with a^ = a + eps ghat against the right one, in units of the
    GPU parity tolerances (stats 2e-5 relative, gradients 1e-5 of the largest entry)"""
    c = mc.make_case(name, "large")
    for i in range(len(c["params"])):
        good, gx = mc.oracle_update(mc.oracle_agents(c), c, i)
        bad, bx = mc.oracle_update(mc.oracle_agents(c), c, i, sign=-1)
        assert abs(bad[4] - good[4]) > 100 * 2e-5 * abs(good[4]), (i, good[4], bad[4])     # mean q'
        assert abs(bad[1] - good[1]) > 100 * 2e-5 * abs(good[1]), (i, good[1], bad[1])     # p_loss
        for w in ("grad_critic", "grad_actor"):
            worst = max(_rel(bx[w][k], gx[w][k]) for k in ("W1", "W2", "W3"))
            assert worst > 100 * 1e-5, (i, w, worst)
        assert good[4] < bad[4]      # the right sign lowers this agent's Q'


@pytest.mark.parametrize("kind", mc.EPS)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_fixture_rows_are_well_conditioned(name, kind):
    """the GPU tests' seeds: in the float64 oracle at most 5 % of a batch's rows have a
    perturbed agent's ss below 1e-6 of the batch median (those rows may be left out
    of the a^ comparison there)"""
    c = mc.make_case(name, kind)
    ags = mc.oracle_agents(c)
    for i in range(len(ags)):
        if ags[i].local_q:
            continue
        bn = mc.batches(c, i)
        _, st = mo.critic_grads(ags, i, bn, mixed_width.narrow(c["u_tgt"][i], c["widths"]), c["eps"][i], dt=F64)
        _, _, ex = mo.actor_grads(ags, i, bn, c["u_act"][i], c["eps"][i], dt=F64)
        for ss in (st["ss"], ex["ss"]):
            assert mo.ill_conditioned(ss).mean() <= 0.05, (name, i)


def test_eps_matrix_follows_the_sides():
    from maddpg_amd.envs import minimax_eps
    e = minimax_eps(4, 3, 1e-3, 1e-5)
    assert e.dtype == np.float32 and not e.diagonal().any()
    assert e[0, 3] == e[3, 1] == F32(1e-3) and e[0, 1] == e[2, 0] == F32(1e-5)
    assert np.array_equal(minimax_eps(3, 0, 1e-3, 1e-5), F32(1e-5) * (1 - np.eye(3, dtype=F32)))


# ---- host surface
def test_library_exports_minimax_entry_points_and_refuses_null():
    from maddpg_amd import _lib
    lib = _lib.load()
    for name in ("mdp_minimax_enable", "mdp_minimax_info", "mdp_minimax_debug_adv"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols(), name
    eps = np.zeros((3, 3), np.float32)
    assert lib.mdp_minimax_enable(None, _lib.fptr(eps)) < 0
    assert lib.mdp_minimax_info(None, _lib.fptr(eps)) < 0
    assert lib.mdp_minimax_debug_adv(None, None, None) < 0
    # a handle whose create failed (no arena) is refused as a NULL one
    from tests.test_host_logic import _cfg
    h = ctypes.c_void_p()
    assert lib.mdp_create(ctypes.byref(_cfg()), None, 0, None, ctypes.byref(h)) != 0 and h.value
    assert lib.mdp_minimax_enable(h, _lib.fptr(eps)) < 0 and lib.mdp_minimax_info(h, _lib.fptr(eps)) < 0
    assert lib.mdp_minimax_debug_adv(h, None, None) < 0
    lib.mdp_destroy(h)
    assert lib.mdp_abi_version() == _lib.ABI_VERSION == 5


def test_cli_defaults_and_refusals():
    from experiments.train import minimax_flags, parse_args
    from maddpg_amd.common.tf_util import minimax_kwargs
    a = parse_args([])
    assert a.minimax is False and a.adv_eps == 1e-3 and a.adv_eps_s == 1e-5
    minimax_flags(a)                           # off: nothing to refuse
    assert minimax_kwargs(a) == {}
    for extra in (["--td3"], ["--prioritized-replay"], ["--update-mode", "throughput"], ["--num-gpus", "2"],
                  ["--adv-eps", "-1"], ["--adv-eps-s", "nan"], ["--adv-eps", "inf"]):
        with pytest.raises(SystemExit):
            minimax_flags(parse_args(["--minimax"] + extra))
    b = parse_args(["--minimax", "--adv-eps", "0.01", "--adv-eps-s", "0"])
    minimax_flags(b)
    assert minimax_kwargs(b) == dict(minimax=True, adv_eps=0.01, adv_eps_s=0.0)
