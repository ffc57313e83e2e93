"""CPU: the mixed-width restatement (tests/mixed_width.py) against torch.autograd
in float64, in the style of tests/test_oracle_autograd.py, and the host-side
width plumbing that needs no GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import nets, trainer  # noqa: E402
from tests import mixed_width as mw  # noqa: E402
from tests.test_oracle_autograd import F64, _cin, _gsm, _mlp, _t, fp64_oracle  # noqa: E402

CASES = [([3, 11], [3, 5], 24, 64, None), ([11, 3], [5, 3], 24, 64, None), ([6, 6, 6], [4, 4, 4], 16, 64, None),
         ([3, 11], [3, 5], 24, 64, [True, False]), ([5, 7, 4], [1, 2, 5], 16, 128, [False, True, False])]


def _case(dims, widths, B, H, local_q, seed):
    c = mw.mixed_case(dims, widths, B, 4 * B, seed, local_q, H)
    idx = c["idx"][0]
    batch_n = [tuple(np.asarray(x[idx], np.float64) for x in c["data"][j]) for j in range(len(dims))]
    params = [{w: {k: np.asarray(v, np.float64) for k, v in p[w].items()} for w in p} for p in c["params"]]
    return c, batch_n, params


@pytest.mark.parametrize("dims,widths,B,H,local_q", CASES)
def test_mixed_width_actor_grads_match_autograd(dims, widths, B, H, local_q):
    reg = 1e-3
    c, batch_n, params = _case(dims, widths, B, H, local_q, seed=303)
    lq, n = c["local_q"], len(dims)
    for i in range(n):
        u_act = np.asarray(c["u_act"][i], np.float64)
        with fp64_oracle():
            agents = [trainer.AgentParams(**{w: dict(p[w]) for w in p}, local_q=lq[j]) for j, p in enumerate(params)]
            g, p_loss = mw.actor_grads(agents, i, batch_n, u_act, actor_reg=reg)
        obs_n = [torch.tensor(b[0], dtype=F64) for b in batch_n]
        act_n = [torch.tensor(b[1], dtype=F64) for b in batch_n]
        assert [a.shape[1] for a in act_n] == widths
        ap = _t(params[i]["actor"], grad=True)
        logits = _mlp(ap, obs_n[i])
        assert logits.shape[1] == widths[i]
        act_in = list(act_n)
        act_in[i] = _gsm(logits, torch.tensor(u_act[:, :widths[i]], dtype=F64))
        q = _mlp(_t(params[i]["critic"]), _cin(obs_n, act_in, i, lq[i]))[:, 0]
        loss = -torch.mean(q) + reg * torch.mean(logits ** 2)
        gt = dict(zip(ap, torch.autograd.grad(loss, list(ap.values()))))
        assert abs(p_loss - loss.item()) <= 1e-12 * abs(loss.item())
        for k in nets.NAMES:
            want = gt[k].numpy().reshape(np.shape(g[k]))
            np.testing.assert_allclose(g[k], want, rtol=1e-10, atol=1e-14 * max(1.0, np.abs(want).max()),
                                       err_msg=f"agent {i} actor {k}")


@pytest.mark.parametrize("dims,widths,B,H,local_q", CASES[:2])
def test_mixed_width_critic_grads_match_autograd(dims, widths, B, H, local_q):
    """oracle.trainer.critic_grads is width-agnostic: fed A_j-wide uniforms it is the
    reference's critic step on Discrete(A_j) agents"""
    gamma = 0.95
    c, batch_n, params = _case(dims, widths, B, H, local_q, seed=404)
    lq, n = c["local_q"], len(dims)
    for i in range(n):
        u_tgt = mw.narrow(np.asarray(c["u_tgt"][i], np.float64), widths)
        with fp64_oracle():
            agents = [trainer.AgentParams(**{w: dict(p[w]) for w in p}, local_q=lq[j]) for j, p in enumerate(params)]
            g, st = trainer.critic_grads(agents, i, batch_n, u_tgt, gamma)
        obs_n = [torch.tensor(b[0], dtype=F64) for b in batch_n]
        act_n = [torch.tensor(b[1], dtype=F64) for b in batch_n]
        obs2_n = [torch.tensor(b[3], dtype=F64) for b in batch_n]
        rew, done = torch.tensor(batch_n[i][2], dtype=F64), torch.tensor(batch_n[i][4], dtype=F64)
        with torch.no_grad():
            tgt_act = [_gsm(_mlp(_t(params[j]["tgt_actor"]), obs2_n[j]), torch.tensor(u_tgt[j], dtype=F64))
                       for j in range(n)]
            y = rew + gamma * (1.0 - done) * _mlp(_t(params[i]["tgt_critic"]), _cin(obs2_n, tgt_act, i, lq[i]))[:, 0]
        cp = _t(params[i]["critic"], grad=True)
        loss = torch.mean((_mlp(cp, _cin(obs_n, act_n, i, lq[i]))[:, 0] - y) ** 2)
        gt = dict(zip(cp, torch.autograd.grad(loss, list(cp.values()))))
        assert abs(st["q_loss"] - loss.item()) <= 1e-12 * abs(loss.item())
        for k in nets.NAMES:
            want = gt[k].numpy().reshape(np.shape(g[k]))
            np.testing.assert_allclose(g[k], want, rtol=1e-10, atol=1e-14 * max(1.0, np.abs(want).max()))


def test_wrong_slice_offset_would_be_caught():
    """the uniform-width offset A * i of oracle/trainer.py is a different slice when widths differ"""
    c, batch_n, params = _case([11, 3], [5, 3], 24, 64, None, seed=505)
    with fp64_oracle():
        agents = [trainer.AgentParams(**{w: dict(p[w]) for w in p}) for p in params]
        good, _ = mw.actor_grads(agents, 1, batch_n, np.asarray(c["u_act"][1], np.float64))
        bad, _ = trainer.actor_grads(agents, 1, batch_n, np.asarray(c["u_act"][1], np.float64)[:, :3])
    assert np.abs(good["W3"] - bad["W3"]).max() > 1e-6


def test_joint_rows_keep_pad_entries_zero():
    c = mw.mixed_case([3, 11], [3, 5], 8, 32, seed=1)
    rows = mw.joint_rows_w(c["data"], c["dims"])
    S = 14
    assert rows.shape[1] == (2 * S + 7 * 2 + 3) // 4 * 4
    assert (rows[:, S + 3:S + 5] == 0).all() and np.allclose(rows[:, S:S + 3].sum(1), 1, atol=1e-6)
    assert np.allclose(rows[:, S + 5:S + 10].sum(1), 1, atol=1e-6)


def test_scenario_spec_and_facade_widths():
    from maddpg_amd.envs import Discrete, ScenarioSpec, spec
    sp = spec("simple_spread")
    assert sp.act_dims == [5, 5, 5] and [a.n for a in sp.action_space] == [5, 5, 5]
    sp = ScenarioSpec("x", 2, 0, [3, 11], [3, 5])
    assert [a.n for a in sp.action_space] == [3, 5]
    from types import SimpleNamespace
    from maddpg_amd.common import tf_util as U
    from maddpg_amd.trainer.maddpg import MADDPGAgentTrainer
    args = SimpleNamespace(num_units=64, batch_size=8, max_episode_len=25, lr=1e-2, gamma=0.95)
    with_session = U.Session()
    U._DEFAULT, prev = with_session, U._DEFAULT
    try:
        t = MADDPGAgentTrainer("agent_0", None, [(3,), (11,)], [Discrete(3), Discrete(5)], 0, args)
        assert t.act_dims == [3, 5]
        for bad in (Discrete(6), Discrete(0), SimpleNamespace(n=[3, 3])):
            with pytest.raises(NotImplementedError):
                MADDPGAgentTrainer("agent_1", None, [(3,), (11,)], [Discrete(3), bad], 1, args)
    finally:
        U._DEFAULT = prev
