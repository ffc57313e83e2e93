"""CPU tests of the MATD3 restatement (tests/td3_oracle.py) and of the host surface of
mdp_td3_enable: the degenerate case equals the MADDPG oracle bit for bit, the
delay leaves the actor and the targets alone, and both critics' gradients agree
with a torch.autograd derivation in float64."""
import copy
import ctypes

import numpy as np
import pytest

from oracle import nets, trainer
from tests import td3_oracle
from tests.helpers import synthetic_trainer_case

torch = pytest.importorskip("torch")

DIMS, B, L = [6, 5, 4], 40, 200


def _agents(c, twins, lq=None):
    n = len(c["params"])
    lq = c["local_q"] if lq is None else lq
    ags = [trainer.AgentParams(**copy.deepcopy(p), local_q=lq[j]) for j, p in enumerate(c["params"])]
    for j in range(n):
        td3_oracle.add_twin(ags[j], copy.deepcopy(twins[j]["critic2"]), copy.deepcopy(twins[j]["tgt_critic2"]))
    return ags


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in nets.NAMES)


def test_degenerate_td3_equals_maddpg_bit_for_bit():
    c = synthetic_trainer_case(DIMS, B, L, seed=3)
    n = len(DIMS)
    ref = [trainer.AgentParams(**copy.deepcopy(p)) for p in c["params"]]
    twins = [dict(critic2=p["critic"], tgt_critic2=p["tgt_critic"]) for p in c["params"]]
    td3 = _agents(c, twins)
    for rnd in range(2):
        for i in range(n):
            want, _ = trainer.update(ref, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i])
            got, ex = td3_oracle.update(td3, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], d=1)
            assert [type(x) for x in got] == [type(x) for x in want]
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (got, want)
            for w in ("actor", "critic", "tgt_actor", "tgt_critic"):
                assert _same(getattr(td3[i], w), getattr(ref[i], w)), (rnd, i, w)
            assert _same(td3[i].critic2, td3[i].critic) and _same(td3[i].tgt_critic2, td3[i].tgt_critic)
            assert ex["q_loss2"] == got[0]


def test_delay_leaves_actor_and_targets_untouched_on_odd_updates():
    c = synthetic_trainer_case(DIMS, B, L, seed=4)
    twins = td3_oracle.twin_case(c, DIMS, seed=4)
    ags = _agents(c, twins)
    i = 1
    for k in range(1, 5):
        before = copy.deepcopy({w: getattr(ags[i], w) for w in ("actor", "tgt_actor", "tgt_critic", "tgt_critic2")})
        opt = copy.deepcopy((ags[i].opt_actor.m, ags[i].opt_actor.v, ags[i].opt_actor.b1p, ags[i].opt_actor.b2p))
        c1, c2 = copy.deepcopy(ags[i].critic), copy.deepcopy(ags[i].critic2)
        st, ex = td3_oracle.update(ags, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], d=2)
        assert not _same(ags[i].critic, c1) and not _same(ags[i].critic2, c2)     # both critics step every time
        moved = {w: not _same(getattr(ags[i], w), before[w]) for w in before}
        if k % 2:
            assert not any(moved.values()), (k, moved)
            assert _same(ags[i].opt_actor.m, opt[0]) and _same(ags[i].opt_actor.v, opt[1])
            assert (ags[i].opt_actor.b1p, ags[i].opt_actor.b2p) == opt[2:]
            assert st[1] == (np.float32(0) if k == 1 else prev_p)                 # the most recent actor step's
        else:
            assert all(moved.values()), (k, moved)
            assert ex["actor_step"]
        prev_p = st[1]
    assert ags[i].td3_k == 4 and ags[i].td3_actor_steps == 2


def test_fixture_rule_balances_the_min():
    c = synthetic_trainer_case(DIMS, B, L, seed=5)
    twins = td3_oracle.twin_case(c, DIMS, seed=5)
    ags = _agents(c, twins)
    td3_oracle.balanced_twin_targets(ags, twins, c["data"], c["idx"], c["u_tgt"])
    ags = _agents(c, twins)
    for i in range(len(DIMS)):
        _, ex = td3_oracle.update(ags, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], d=2)
        share = ex["take_q1"].mean()
        assert 0.4 <= share <= 0.6, (i, share)


# ---- second derivation of both critics' gradients (the manner of tests/test_oracle_autograd.py)
from tests.test_oracle_autograd import F64, _cin, _gsm, _mlp, _t, fp64_oracle  # noqa: E402

CASES = [([18, 18, 18], 64, 64, None), ([8, 10, 10], 48, 64, [True, False, False])]


@pytest.mark.parametrize("dims,Bc,H,local_q", CASES)
def test_twin_critic_grads_match_autograd(dims, Bc, H, local_q):
    gamma = 0.95
    c = synthetic_trainer_case(dims, Bc, L=4 * Bc, seed=303, local_q=local_q, H=H)
    n, lq = len(dims), c["local_q"]
    twins = td3_oracle.twin_case(c, dims, seed=303, H=H)
    idx = c["idx"][0]
    batch_n = [tuple(np.asarray(x[idx], np.float64) for x in c["data"][j]) for j in range(n)]
    f64 = lambda p: {k: np.asarray(v, np.float64) for k, v in p.items()}  # noqa: E731
    params = [{w: f64(p[w]) for w in p} for p in c["params"]]
    tw = [{w: f64(t[w]) for w in t} for t in twins]
    for i in range(n):
        u_tgt = np.asarray(c["u_tgt"][i], np.float64)
        with fp64_oracle():
            ags = [trainer.AgentParams(**{w: dict(p[w]) for w in p}, local_q=lq[j]) for j, p in enumerate(params)]
            for j in range(n):
                td3_oracle.add_twin(ags[j], dict(tw[j]["critic2"]), dict(tw[j]["tgt_critic2"]))
            g1, g2, st = td3_oracle.critic_grads(ags, i, batch_n, u_tgt, gamma)
        obs_n = [torch.tensor(b[0], dtype=F64) for b in batch_n]
        act_n = [torch.tensor(b[1], dtype=F64) for b in batch_n]
        obs2_n = [torch.tensor(b[3], dtype=F64) for b in batch_n]
        rew, done = torch.tensor(batch_n[i][2], dtype=F64), torch.tensor(batch_n[i][4], dtype=F64)
        with torch.no_grad():
            tgt_act = [_gsm(_mlp(_t(params[j]["tgt_actor"]), obs2_n[j]), torch.tensor(u_tgt[j], dtype=F64))
                       for j in range(n)]
            x2 = _cin(obs2_n, tgt_act, i, lq[i])
            qn = torch.minimum(_mlp(_t(params[i]["tgt_critic"]), x2)[:, 0], _mlp(_t(tw[i]["tgt_critic2"]), x2)[:, 0])
            y = rew + gamma * (1.0 - done) * qn
        np.testing.assert_allclose(st["target_q"], y.numpy(), rtol=1e-12, atol=1e-12)
        for g, p, loss_o in ((g1, params[i]["critic"], st["q_loss"]), (g2, tw[i]["critic2"], st["q_loss2"])):
            cp = _t(p, grad=True)
            q = _mlp(cp, _cin(obs_n, act_n, i, lq[i]))[:, 0]
            loss = torch.mean((q - y) ** 2)
            gt = dict(zip(cp, torch.autograd.grad(loss, list(cp.values()))))
            assert abs(loss_o - loss.item()) <= 1e-12 * abs(loss.item())
            for k in nets.NAMES:
                want = gt[k].numpy().reshape(np.shape(g[k]))
                np.testing.assert_allclose(g[k], want, rtol=1e-10, atol=1e-14 * max(1.0, np.abs(want).max()),
                                           err_msg=f"agent {i} {k}")


# ---- host surface
def test_library_exports_td3_entry_points_and_refuses_null():
    from maddpg_amd import _lib
    lib = _lib.load()
    for name in ("mdp_td3_bytes", "mdp_td3_enable", "mdp_td3_info"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols(), name
    out = (ctypes.c_double * 4)()
    assert lib.mdp_td3_enable(None, None, 0, 2) < 0
    assert lib.mdp_td3_info(None, 0, out) < 0
    assert lib.mdp_td3_bytes(None) < 0
    # a handle whose create failed (no arena) is refused as a NULL one
    from tests.test_host_logic import _cfg
    h = ctypes.c_void_p()
    assert lib.mdp_create(ctypes.byref(_cfg()), None, 0, None, ctypes.byref(h)) != 0 and h.value
    assert lib.mdp_td3_enable(h, None, 0, 2) < 0 and lib.mdp_td3_info(h, 0, out) < 0
    lib.mdp_destroy(h)
    for k, v in (("critic2", 10), ("tgt_critic2", 11), ("m_critic2", 12), ("v_critic2", 13), ("g_critic2", 14)):
        assert _lib.WHICH[k] == v
    assert lib.mdp_abi_version() == _lib.ABI_VERSION == 5


def test_td3_bytes_holds_the_twin():
    from maddpg_amd import _lib
    from tests.test_host_logic import _cfg
    lib = _lib.load()
    pt = ctypes.c_int64()
    cfg = _cfg()
    assert lib.mdp_arena_bytes(ctypes.byref(cfg), ctypes.byref(pt)) > 0
    nb = lib.mdp_td3_bytes(ctypes.byref(cfg))
    assert nb >= 5 * 4 * pt.value            # five param-space-long regions, then partials, stats, sync area
    assert lib.mdp_td3_bytes(ctypes.byref(_cfg(n_agents=0))) < 0


def test_cli_defaults_and_refusals():
    from experiments.train import parse_args, td3_flags
    a = parse_args([])
    assert a.td3 is False and a.policy_delay == 2
    td3_flags(a)                               # off: nothing to refuse
    for extra in (["--prioritized-replay"], ["--update-mode", "throughput"], ["--num-gpus", "2"],
                  ["--save-format", "tf1"], ["--policy-delay", "0"], ["--policy-delay", "9"]):
        with pytest.raises(SystemExit):
            td3_flags(parse_args(["--td3"] + extra))
    td3_flags(parse_args(["--td3", "--policy-delay", "3"]))
