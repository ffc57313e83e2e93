"""GPU: simple_speaker_listener on the device (k_rollout, k_env_obs, reset, the
comm state) against its restatement in tests/speaker_listener.py, with the
tolerances of tests/test_gpu_parity.py's env tests: state and observations
atol 2e-5, reward rtol 1e-5 / atol 5e-5, stored actions exact, reset positions
atol 1e-6.  The scenario is restated from memory of upstream MPE: UNPINNED.
"""
import argparse
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd import _lib  # noqa: E402
from maddpg_amd.engine import Engine  # noqa: E402
from maddpg_amd.envs import Discrete, spec  # noqa: E402
from oracle import nets, philox  # noqa: E402
from tests.helpers import row_layout  # noqa: E402
from tests.speaker_listener import SimpleSpeakerListener  # noqa: E402

NAME = "simple_speaker_listener"
ACT = 5
SP = spec(NAME)
LAY, _STRIDE = row_layout(SP.obs_dims)


def _engine(E, **kw):
    kw.setdefault("batch_size", 16)
    kw.setdefault("capacity", 1000)
    return Engine(SP.obs_dims, num_envs=E, scenario=NAME, **kw)


def _oracle_state(st):
    return {"pos": st["pos"].astype(np.float64), "vel": st["vel"].astype(np.float64), "goal": st["goal"],
            "comm": st["comm"][:, :, :3].astype(np.float64)}


def test_handle_has_the_scenarios_widths():
    eng = _engine(4)
    assert eng.act_dims == [3, 5] and eng.obs_dims == [3, 11]
    assert [(r, c) for (_o, r, c, _dr, _dc) in eng.net_tensors(0, 0)][4:] == [(64, 3), (1, 3)]
    assert eng.net_tensors(1, 1)[0][1:3] == (3 + 11 + 3 + 5, 64)
    with pytest.raises(ValueError, match="scenario"):
        _engine(4, act_dims=[5, 5])
    with pytest.raises(ValueError, match="2 agents"):
        Engine([3, 11, 11], num_envs=4, scenario=NAME, batch_size=16, capacity=100)


def test_env_step_parity():
    E = 37   # ragged: not a multiple of the 16-env tile
    eng = _engine(E, max_episode_len=25, seed=3)
    eng.env_reset()
    sc = SimpleSpeakerListener()
    rng = np.random.default_rng(4)
    for step in range(3):
        z = rng.normal(size=(E, 2, ACT))
        z[:, 0, 3:] = -np.inf                                  # the speaker's 3-vector, padded with zeros
        act = (np.exp(z) / np.exp(z).sum(-1, keepdims=True)).astype(np.float32)
        assert np.all(act[:, 0, 3:] == 0)
        st = eng.env_state()
        ost = _oracle_state(st)
        obs0 = sc.observation(ost)
        np.testing.assert_allclose(eng.env_obs().cpu().numpy(), np.concatenate(obs0, 1), atol=2e-5)
        nst, obs1, rew = sc.step(ost, act.astype(np.float64))
        eng.env_step(act_in=torch.from_numpy(act))
        got = eng.env_state()
        np.testing.assert_allclose(got["pos"], nst["pos"], atol=2e-5)
        np.testing.assert_allclose(got["vel"], nst["vel"], atol=2e-5)
        np.testing.assert_array_equal(got["pos"][:, 0], st["pos"][:, 0])       # the speaker does not move
        np.testing.assert_array_equal(got["comm"][:, 0, :3], act[:, 0, :3])   # state.c = action.c, no noise
        assert np.all(got["comm"][:, 0, 3:] == 0) and np.all(got["comm"][:, 1] == 0)
        rows = eng.replay_rows(step * E, E).cpu().numpy()
        for j in range(2):
            lj, o = LAY[j], SP.obs_dims[j]
            np.testing.assert_allclose(rows[:, lj["obs"]:lj["obs"] + o], obs0[j], atol=2e-5)
            np.testing.assert_array_equal(rows[:, lj["act"]:lj["act"] + ACT], act[:, j])
            np.testing.assert_allclose(rows[:, lj["nobs"]:lj["nobs"] + o], obs1[j], atol=2e-5)
            np.testing.assert_allclose(rows[:, lj["rew"]], rew[:, j], rtol=1e-5, atol=5e-5)
            assert np.all(rows[:, lj["done"]] == 0)
        # the listener's next observation carries the message emitted this step
        np.testing.assert_array_equal(rows[:, LAY[1]["nobs"] + 8:LAY[1]["nobs"] + 11], act[:, 0, :3])
        np.testing.assert_allclose(eng.env_obs().cpu().numpy(), np.concatenate(obs1, 1), atol=2e-5)
    assert eng.buffer_len() == 3 * E


def test_set_comm_round_trip_and_obs():
    E = 5
    eng = _engine(E)
    eng.env_reset()
    st = eng.env_state()
    comm = np.zeros((E, 2, ACT), np.float32)
    comm[:, 0, :3] = np.random.default_rng(1).uniform(size=(E, 3))
    eng.set_env_state(st["pos"], st["vel"], st["goal"], st["ep_step"], comm=comm)
    np.testing.assert_array_equal(eng.env_state()["comm"], comm)
    obs = eng.env_obs().cpu().numpy()
    np.testing.assert_array_equal(obs[:, 3 + 8:], comm[:, 0, :3])
    # a scenario whose agents are all silent: zeros, and set is refused
    sp = spec("simple_spread")
    e2 = Engine(sp.obs_dims, num_envs=3, scenario="simple_spread", batch_size=16, capacity=100)
    e2.env_reset()
    assert np.all(e2.env_state()["comm"] == 0)
    with pytest.raises(_lib.MdpError, match="silent"):
        s2 = e2.env_state()
        e2.set_env_state(s2["pos"], s2["vel"], comm=np.zeros((3, 3, ACT), np.float32))


def test_reset_on_pinned_philox():
    E, seed = 37, 0x0123456789ABCDEF
    eng = _engine(E, seed=seed)
    sc = SimpleSpeakerListener()
    goals = set()
    for k in range(2):
        eng.env_reset()
        st = eng.env_state()
        u = philox.slot_uniforms(seed, 0x30000, k, np.arange(E), 2 * 5 + 1)
        want = sc.reset(philox.ResetStream(u, 5), E)
        np.testing.assert_allclose(st["pos"], want["pos"], rtol=0, atol=1e-6, err_msg=f"reset {k}")
        assert np.all(st["vel"] == 0) and np.all(st["ep_step"] == 0) and np.all(st["comm"] == 0)
        np.testing.assert_array_equal(st["goal"], want["goal"])
        goals |= set(st["goal"].tolist())
    assert goals <= {0, 1, 2} and len(goals) > 1


def test_episode_end_resets_comm_and_redraws_the_goal():
    E, seed, T = 20, 0xDEADBEEF12345678, 3
    eng = _engine(E, max_episode_len=T, seed=seed)
    eng.env_reset()
    eng.init_params(0)
    for k in range(T):
        eng.env_step()
        eng.synchronize()
        st = eng.env_state()
        if k < T - 1:
            rows = eng.replay_rows(k * E, E).cpu().numpy()
            np.testing.assert_array_equal(st["comm"][:, 0], rows[:, LAY[0]["act"]:LAY[0]["act"] + ACT])
            assert np.all(st["comm"][:, 0, :3] > 0) and np.all(st["ep_step"] == k + 1)
    assert np.all(st["ep_step"] == 0) and np.all(st["comm"] == 0)
    assert eng.episode_count() == E
    sc = SimpleSpeakerListener()
    want = sc.reset(philox.ResetStream(philox.slot_uniforms(seed, 0x20000, T - 1, np.arange(E), 11), 5), E)
    np.testing.assert_allclose(st["pos"], want["pos"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(st["goal"], want["goal"])
    assert len(set(st["goal"].tolist())) > 1
    log = eng.episode_log(0, E)
    assert log.shape == (E, 3)
    rows = eng.replay_rows(0, T * E).cpu().numpy()
    per_env = sum(rows[k * E:(k + 1) * E, LAY[j]["rew"]] for k in range(T) for j in range(2))
    np.testing.assert_allclose(log[:, 0], per_env, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(log[:, 0], log[:, 1:].sum(1), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("H", [64, 128])
def test_policy_rollout_without_injected_actions(H):
    """the stored speaker action is the 3-wide Gumbel-softmax of its actor on its
    stored obs (Philox stream 0x10000 | agent, counter = vector step, first 3 of
    the 5 uniforms), pad entries zero; the next listener obs carries it"""
    E, seed = 37, 0xDEADBEEF12345678
    eng = _engine(E, seed=seed, num_units=H)
    eng.init_params(4)
    eng.env_reset()
    actors = [eng.get_params(j, "actor") for j in range(2)]
    assert actors[0]["W3"].shape == (H, 3)
    for k in range(2):
        eng.env_step()
        eng.synchronize()
        rows = eng.replay_rows(k * E, E).cpu().numpy()
        for j, w in enumerate((3, 5)):
            o = SP.obs_dims[j]
            logits = nets.mlp_fwd(actors[j], rows[:, LAY[j]["obs"]:LAY[j]["obs"] + o])[0]
            u = philox.uniforms5(seed, 0x10000 | j, k, np.arange(E))[:, :w]
            got = rows[:, LAY[j]["act"]:LAY[j]["act"] + ACT]
            np.testing.assert_allclose(got[:, :w], nets.gumbel_softmax(logits, u), atol=2e-6, err_msg=f"{k} {j}")
            assert np.all(got[:, w:] == 0)
        np.testing.assert_array_equal(rows[:, LAY[1]["nobs"] + 8:LAY[1]["nobs"] + 11],
                                      rows[:, LAY[0]["act"]:LAY[0]["act"] + 3])
    # injected uniforms: the same through u_in
    u = np.random.default_rng(2).uniform(1e-6, 1, size=(E, 2, ACT)).astype(np.float32)
    u[:, 0, 3:] = np.nan                                      # pad uniforms are never used
    obs = eng.env_obs().cpu().numpy()
    eng.env_step(u=torch.from_numpy(u))
    rows = eng.replay_rows(2 * E, E).cpu().numpy()
    want = nets.gumbel_softmax(nets.mlp_fwd(actors[0], obs[:, :3])[0], u[:, 0, :3])
    np.testing.assert_allclose(rows[:, LAY[0]["act"]:LAY[0]["act"] + 3], want, atol=2e-6)
    assert np.all(rows[:, LAY[0]["act"] + 3:LAY[0]["act"] + 5] == 0)


def _snapshot(eng, nrows):
    st = eng.env_state()
    return [st["pos"], st["vel"], st["goal"], st["ep_step"], st["comm"],
            eng.replay_rows(0, nrows).cpu().numpy().copy()]


def test_multi_step_rollout_equals_single_steps():
    """num_envs = 16: a mdp_train_steps group of rollout-only steps runs in one launch
    (the comm state handed from step to step inside it); bitwise the same as one by one"""
    E, T = 16, 7
    res = []
    for multi in (True, False):
        eng = _engine(E, seed=11, max_episode_len=3)          # episodes end inside the group
        eng.init_params(2)
        eng.env_reset()
        if multi:
            eng.train_steps([0] * T)
        else:
            for _ in range(T):
                eng.train_step(0)
        eng.synchronize()
        assert eng.buffer_len() == E * T
        res.append(_snapshot(eng, E * T))
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    assert np.any(res[0][4] != 0)                             # mid-episode: a message is standing


def test_train_step_graph_equals_eager():
    """one mdp_train_step with rounds due: captured and eager give bit-identical parameters"""
    from maddpg_amd.runner import VecRunner
    res = []
    for graphs in (True, False):
        r = VecRunner(NAME, 64, batch_size=128, capacity=20000, seed=3, train_every=16, max_episode_len=5)
        assert r.eng.act_dims == [3, 5]
        r.eng.set_graphs(graphs)
        r.prefill()
        for _ in range(3):
            assert r.step() == 4
        r.eng.synchronize()
        assert r.eng.check_finite() == 0
        res.append([r.eng.region(k).cpu().numpy().view(np.uint32).copy() for k in ("theta", "target", "adam_m", "adam_v")]
                   + _snapshot(r.eng, 1000) + [r.eng.get_rng_state()])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_benchmark_records_are_refused():
    eng = _engine(4)
    eng.init_params(0)
    eng.env_reset()
    with pytest.raises(_lib.MdpError, match="benchmark_data"):
        eng.env_step_bench()
    assert eng.buffer_len() == 0


def test_facade_reference_loop():
    """the reference-style loop of tests/test_facade_gpu.py with act_space_n =
    [Discrete(3), Discrete(5)], the scenario stepped on the host"""
    from maddpg_amd.common import tf_util as U
    from maddpg_amd.trainer.maddpg import MADDPGAgentTrainer
    args = argparse.Namespace(lr=1e-2, gamma=0.95, batch_size=64, num_units=64, max_episode_len=5)
    sc = SimpleSpeakerListener()
    rng = np.random.default_rng(0)
    with U.single_threaded_session():
        trainers = [MADDPGAgentTrainer(f"agent_{i}", None, [(3,), (11,)], [Discrete(3), Discrete(5)], i, args)
                    for i in range(2)]
        U.initialize()
        eng = U.get_session().engine()
        assert eng.act_dims == [3, 5]
        random.seed(5)
        st = sc.reset(rng, 1)
        obs_n = [o[0] for o in sc.observation(st)]
        episode_step = trained = 0
        for train_step in range(1, 421):
            action_n = [a.action(o) for a, o in zip(trainers, obs_n)]
            assert action_n[0].shape == (3,) and action_n[1].shape == (5,)
            for a in action_n:
                assert a.dtype == np.float32 and abs(float(a.sum()) - 1) < 1e-5
            padded = np.zeros((1, 2, 5))
            padded[0, 0, :3], padded[0, 1] = action_n[0], action_n[1]
            st, new_obs_n, rew = sc.step(st, padded)
            episode_step += 1
            terminal = episode_step >= args.max_episode_len
            for i, ag in enumerate(trainers):
                ag.experience(obs_n[i], action_n[i], rew[0, i], new_obs_n[i][0], False, terminal)
            obs_n = [o[0] for o in new_obs_n]
            if terminal:
                st = sc.reset(rng, 1)
                obs_n = [o[0] for o in sc.observation(st)]
                episode_step = 0
            for ag in trainers:
                ag.preupdate()
            for ag in trainers:
                loss = ag.update(trainers, train_step)
                if not (len(ag.replay_buffer) >= 320 and train_step % 100 == 0):
                    assert loss is None
                    continue
                trained += 1
                assert type(loss) is list and len(loss) == 6 and all(np.isfinite(loss))
                assert [type(x) for x in loss] == [np.float32, np.float32, np.float64, np.float64,
                                                   np.float32, np.float64]
        assert trained == 2
        # the stored speaker actions: 3 wide through the buffer, pad entries zero on the device
        o, a, r, o2, d = trainers[0].replay_buffer.sample_index(list(range(8)))
        assert a.shape == (8, 3) and o.shape == (8, 3)
        rows = eng.replay_rows(0, 8).cpu().numpy()
        assert np.all(rows[:, LAY[0]["act"] + 3:LAY[0]["act"] + 5] == 0)
        np.testing.assert_array_equal(rows[:, LAY[0]["act"]:LAY[0]["act"] + 3], a)
        ob = [np.stack([obs_n[j]] * 7) for j in range(2)]
        assert trainers[0].p_debug["target_act"](ob[0]).shape == (7, 3)
        assert trainers[0].p_debug["p_values"](ob[0]).shape == (7, 3)
        acts = [np.full((7, 3), 1 / 3, np.float32), np.full((7, 5), 0.2, np.float32)]
        q = trainers[1].q_debug["q_values"](ob[0], ob[1], acts[0], acts[1])
        assert q.shape == (7,) and np.all(np.isfinite(q))
