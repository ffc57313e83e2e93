"""CPU: the scenario table of simple_speaker_listener and hand-computed cases of
its restatement (tests/speaker_listener.py)."""
import numpy as np
import pytest

from maddpg_amd.envs import bench_record, spec
from tests.speaker_listener import SimpleSpeakerListener


def test_spec():
    sp = spec("simple_speaker_listener")
    assert sp.n_agents == 2 and sp.obs_dims == [3, 11] and sp.act_dims == [3, 5]
    assert [a.n for a in sp.action_space] == [3, 5]
    assert sp.observation_shapes == [(3,), (11,)]
    assert SimpleSpeakerListener().obs_dims() == [3, 11]
    with pytest.raises(AttributeError):
        bench_record(sp, np.zeros(8), 0)


def _state(listener, landmarks, goal):
    pos = np.zeros((1, 5, 2))
    pos[0, 0] = [0.9, -0.9]
    pos[0, 1] = listener
    pos[0, 2:] = landmarks
    return {"pos": pos, "vel": np.zeros((1, 5, 2)), "goal": np.array([goal]), "comm": np.zeros((1, 2, 3))}


def test_hand_computed_cases():
    sc = SimpleSpeakerListener()
    lm = [[0.5, 0.5], [-0.5, 0.25], [0.0, -0.75]]
    stay = np.zeros((1, 2, 5))
    stay[0, 0, :3] = [0.2, 0.7, 0.1]
    stay[0, 1, 0] = 1.0                                     # the no-op action: no force
    # the listener sits on the goal and does not move: reward 0 for both
    nst, obs, rew = sc.step(_state([-0.5, 0.25], lm, 1), stay)
    assert np.all(rew == 0.0) and rew.shape == (1, 2)
    np.testing.assert_array_equal(nst["pos"][0, 0], [0.9, -0.9])     # the speaker never moves
    # a known offset: d^2 = 0.3^2 + 0.4^2 = 0.25 -> -2 d^2 = -0.5 for both
    nst, obs, rew = sc.step(_state([0.3, -0.35], lm, 2), stay)
    np.testing.assert_allclose(rew, [[-0.5, -0.5]], atol=1e-15)
    # the message seen is the one emitted in the same step; the speaker sees the goal colour
    np.testing.assert_array_equal(obs[1][0, -3:], [0.2, 0.7, 0.1])
    np.testing.assert_array_equal(obs[0], [[0.15, 0.15, 0.65]])
    np.testing.assert_array_equal(nst["comm"][0], [[0.2, 0.7, 0.1], [0, 0, 0]])
    np.testing.assert_allclose(obs[1][0, :8], [0, 0, 0.2, 0.85, -0.8, 0.6, -0.3, -0.4], atol=1e-15)
    # the speaker's action moves nothing, the listener's does: a = [0, 1, 0, 0, 0] -> force +5 x
    push = stay.copy()
    push[0, 1] = [0, 1, 0, 0, 0]
    push[0, 0, :3] = [0, 1, 0]                              # would be a +x force on a movable agent
    nst, obs, rew = sc.step(_state([0.0, 0.0], lm, 0), push)
    np.testing.assert_array_equal(nst["pos"][0, 0], [0.9, -0.9])
    np.testing.assert_allclose(nst["vel"][0, 1], [0.5, 0.0])
    np.testing.assert_allclose(nst["pos"][0, 1], [0.05, 0.0])
    np.testing.assert_allclose(rew, -2 * (0.45 ** 2 + 0.5 ** 2) * np.ones((1, 2)))
    # comm is zero after a reset, and the goal is one of the 3 landmarks
    st = sc.reset(np.random.default_rng(0), 64)
    assert np.all(st["comm"] == 0) and st["comm"].shape == (64, 2, 3)
    assert set(st["goal"].tolist()) == {0, 1, 2} and np.all(st["vel"] == 0)
    assert np.abs(st["pos"]).max() <= 1 and np.abs(st["pos"][:, 2:]).max() > 0.8    # landmarks unscaled
    assert np.all(sc.observation(st)[1][:, -3:] == 0)
