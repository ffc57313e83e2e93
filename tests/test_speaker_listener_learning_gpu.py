"""GPU: simple_speaker_listener learns, and what it learns goes through the channel.

No CPU curve fixture exists (oracle/train_loop.py is fixed at width 5), so the
test states no absolute reward: the last window of the training curve must
beat the first, and the trained policies must do better with the speaker's
real messages than with the constant message [1/3, 1/3, 1/3], episode by
episode from identical reset states.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

NAME = "simple_speaker_listener"
E, T = 1024, 25
BATCHES = 12          # lockstep batches of E episodes ("Action widths and simple_speaker_listener")


def train(batches, seed=0):
    """VecRunner on E env copies; the mean total episode reward of every batch of E episodes"""
    from maddpg_amd.runner import VecRunner
    r = VecRunner(NAME, E, seed=seed, episode_log_rows=4 * E, max_episode_len=T)
    curve = []
    for _ in range(batches):
        for _ in range(T):
            r.step()
        r.synchronize()
        n = r.episodes()
        rew = r.episode_rewards(n - E, E)
        assert np.all(np.isfinite(rew))
        curve.append(float(rew[:, 0].mean()))
    return r, curve


def evaluate(r, start, ablate):
    """E episodes of the trained policies from the reset states `start`; ablate: the
    speaker's action replaced by the constant [1/3, 1/3, 1/3] (through act_in, the
    listener still acting by its own policy on what it then observes)"""
    eng = r.eng
    eng.set_env_state(start["pos"], start["vel"], start["goal"], np.zeros(E, np.int32),
                      comm=np.zeros((E, 2, 5), np.float32))
    first = eng.episode_count()
    for _ in range(T):
        if ablate:
            obs = eng.env_obs()
            act = torch.zeros((E, 2, 5), device=obs.device)
            act[:, 0, :3] = 1.0 / 3.0
            act[:, 1] = eng.act(1, obs[:, 3:])
            eng.env_step(act_in=act)
        else:
            eng.env_step()
    eng.synchronize()
    assert eng.episode_count() == first + E
    return eng.episode_log(first, E)[:, 0].astype(np.float64)      # env order (lockstep)


def channel_gap(r):
    start = r.eng.env_state()
    assert np.all(start["ep_step"] == 0)
    real, abl = evaluate(r, start, False), evaluate(r, start, True)
    d = real - abl
    return float(real.mean()), float(abl.mean()), float(d.mean()), float(d.std(ddof=1) / np.sqrt(len(d)))


def test_learns_and_the_channel_matters():
    r, curve = train(BATCHES)
    first, last = float(np.mean(curve[:2])), float(np.mean(curve[-4:]))
    real, abl, gap, se = channel_gap(r)
    print(f"speaker_listener: first window {first:.2f}, last window {last:.2f}; trained policies over {E} episodes: "
          f"real messages {real:.2f}, constant message {abl:.2f}, mean difference {gap:.2f} +- {se:.2f} (s.e.)")
    assert last > first, curve
    assert gap > 2.0 * se, (real, abl, gap, se)
