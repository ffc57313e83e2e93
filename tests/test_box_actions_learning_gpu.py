"""GPU: `simple` with a Box(2) action space learns.

No CPU curve exists for Box actions (oracle/train_loop.py is Discrete), so the
test states no absolute reward, as tests/test_speaker_listener_learning_gpu.py
does not: over 12 lockstep batches of 1,024 episodes the mean of the last 4
batches must lie above the mean of the first 2 by more than 2 standard errors
of the per-episode means, on seeds 0 and 1, and every parameter stays finite.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

E, T, BATCHES = 1024, 25, 12


def train(seed, continuous=True):
    """VecRunner on E env copies; the total reward of every episode, one row per batch of E episodes"""
    from maddpg_amd.runner import VecRunner
    r = VecRunner("simple", E, seed=seed, episode_log_rows=4 * E, max_episode_len=T, continuous=continuous)
    rows = []
    for _ in range(BATCHES):
        for _ in range(T):
            r.step()
        r.synchronize()
        rew = r.episode_rewards(r.episodes() - E, E)
        assert np.all(np.isfinite(rew))
        rows.append(rew[:, 0].astype(np.float64))
    return r, np.stack(rows)


@pytest.mark.parametrize("seed", [0, 1])
def test_simple_with_box_actions_learns(seed):
    r, rew = train(seed)
    assert r.eng.act_kinds == ["box"] and r.rounds > 0
    first, last = rew[:2].ravel(), rew[-4:].ravel()
    se = float(np.sqrt(first.var(ddof=1) / first.size + last.var(ddof=1) / last.size))
    print(f"simple Box(2) seed {seed}: curve {[round(float(x), 3) for x in rew.mean(1)]}; first window "
          f"{first.mean():.3f}, last window {last.mean():.3f}, s.e. of the difference {se:.4f}")
    assert r.eng.check_finite() == 0
    assert last.mean() - first.mean() > 2.0 * se, rew.mean(1).tolist()
