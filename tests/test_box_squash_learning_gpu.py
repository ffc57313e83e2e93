"""GPU: `simple_spread` with tanh-squashed Box(2) actions stays finite and learns.

With the plain Gaussian policy this scenario reports -inf at every point (an
unbounded force overflows at random initialisation); the
squash bounds the force, so every episode reward and every parameter must be
finite throughout.  The improvement criterion is
tests/test_box_actions_learning_gpu.py's: over BATCHES lockstep batches of 1,024
episodes the mean of the last 4 batches must lie above the mean of the first 2
by more than 2 standard errors of the difference, on seeds 0 and 1.  BATCHES is
the smallest of 12, 24, 48 at which both seeds met it on MI355X (DESIGN.md
section 26 has the curves).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

E, T, BATCHES = 1024, 25, 12


def train(seed, batches=BATCHES, continuous=True, squash="tanh"):
    """VecRunner on E env copies; the team reward of every episode, one row per batch of E episodes"""
    from maddpg_amd.runner import VecRunner
    r = VecRunner("simple_spread", E, seed=seed, episode_log_rows=4 * E, max_episode_len=T, continuous=continuous,
                  **({"squash": squash} if continuous else {}))
    rows = []
    for _ in range(batches):
        for _ in range(T):
            r.step()
        r.synchronize()
        rew = r.episode_rewards(r.episodes() - E, E)
        assert np.all(np.isfinite(rew))
        assert r.eng.check_finite() == 0
        rows.append(rew[:, 0].astype(np.float64))
    return r, np.stack(rows)


def criterion(rew):
    first, last = rew[:2].ravel(), rew[-4:].ravel()
    se = float(np.sqrt(first.var(ddof=1) / first.size + last.var(ddof=1) / last.size))
    return float(first.mean()), float(last.mean()), se


@pytest.mark.parametrize("seed", [0, 1])
def test_simple_spread_with_squashed_box_actions_is_finite_and_learns(seed):
    r, rew = train(seed)
    assert r.eng.act_kinds == ["box"] * 3 and r.eng.act_squash == ["tanh"] * 3 and r.rounds > 0
    first, last, se = criterion(rew)
    print(f"simple_spread tanh Box(2) seed {seed}: curve {[round(float(x), 3) for x in rew.mean(1)]}; first window "
          f"{first:.3f}, last window {last:.3f}, s.e. of the difference {se:.4f}")
    assert r.eng.check_finite() == 0
    assert last - first > 2.0 * se, rew.mean(1).tolist()
