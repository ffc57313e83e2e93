"""GPU: the critic diagnostic measures something.  `simple` trained as
tests/test_learning_gpu.py trains it (12 lockstep batches of 1,024 env copies):
the trained critic's Q lies closer to the discounted return its policy then
collects than the freshly initialised critic's does to its own policy's, on the
same 1,024 evaluation ids (RMS over the episodes of the mean gap of the 25 scored
steps; 115 steps played).  Measured on MI355X: untrained mean Q 0.03, mean return-to-go
-28.09, RMS gap 36.35; trained mean Q -0.906, mean return-to-go -0.949, RMS gap
0.064.  The pair, and MATD3's, are in profiles/eval_q.json (tools/eval_q_bench.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_training_closes_the_gap_between_q_and_the_realised_return():
    from maddpg_amd.runner import VecRunner
    r = VecRunner("simple", 1024, seed=0, episode_log_rows=4096)
    fresh = r.evaluate_q(1024)
    assert (fresh["steps"], fresh["scored"]) == (115, 25) and fresh["q"].shape == (1024, 115, 1, 1)
    for _ in range(12 * 25):
        r.step()
    r.synchronize()
    trained = r.evaluate_q(1024)
    f, t = fresh["summary"], trained["summary"]
    print(f"untrained: mean Q {f['q_mean'][0][0]:.4f}, mean G {f['g_mean'][0][0]:.4f}, rms gap {f['gap_rms'][0][0]:.4f}; "
          f"trained: mean Q {t['q_mean'][0][0]:.4f}, mean G {t['g_mean'][0][0]:.4f}, rms gap {t['gap_rms'][0][0]:.4f}")
    assert np.isfinite(f["gap_rms"][0][0]) and np.isfinite(t["gap_rms"][0][0])
    assert t["g_mean"][0][0] > f["g_mean"][0][0]          # the policy learned (the returns are negative distances)
    assert t["gap_rms"][0][0] < f["gap_rms"][0][0]
