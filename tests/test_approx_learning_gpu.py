"""MADDPG with inferred policies learns (end to end, GPU): simple_spread, 1,024 env
copies, every agent's TD target built from its own approximators of the others.

The reward bar follows tests/test_minimax_learning_gpu.py's rule: from the MADDPG
run of the same seed, measured once on an MI355X and kept with both curves in
tests/golden/approx_learning.json, r0 is the untrained first batch and r1 the
mean of the last 4 batches.  The approx run must reach r0 + 0.5 (r1 - r0): half
the MADDPG improvement is the allowance for seed noise.

The approximators themselves: at the end of the run the mean cross-entropy of
every pair on fresh replay rows must be below log A_j, what a constant uniform
guess scores.  The cross-entropy of the true policies on the same rows and the
mean KL are printed for the record and not asserted: untrained, policy and
approximator are both near uniform, so the KL starts near zero and rises as the
policies sharpen -- its direction proves nothing; and the ring holds actions of
older policies, so the present policy need not score well on them."""
import json
import math
import os

import numpy as np
import pytest

from tests.test_learning_gpu import _curve

pytestmark = pytest.mark.gpu


def test_simple_spread_learns_with_inferred_policies(monkeypatch):
    from maddpg_amd import runner
    with open(os.path.join(os.path.dirname(__file__), "golden", "approx_learning.json")) as f:
        g = json.load(f)
    r0, r1 = g["r0"], g["r1"]
    # the fixture itself shows MADDPG learning (tests/test_learning_gpu.py's own bars for this scenario)
    assert r0 < -550.0 and r1 > r0 + 120.0, (r0, r1)
    made = []

    class Kept(runner.VecRunner):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(runner, "VecRunner", Kept)
    c = _curve(g["scenario"], g["batches"], seed=g["seed"], num_envs=g["num_envs"], approx=True)
    final, bar = float(np.mean(c[-4:])), r0 + 0.5 * (r1 - r0)
    print(f"MADDPG r0 {r0:.1f} r1 {r1:.1f}; inferred policies final {final:.1f} (bar {bar:.1f})")
    assert final >= bar, c
    eng = made[0].eng
    assert eng.approx and eng.check_finite() == 0
    q = eng.approx_quality()
    assert len(q["pairs"]) == 6
    for (i, j), v in sorted(q["pairs"].items()):
        print(f"pair ({i}, {j}): cross-entropy {v['ce']:.3f} (uniform guess {math.log(eng.act_dims[j]):.3f}), "
              f"true policy's {v['ce_true']:.3f}, KL {v['kl']:.3f}")
        assert v["ce"] < math.log(eng.act_dims[j]), (i, j, v)
        assert eng.approx_info(i, j)["updates"] > 0
