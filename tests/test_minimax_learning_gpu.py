"""M3DDPG learns (end to end, GPU): simple_adversary with the settings of
tests/test_learning_gpu.py's adversary case (the adversary on DDPG's local critic,
the two good agents on MADDPG critics -- the agents --minimax changes) and --minimax
at the default rates 1e-3 / 1e-5.

The bar follows tests/test_per_learning_gpu.py's rule, agent by agent: from the
MADDPG run of the same seed, measured once on an MI355X and kept with both curves
in tests/golden/minimax_learning.json, r0 is an agent's mean reward in the
untrained first batch and r1 its final value (mean of the last 4 batches).
M3DDPG must reach at least r0 + 0.5 (r1 - r0) for every agent: half the MADDPG
improvement is the allowance for seed noise."""
import json
import os

import numpy as np
import pytest

from tests.test_learning_gpu import _curve

pytestmark = pytest.mark.gpu


def test_simple_adversary_learns_with_minimax():
    with open(os.path.join(os.path.dirname(__file__), "golden", "minimax_learning.json")) as f:
        g = json.load(f)
    r0, r1 = np.array(g["r0"]), np.array(g["r1"])
    assert r0[0] < -20.0 and r1[0] > r0[0] + 10.0, (r0, r1)      # the fixture itself shows the adversary learning
    c = _curve("simple_adversary", g["batches"], seed=g["seed"], per_agent=True, num_adversaries=1,
               adv_policy="ddpg", minimax=True)[:, 1:]
    final = c[-4:].mean(0)
    bar = r0 + 0.5 * (r1 - r0)
    print(f"MADDPG r0 {r0} r1 {r1}; M3DDPG final {final} (bar {bar})")
    assert np.all(final >= bar), c
