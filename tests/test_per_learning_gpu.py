"""Prioritized replay learns (end to end, GPU): `simple` with the settings of
tests/test_learning_gpu.py's simple case and --prioritized-replay.

The bar comes from the uniform run of the same seed, measured once on an
MI355X and kept with both curves in tests/golden/per_learning.json: r0 its
untrained first batch, r1 its final value (mean of the last 4 batches).  PER
must reach at least r0 + 0.5 (r1 - r0): half the uniform improvement is the
allowance for seed noise."""
import json
import os

import numpy as np
import pytest

from tests.test_learning_gpu import _curve

pytestmark = pytest.mark.gpu


def test_simple_learns_with_prioritized_replay():
    with open(os.path.join(os.path.dirname(__file__), "golden", "per_learning.json")) as f:
        g = json.load(f)
    r0, r1 = g["r0"], g["r1"]
    assert r1 > r0 + 10.0, (r0, r1)                  # the fixture itself shows learning
    c = _curve("simple", g["batches"], seed=g["seed"], prioritized=True)
    final = float(np.mean(c[-4:]))
    print(f"uniform r0 {r0:.2f} r1 {r1:.2f}; prioritized final {final:.2f} (bar {r0 + 0.5 * (r1 - r0):.2f})")
    assert final >= r0 + 0.5 * (r1 - r0), c
