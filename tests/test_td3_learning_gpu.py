"""MATD3 learns (end to end, GPU): `--td3` on `simple` with 1,024 env copies.

The bar is the MADDPG test's for the same scenario (tests/test_learning_gpu.py:
mean episode reward > -9 over the last 4 of 12 batches of 1,024 episodes; MADDPG
measured about -6).  It is this project's bar, not a MATD3 reference number.
Measured curves (MI355X, d = 2): profiles/td3_learning.json and DESIGN.md
section 17.
"""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.slow]


@pytest.mark.parametrize("seed", [0, 1])
def test_simple_learns_with_td3(seed):
    from tests.test_learning_gpu import _curve
    c = _curve("simple", 12, seed=seed, td3=True, policy_delay=2)
    print(f"td3 simple seed {seed}: {[round(x, 3) for x in c]}")
    assert c[0] < -20.0, c                       # untrained (training starts after the first batch)
    assert np.mean(c[-4:]) > -9.0, c
