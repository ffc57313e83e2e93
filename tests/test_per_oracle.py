"""CPU tests of the prioritized-replay restatement (tests/per_oracle.py) and of
the host surface the feature adds (C-ABI symbols, CLI flags)."""
import subprocess
import sys
import os

import numpy as np

from tests import per_oracle as po

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_tree(t, prio, filled):
    P = len(t) // 2
    assert t.dtype == F32 and t.shape == (2 * P, 2)
    assert (t[0] == 0).all()
    lv = t[P:]
    k = len(prio)
    assert (lv[:k][filled, 0] == prio[filled]).all() and (lv[:k][filled, 1] == prio[filled]).all()
    empty = np.ones(P, bool)
    empty[:k] = ~filled
    assert (lv[empty, 0] == 0).all() and np.isinf(lv[empty, 1]).all()
    for node in range(1, P):
        l, r = t[2 * node], t[2 * node + 1]
        assert t[node, 0] == F32(l[0] + r[0])
        assert t[node, 1] == min(l[1], r[1])
    if filled.any():
        assert t[1, 1] == prio[filled].min()
        assert abs(float(t[1, 0]) - float(prio[filled].astype(np.float64).sum())) <= 1e-5 * float(t[1, 0])


def test_tree_invariants():
    rng = np.random.default_rng(0)
    for cap in (1, 2, 37, 64, 100):
        P = po.tree_leaves(cap)
        assert P >= cap and P & (P - 1) == 0 and (P == 1 or P // 2 < cap)
        prio = rng.uniform(0.05, 1.0, cap).astype(F32)
        filled = rng.uniform(size=cap) < 0.7
        _check_tree(po.build(prio, P, filled), prio, filled)
    # a pure function of the leaves: the order the leaves were set in cannot matter
    prio = rng.uniform(0.05, 1.0, 37).astype(F32)
    a = po.build(prio, 64)
    b = po.build(prio[::-1].copy()[::-1], 64)
    assert a.tobytes() == b.tobytes()


def test_never_an_empty_leaf():
    """200 random partial fills of a 64-leaf tree, u = 0 and u = nextafter(1, 0)
    included: no index >= len, no zero-priority leaf"""
    rng = np.random.default_rng(1)
    top = np.nextafter(F32(1), F32(0))
    for trial in range(200):
        ln = int(rng.integers(1, 65))
        prio = rng.uniform(0.01, 1.0, ln).astype(F32) ** F32(rng.uniform(0.2, 3.0))
        t = po.build(prio, 64)
        B = int(rng.choice([1, 7, 16, 40, 64]))
        for u in (np.zeros(B, F32), np.full(B, top, F32), rng.uniform(0, 1, B).astype(F32)):
            u = np.minimum(u, top)
            idx = po.sample(t, B, u)
            assert idx.min() >= 0 and idx.max() < ln, (trial, ln, idx)
            assert (t[64 + idx, 0] > 0).all()


def test_one_filled_leaf_and_equal_priorities():
    t = po.build(np.array([0, 0, 0.5], F32), 4, filled=[False, False, True])
    assert (po.sample(t, 8, np.linspace(0, 0.99, 8).astype(F32)) == 2).all()
    t = po.build(np.full(16, 0.25, F32), 16)
    assert (po.sample(t, 16, np.full(16, 0.5, F32)) == np.arange(16)).all()
    assert (po.weights(t, np.arange(16), F32(0.7)) == 1).all()


def test_stratified_frequencies_within_4_sigma():
    """leaf frequencies of the stratified sampler on a fixed 64-leaf case against
    the multinomial's N p (1 - p) spread (the stratified draw has less variance)"""
    rng = np.random.default_rng(2)
    prio = po.priority_from_error(rng.exponential(0.3, 50).astype(F32))
    t = po.build(prio, 64)
    B, draws = 256, 200
    counts = np.zeros(64)
    for _ in range(draws):
        u = np.minimum(rng.uniform(0, 1, B).astype(F32), np.nextafter(F32(1), F32(0)))
        counts += np.bincount(po.sample(t, B, u), minlength=64)
    N = B * draws
    p = t[64:, 0].astype(np.float64) / float(t[1, 0])
    sigma = np.sqrt(N * p * (1 - p))
    assert (counts[50:] == 0).all()
    z = np.abs(counts[:50] - N * p[:50]) / sigma[:50]
    print(f"worst |count - N p| / sigma = {z.max():.2f}")
    assert z.max() < 4.0


def test_weights_and_beta():
    prio = np.array([0.1, 0.4, 0.2, 0.8], F32)
    t = po.build(prio, 4)
    w = po.weights(t, [0, 1, 2, 3], F32(0.5))
    np.testing.assert_allclose(w, (prio / F32(0.1)) ** F32(-0.5), rtol=1e-6)
    assert w.max() == 1.0 and (w > 0).all()
    assert po.beta_after(0) == po.BETA0
    assert po.beta_after(1) == F32(po.BETA0 + po.BETA_INC)
    assert po.beta_after(700) == 1.0          # saturates at exactly 1
    assert po.priority_from_error(F32(5.0)) == 1.0
    assert po.priority_from_error(F32(0.0)) == np.power(F32(0.01), F32(0.6))


def test_device_uniforms_are_the_documented_philox_words():
    from oracle import philox
    u = po.device_uniforms(1234567, 2, 3, 8)
    key = np.array([1234567, 0], np.uint64)
    c = np.array([[i, 3, 0x50002, 0] for i in range(8)], np.uint64)
    assert (u == philox.u01(philox.philox4x32_10(c, key)[:, 0])).all()
    assert (u >= 0).all() and (u < 1).all()


def test_lib_declares_the_per_symbols():
    from maddpg_amd import _lib
    want = {"mdp_per_bytes", "mdp_per_enable", "mdp_per_sample", "mdp_per_set_priorities",
            "mdp_per_update_errors", "mdp_per_get_tree", "mdp_per_info"}
    assert want <= set(_lib.SIGNATURES)
    assert want <= set(_lib.header_symbols())
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in want)
    # additive: same ABI version, the configuration keeps its layout
    assert lib.mdp_abi_version() == 5


def test_per_bytes_needs_no_gpu():
    import ctypes
    from maddpg_amd import _lib
    lib = _lib.load()
    c = _lib.MdpConfig()
    c.n_agents = 3
    for i in range(3):
        c.obs_dim[i] = 18
    c.act_dim, c.num_units, c.batch_size, c.max_episode_len = 5, 64, 1024, 25
    c.capacity, c.num_envs, c.scenario = 1000000, 1024, 2
    nb = lib.mdp_per_bytes(ctypes.byref(c))
    P = 1 << 20
    assert 3 * 2 * P * 8 <= nb < 3 * 2 * P * 8 + 3 * 3 * 4 * 1024 + 8192
    c.act_dim = 4
    assert lib.mdp_per_bytes(ctypes.byref(c)) < 0


def test_train_help_lists_the_per_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "experiments", "train.py"), "--help"],
                         capture_output=True, text=True, cwd=ROOT, check=True).stdout
    for flag in ("--prioritized-replay", "--per-alpha", "--per-beta0", "--per-beta-inc", "--per-eps"):
        assert flag in out, flag
