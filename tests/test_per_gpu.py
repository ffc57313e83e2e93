"""Device-side prioritized replay (mdp_per.hip, mdp_per_*) against the CPU
restatement tests/per_oracle.py: tree and sampler bit-exact, the device noise
stream, the sampling distribution, beta, the importance-weighted critic step,
ring sync, graph replay == eager, refusals and the PrioritizedReplayMemory facade."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import trainer
from tests import per_oracle as po
from tests.helpers import joint_rows, synthetic_trainer_case

pytestmark = pytest.mark.gpu

F32 = np.float32
TOP = np.nextafter(F32(1), F32(0))


def _engine(cap, n_rows=None, dims=(6,), B=16, **kw):
    from maddpg_amd.engine import Engine
    eng = Engine(list(dims), batch_size=B, capacity=cap, prioritized=True, **kw)
    n_rows = cap if n_rows is None else n_rows
    if n_rows:
        rows = np.random.default_rng(5).normal(size=(n_rows, eng.row_stride)).astype(F32)
        eng.add_rows(torch.from_numpy(rows))
    return eng


def _set(eng, agent, pos, p):
    eng.per_set_priorities(agent, torch.from_numpy(np.asarray(pos, np.int32)), torch.from_numpy(np.asarray(p, F32)))


def _same_bits(a, b):
    return np.asarray(a, F32).tobytes() == np.asarray(b, F32).tobytes()


# ------------------------------------------------------- tree and sampler
@pytest.mark.parametrize("cap", [37, 4096])
@pytest.mark.parametrize("B", [16, 40])
def test_tree_and_sampler_bit_exact(cap, B):
    rng = np.random.default_rng(cap + B)
    eng = _engine(cap)
    P = po.tree_leaves(cap)
    assert eng.per_nodes == 2 * P
    # a fresh tree: every filled row at the new-row priority abs_err_upper ** alpha = 1
    assert _same_bits(eng.per_tree(0), po.build(np.ones(cap, F32), P))
    prio = (rng.uniform(0.02, 1.0, cap).astype(F32) ** F32(2.5)).astype(F32)
    order = rng.permutation(cap)
    for chunk in np.array_split(order, 3):                    # any update order gives the same bits
        _set(eng, 0, chunk, prio[chunk])
    want = po.build(prio, P)
    assert _same_bits(eng.per_tree(0), want)
    k = 0
    for u in (rng.uniform(0, 1, B).astype(F32), np.zeros(B, F32), np.full(B, TOP, F32)):
        u = np.minimum(u, TOP)
        idx, w = eng.per_sample(0, B, u=torch.from_numpy(u))
        k += 1
        assert (idx.cpu().numpy() == po.sample(want, B, u)).all()
        np.testing.assert_allclose(w.cpu().numpy(), po.weights(want, idx.cpu().numpy(), po.beta_after(k)), rtol=2e-6)
        assert (w.cpu().numpy() > 0).all() and (w.cpu().numpy() <= 1).all()
    info = eng.per_info(0)
    assert info["samples"] == k and info["total"] == want[1, 0] and info["p_min"] == want[1, 1]


@pytest.mark.parametrize("count", [257, 1000, 2048])
def test_sampler_bit_exact_over_several_workgroups(count):
    """k_per_sample runs ceil(count / 256) workgroups per agent: two with the
    second holding one sample, four with a ragged last one, eight full ones.
    Injected uniforms and the device's own draw give the oracle's positions and
    weights, and the LAST workgroup to finish advances beta and the sample
    counter once per call, not once per workgroup."""
    cap, seed = 4096, 0x0BAD_5EED_1234
    rng = np.random.default_rng(count)
    eng = _engine(cap, seed=seed)
    P = po.tree_leaves(cap)
    prio = (rng.uniform(0.02, 1.0, cap).astype(F32) ** F32(2.5)).astype(F32)
    _set(eng, 0, np.arange(cap), prio)
    want = po.build(prio, P)
    assert _same_bits(eng.per_tree(0), want)
    k = 0
    draws = [np.minimum(rng.uniform(0, 1, count).astype(F32), TOP), None, np.zeros(count, F32),
             np.full(count, TOP, F32), None]
    for u in draws:
        idx, w = eng.per_sample(0, count, u=None if u is None else torch.from_numpy(u))
        if u is None:                                           # the device's own Philox draw of call k
            u = po.device_uniforms(seed, 0, k, count)
        k += 1
        idx, w = idx.cpu().numpy(), w.cpu().numpy()
        assert (idx == po.sample(want, count, u)).all(), k
        np.testing.assert_allclose(w, po.weights(want, idx, po.beta_after(k)), rtol=2e-6)
        info = eng.per_info(0)
        assert info["samples"] == k and info["beta"] == po.beta_after(k), (k, info)
    assert _same_bits(eng.per_tree(0), want)                    # sampling writes no node


@pytest.mark.parametrize("cap", [37, 4096])
def test_partial_fill_one_leaf_equal_priorities_and_repeats(cap):
    rng = np.random.default_rng(cap)
    P = po.tree_leaves(cap)
    # len < capacity: no index >= len, whatever u
    ln = cap // 3
    eng = _engine(cap, n_rows=ln)
    prio = rng.uniform(0.01, 1.0, ln).astype(F32)
    _set(eng, 0, np.arange(ln), prio)
    want = po.build(prio, P)
    assert _same_bits(eng.per_tree(0), want)
    for B in (16, 40):
        for u in (np.zeros(B, F32), np.full(B, TOP, F32), np.minimum(rng.uniform(0, 1, B).astype(F32), TOP)):
            idx = eng.per_sample(0, B, u=torch.from_numpy(u))[0].cpu().numpy()
            assert (idx == po.sample(want, B, u)).all() and idx.max() < ln and idx.min() >= 0
    # all-equal priorities: weights exactly 1
    _set(eng, 0, np.arange(ln), np.full(ln, 0.25, F32))
    want = po.build(np.full(ln, 0.25, F32), P)
    assert _same_bits(eng.per_tree(0), want)
    u = np.minimum(rng.uniform(0, 1, 40).astype(F32), TOP)
    idx, w = eng.per_sample(0, 40, u=torch.from_numpy(u))
    assert (idx.cpu().numpy() == po.sample(want, 40, u)).all() and (w.cpu().numpy() == 1).all()
    # repeated positions in one call (the same row, the same value)
    pos = np.array([3, 5, 3, 3, 5, 0, ln - 1, ln - 1], np.int32)
    val = np.array([0.5, 0.125, 0.5, 0.5, 0.125, 0.75, 0.0625, 0.0625], F32)
    _set(eng, 0, pos, val)
    p2 = np.full(ln, 0.25, F32)
    p2[pos] = val
    assert _same_bits(eng.per_tree(0), po.build(p2, P))
    # ... and with different values the largest one wins, whatever the order
    _set(eng, 0, [7, 2, 7, 7, 2], [0.25, 0.875, 0.75, 0.5, 0.0625])
    p2[7], p2[2] = 0.75, 0.875
    assert _same_bits(eng.per_tree(0), po.build(p2, P))
    # one filled leaf
    one = _engine(cap, n_rows=1)
    _set(one, 0, [0], [0.3])
    assert _same_bits(one.per_tree(0), po.build(np.array([0.3], F32), P))
    idx, w = one.per_sample(0, 16, u=torch.from_numpy(np.linspace(0, TOP, 16).astype(F32)))
    assert (idx.cpu().numpy() == 0).all() and (w.cpu().numpy() == 1).all()


def test_update_errors_makes_the_documented_priority():
    eng = _engine(64)
    err = np.array([0.0, 0.004, 0.3, 0.99, 1.0, 7.5], F32)
    eng.per_update_errors(0, torch.arange(6, dtype=torch.int32), torch.from_numpy(err))
    leaves = eng.per_tree(0)[64:70, 0]
    np.testing.assert_allclose(leaves, po.priority_from_error(err), rtol=1e-6)
    assert leaves[4] == 1.0 and leaves[5] == 1.0
    full = np.ones(64, F32)
    full[:6] = leaves
    assert _same_bits(eng.per_tree(0), po.build(full, 64))


# ------------------------------------------------------------ device noise
def test_device_noise_is_the_documented_philox_draw():
    seed = 0x1234_5678_9ABC
    eng = _engine(64, n_rows=50, dims=(6, 5), B=16, seed=seed)
    rng = np.random.default_rng(3)
    for agent in (0, 1):
        prio = rng.uniform(0.05, 1.0, 50).astype(F32)
        _set(eng, agent, np.arange(50), prio)
        t = po.build(prio, 64)
        for call in range(2):                                   # the counter advances
            idx = eng.per_sample(agent, 16)[0].cpu().numpy()
            u = po.device_uniforms(seed, agent, call, 16)
            assert (idx == po.sample(t, 16, u)).all(), (agent, call)


def test_distribution_of_the_device_draw():
    rng = np.random.default_rng(2)
    eng = _engine(64, n_rows=50, B=16, seed=99)
    prio = po.priority_from_error(rng.exponential(0.3, 50).astype(F32))
    _set(eng, 0, np.arange(50), prio)
    t = po.build(prio, 64)
    B, draws = 256, 200
    counts = np.zeros(64)
    idx = torch.cat([eng.per_sample(0, B)[0] for _ in range(draws)]).cpu().numpy()
    counts = np.bincount(idx, minlength=64).astype(float)
    N = B * draws
    p = t[64:, 0].astype(np.float64) / float(t[1, 0])
    z = np.abs(counts[:50] - N * p[:50]) / np.sqrt(N * p[:50] * (1 - p[:50]))
    print(f"worst |count - N p| / sigma = {z.max():.2f}")
    assert (counts[50:] == 0).all()
    assert z.max() < 4.0


def test_beta_advances_and_saturates():
    eng = _engine(37, per_beta0=0.4, per_beta_inc=0.125)
    for k in range(1, 8):
        eng.per_sample(0, 16)
        assert eng.per_info(0)["beta"] == po.beta_after(k, F32(0.4), F32(0.125)), k
    assert eng.per_info(0)["beta"] == 1.0 and eng.per_info(0)["samples"] == 7
    eng = _engine(37)
    for k in range(1, 4):
        eng.per_sample(0, 16)
        assert eng.per_info(0)["beta"] == po.beta_after(k)


# ------------------------------------------------------ weighted update
def _loaded_engine(c, dims, B, L, H, **kw):
    from maddpg_amd.engine import Engine
    eng = Engine(dims, c["local_q"], num_units=H, batch_size=B, capacity=L + 7, **kw)
    eng.add_rows(torch.from_numpy(joint_rows(c["data"], dims)))
    for i, p in enumerate(c["params"]):
        for w in ("actor", "critic", "tgt_actor", "tgt_critic"):
            eng.set_params(i, w, p[w])
    return eng


@pytest.mark.parametrize("dims,B,L,H,local_q", [
    ([8, 10, 10], 40, 300, 64, None),
    ([8, 10, 10], 40, 300, 64, [True, False, False]),
    ([16, 16, 16, 14], 48, 300, 64, None),
    ([8, 10, 10], 40, 300, 128, None),
    ([8, 10, 10], 272, 1200, 64, None),      # two sampling workgroups, the second ragged (16 of 256)
])
def test_weighted_update_parity(dims, B, L, H, local_q):
    from tests.test_gpu_parity import _device_grads
    c = synthetic_trainer_case(dims, B, L, 21, local_q, H)
    n = len(dims)
    eng = _loaded_engine(c, dims, B, L, H, prioritized=True)
    P = po.tree_leaves(L + 7)
    rng = np.random.default_rng(8)
    agents = [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][i]) for i, p in enumerate(c["params"])]
    for i in range(n):
        prio = rng.uniform(0.05, 1.0, L).astype(F32)
        _set(eng, i, np.arange(L), prio)
        tree = po.build(prio, P)
        idx = c["idx"][i]
        w = po.weights(tree, idx, po.beta_after(1))
        eng.update(i, idx=torch.from_numpy(idx), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                   u_act=torch.from_numpy(c["u_act"][i]))
        got = eng.stats(i)
        s_idx, s_w, s_td = (x.cpu().numpy() for x in eng.per_slots(i))
        assert (s_idx == idx).all()
        np.testing.assert_allclose(s_w, w, rtol=2e-6)
        batch_n = [tuple(x[idx] for x in c["data"][j]) for j in range(n)]
        want, og, st = po.update_batch(agents, i, batch_n, c["u_tgt"][i], c["u_act"][i], w)
        conditioned = {}
        for net, name in ((1, "grad_critic"), (0, "grad_actor")):
            dg = _device_grads(eng, i, net)
            for k, ref in og[name].items():
                ref = np.asarray(ref, np.float64).reshape(dg[k].shape)
                scale = float(np.abs(ref).max()) or 1.0
                assert float(np.abs(dg[k] - ref).max()) / scale < 1e-5, (i, name, k)
                conditioned[(net, k)] = np.abs(ref) > 1e-3 * scale
        assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]) + 1e-7, (got[0], want[0])
        np.testing.assert_allclose(got[1:], want[1:], rtol=2e-5, atol=2e-6)
        for wn, ref in (("actor", agents[i].actor), ("critic", agents[i].critic),
                        ("tgt_actor", agents[i].tgt_actor), ("tgt_critic", agents[i].tgt_critic)):
            dev = eng.get_params(i, wn)
            for k in ref:
                err = np.abs(dev[k] - ref[k].reshape(dev[k].shape))
                if wn in ("actor", "critic"):      # where Adam is well-conditioned (tests/test_gpu_parity.py)
                    m = conditioned[(1 if wn == "critic" else 0, k)].reshape(err.shape)
                    assert (float(err[m].max()) if m.any() else 0.0) < 1e-6, (i, wn, k)
                assert err.max() < 2e-4, (i, wn, k)
        # |TD error| out of the critic step and the priorities written back from it
        tol = 1e-5 * np.maximum(np.maximum(np.abs(st["q"]), np.abs(st["y"])), 1.0)
        assert (np.abs(s_td - st["td"]) <= tol).all()
        leaves = eng.per_tree(i)[P:P + L, 0]
        want_p = np.zeros(L, F32)                 # a row drawn twice keeps the larger of its priorities
        np.maximum.at(want_p, idx, po.priority_from_error(s_td))
        np.testing.assert_allclose(leaves[idx], want_p[idx], rtol=1e-6)
        after = prio.copy()
        after[idx] = leaves[idx]
        assert _same_bits(eng.per_tree(i), po.build(after, P))
        assert eng.per_info(i)["beta"] == po.beta_after(1)


@pytest.mark.parametrize("H", [64, 128])
def test_weights_of_one_are_free(H):
    """beta0 = 0, beta_inc = 0: every weight is exactly 1.0 and an update on a PER
    engine is bitwise the plain engine's"""
    dims, B, L = [8, 10, 10], 40, 300
    c = synthetic_trainer_case(dims, B, L, 4, None, H)
    plain = _loaded_engine(c, dims, B, L, H)
    per = _loaded_engine(c, dims, B, L, H, prioritized=True, per_beta0=0.0, per_beta_inc=0.0)
    rng = np.random.default_rng(1)
    for i in range(3):
        _set(per, i, np.arange(L), rng.uniform(0.05, 1.0, L).astype(F32))
    for i in range(3):
        for eng in (plain, per):
            eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                       u_act=torch.from_numpy(c["u_act"][i]))
        assert (per.per_slots(i)[1].cpu().numpy() == 1.0).all()
    plain.synchronize()
    per.synchronize()
    for name in ("theta", "target", "adam_m", "adam_v", "beta", "stats"):
        a, b = plain.region(name, torch.int32).cpu().numpy(), per.region(name, torch.int32).cpu().numpy()
        assert (a == b).all(), name


# -------------------------------------------------------------- ring sync
def _spread(E=16, cap=48, B=16, **kw):
    from maddpg_amd.runner import VecRunner
    return VecRunner("simple_spread", E, batch_size=B, capacity=cap, seed=3, prioritized=True, **kw)


def _ring_sync_steps(cap, steps=5):
    """env steps of E = 16 rows on a ring of `cap`: after each one every tree is
    po.build of the expected leaves -- the step's rows at the new-row priority,
    every other leaf as it was -- with priorities injected at random filled
    positions in between.  Returns the ring heads the steps left."""
    r = _spread(cap=cap)
    eng, E, P = r.eng, 16, 64
    rng = np.random.default_rng(0)
    ln, head, heads = 0, 0, []
    prio = [np.zeros(cap, F32) for _ in range(3)]
    for step in range(steps):
        eng.env_step()
        new = (head + np.arange(E)) % cap
        ln, head = min(cap, ln + E), (head + E) % cap
        heads.append(head)
        for a in range(3):
            prio[a][new] = 1.0                                   # the new-row priority
            assert _same_bits(eng.per_tree(a), po.build(prio[a][:ln], P)), (step, a)
        assert eng.per_info(0)["rows_synced"] == E * (step + 1)
        for a in range(3):                                       # injected priorities the next sync must keep
            pos = rng.choice(ln, size=10, replace=False).astype(np.int32)
            val = rng.uniform(0.05, 0.9, 10).astype(F32)
            _set(eng, a, pos, val)
            prio[a][pos] = val
    # at least `capacity` rows between two syncs: every filled leaf is new again
    for _ in range(3):
        eng.env_step()
    for a in range(3):
        assert _same_bits(eng.per_tree(a), po.build(np.ones(cap, F32), P))
    return heads


def test_ring_sync_resets_exactly_the_rewritten_positions():
    assert _ring_sync_steps(48) == [16, 32, 0, 16, 32]


def test_ring_sync_new_rows_wrap_past_the_ring_end():
    """capacity 40: the third step's rows are positions 32..39 and 0..7, the
    fifth's 24..39 -- k_per_sync's two-run branch (n1 > 0), which the
    capacity-48 ring (heads at multiples of 16) never takes"""
    assert _ring_sync_steps(40) == [16, 32, 8, 24, 0]


def test_ring_sync_env_step_and_host_rows_between_two_syncs():
    """an env step (16 rows) and a host add_rows (5 rows) with no sync between
    them: arrived = E + rows = 21 positions behind the head, 32..39 and 0..12
    on a ring of 40 -- those and no others go back to the new-row priority"""
    cap, E, P, rows = 40, 16, 64, 5
    r = _spread(cap=cap)
    eng = r.eng
    rng = np.random.default_rng(1)
    eng.env_step()
    eng.env_step()
    prio = [rng.uniform(0.05, 0.9, cap).astype(F32) for _ in range(3)]
    for a in range(3):
        _set(eng, a, np.arange(32), prio[a][:32])
        assert _same_bits(eng.per_tree(a), po.build(prio[a][:32], P))
    assert eng.per_info(0)["rows_synced"] == 2 * E
    eng.env_step()                                               # head 32 -> 8: no sync of its own
    eng.add_rows(torch.from_numpy(rng.normal(size=(rows, eng.row_stride)).astype(F32)))   # head 8 -> 13
    assert eng.buffer_len() == cap
    new = np.r_[32:40, 0:13]
    for a in range(3):
        prio[a][new] = 1.0
        assert _same_bits(eng.per_tree(a), po.build(prio[a], P)), a
    assert eng.per_info(0)["rows_synced"] == 2 * E + E + rows


# ---------------------------------------------------------- graph == eager
def _fingerprint(eng):
    eng.synchronize()
    out = {k: eng.region(k, torch.int32).cpu().numpy().copy() for k in ("theta", "target", "adam_m", "adam_v", "beta")}
    out["rng"] = eng.get_rng_state()
    out["ctl"] = eng.region("ctl", torch.int32).cpu().numpy().copy()
    for a in range(eng.n):
        out[f"tree{a}"] = eng.per_tree(a).copy()
        out[f"beta{a}"] = np.array([eng.per_info(a)["beta"], eng.per_info(a)["samples"]])
    return out


def _run(graphs, how, **kw):
    # (simple_spread's TD errors exceed the default clip of 1: a wide clip keeps the priorities apart)
    r = _spread(max_episode_len=5, per_abs_err_upper=1000.0, **kw)
    eng = r.eng
    eng.set_graphs(graphs)
    ks = [0, 0, 0, 0, 0, 2, 1, 2]
    for rep in range(3):                                         # the first training step runs eagerly; then replays
        if how == "train_steps":
            eng.train_steps(ks)
        else:
            for k in ks:
                eng.env_step()
                for _ in range(k):
                    eng.update_round()
    return _fingerprint(eng)


@pytest.mark.parametrize("how", ["train_steps", "update_round"])
def test_graph_replay_equals_eager(how):
    a, b = _run(True, how), _run(False, how)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # the trees moved: priorities were written back
    assert len(np.unique(a["tree0"][64:112, 0])) > 8
    assert a["beta0"][1] == 15                                   # 3 x 5 rounds, one sample call each


@pytest.mark.parametrize("how", ["train_steps", "update_round"])
def test_graph_replay_equals_eager_two_sample_workgroups(how):
    """the same at B = 272: every agent's draw is two k_per_sample workgroups
    (the second ragged), whose ticket must leave beta and the sample counter
    the same in a replayed graph as in the eager run; the ring of 300 wraps in
    the third repetition (3 x 128 rows)"""
    a, b = _run(True, how, B=272, cap=300), _run(False, how, B=272, cap=300)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert len(np.unique(a["tree0"][512:812, 0])) > 8            # priorities were written back
    assert a["beta0"][1] == 15 and a["beta0"][0] == po.beta_after(15)


def test_train_steps_equals_update_round():
    a, b = _run(True, "train_steps"), _run(True, "update_round")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# --------------------------------------------------------------- refusals
def _refused(eng, name, *args):
    rc = getattr(eng.lib, name)(eng.h, *args)
    msg = eng.lib.mdp_last_error(eng.h).decode()
    assert rc < 0 and len(msg) > 10, (name, rc, msg)
    return msg


def test_refusals():
    from maddpg_amd import _lib
    from maddpg_amd.engine import Engine
    eng = _engine(64)
    dev = lambda n, dt: torch.zeros(n, dtype=dt, device=eng.device)  # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    host = np.zeros(64, F32)
    hp = ctypes.c_void_p(host.ctypes.data)
    i16, f16 = dev(16, torch.int32), dev(16, torch.float32)
    before = eng.per_tree(0).copy(), eng.per_info(0)
    for args in ((0, 16, hp, p(i16), p(f16)), (0, 16, None, hp, p(f16)), (0, 16, None, p(i16), hp)):
        assert "not device memory" in _refused(eng, "mdp_per_sample", *args)
    for fn in ("mdp_per_set_priorities", "mdp_per_update_errors"):
        for args in ((0, hp, p(f16), 16), (0, p(i16), hp, 16)):
            assert "not device memory" in _refused(eng, fn, *args)
    after = eng.per_tree(0), eng.per_info(0)
    assert _same_bits(before[0], after[0]) and before[1] == after[1]          # nothing was launched
    # enable: a host pointer, a short buffer, twice
    plain = Engine([6], batch_size=16, capacity=64)
    nb = plain.lib.mdp_per_bytes(ctypes.byref(plain.cfg))
    buf = torch.empty(nb, dtype=torch.uint8, device=plain.device)
    hbuf = np.zeros(nb, np.uint8)
    en = (0.6, 0.4, 0.001, 0.01, 1.0)
    _refused(plain, "mdp_per_enable", ctypes.c_void_p(hbuf.ctypes.data), nb, *en)
    _refused(plain, "mdp_per_enable", p(buf), nb - 8, *en)
    assert "not enabled" in _refused(plain, "mdp_per_get_tree", 0, host.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    _refused(eng, "mdp_per_enable", p(buf), nb, *en)                          # already enabled
    # enable after the first update
    plain.add_rows(torch.zeros(32, plain.row_stride))
    plain.update(0)
    assert "before" in _refused(plain, "mdp_per_enable", p(buf), nb, *en)
    # throughput mode, both orders
    with pytest.raises(_lib.MdpError, match="strict"):
        eng.set_update_mode("throughput")
    tp = Engine([6], batch_size=16, capacity=64)
    tp.set_update_mode("throughput")
    assert "strict" in _refused(tp, "mdp_per_enable", p(buf), nb, *en)
    # data parallelism
    with pytest.raises(_lib.MdpError, match="one GPU"):
        Engine([6], batch_size=16, capacity=64, world_size=2, prioritized=True)
    assert "one GPU" in _refused(eng, "mdp_dp_init", bytes(128), 2, 0)
    assert "one GPU" in _refused(eng, "mdp_dp_xgmi_open", 2, 0, ctypes.create_string_buffer(64))


def test_short_device_buffers_refused():
    """15 of the 16 elements at the very end of a hipMalloc allocation, to every new
    entry point that takes a device buffer.  Run where the runtime reports an
    allocation's exact extent (the library checks with the same hipMemGetAddressRange)."""
    eng = _engine(64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    i16 = torch.zeros(16, dtype=torch.int32, device=eng.device)
    f16 = torch.zeros(16, dtype=torch.float32, device=eng.device)
    before = eng.per_tree(0).copy(), eng.per_info(0)
    nbytes, base = 4 << 20, ctypes.c_void_p()
    assert eng.lib.hipMalloc(ctypes.byref(base), ctypes.c_size_t(nbytes)) == 0
    try:
        rb, ext = ctypes.c_void_p(), ctypes.c_size_t()
        exact = (eng.lib.hipMemGetAddressRange(ctypes.byref(rb), ctypes.byref(ext), base) == 0
                 and rb.value == base.value and ext.value == nbytes)
        if not exact:
            pytest.skip(f"runtime reports extent {ext.value} for a {nbytes}-byte allocation")
        tail = ctypes.c_void_p(base.value + nbytes - 4 * 15)
        for args in ((0, 16, tail, p(i16), p(f16)), (0, 16, None, tail, p(f16)), (0, 16, None, p(i16), tail)):
            assert "allocation too small" in _refused(eng, "mdp_per_sample", *args)
        for fn in ("mdp_per_set_priorities", "mdp_per_update_errors"):
            for args in ((0, tail, p(f16), 16), (0, p(i16), tail, 16)):
                assert "allocation too small" in _refused(eng, fn, *args)
        # the enable call: a buffer that ends before mdp_per_bytes
        from maddpg_amd.engine import Engine
        plain = Engine([6], batch_size=16, capacity=64)
        nb = plain.lib.mdp_per_bytes(ctypes.byref(plain.cfg))
        assert nb < nbytes
        short = ctypes.c_void_p(base.value + nbytes - (nb - 256))
        assert "allocation too small" in _refused(plain, "mdp_per_enable", short, nb, 0.6, 0.4, 0.001, 0.01, 1.0)
    finally:
        torch.cuda.synchronize()
        assert eng.lib.hipFree(base) == 0
    after = eng.per_tree(0), eng.per_info(0)
    assert _same_bits(before[0], after[0]) and before[1] == after[1]          # nothing was launched


def test_rows_without_a_priority_get_weight_zero():
    """given rows at or beyond the ring length (unfilled leaves) weigh 0 and are not
    marked filled by the write-back; a zero priority weighs 0 too"""
    eng = _engine(64, n_rows=20)
    _set(eng, 0, [3], [0.0])
    before = eng.per_tree(0).copy()
    idx = torch.tensor([0, 3, 25, 63, 1] + [2] * 11, dtype=torch.int32)
    eng.init_params(0)
    eng.update(0, idx=idx)
    s_idx, s_w, s_td = (x.cpu().numpy() for x in eng.per_slots(0))
    assert (s_idx == idx.numpy()).all()
    assert np.isfinite(s_w).all() and (s_w[[1, 2, 3]] == 0).all() and (s_w[[0, 4, 5]] > 0).all()
    after = eng.per_tree(0)
    assert (after[64 + 20:] == before[64 + 20:]).all()           # unfilled leaves stay {0, +inf}
    assert np.isfinite(after[1, 0]) and after[1, 0] > 0


def test_new_row_priority_is_the_clipped_priority():
    """abs_err_upper ** alpha of a new row is bitwise the priority of a trained row at the clip"""
    eng = _engine(64, per_abs_err_upper=2.5, per_alpha=0.7)
    fresh = eng.per_tree(0)[64:, 0].copy()
    assert (fresh == fresh[0]).all() and abs(float(fresh[0]) - 2.5 ** 0.7) < 1e-5
    eng.per_update_errors(0, torch.tensor([5], dtype=torch.int32), torch.tensor([100.0]))
    assert eng.per_tree(0)[64 + 5, 0] == fresh[0]


# ----------------------------------------------------------------- facade
def test_prioritized_replay_memory_facade():
    from maddpg_amd.trainer.prioritized_replay_buffer import PrioritizedReplayMemory
    rng = np.random.default_rng(0)
    mem = PrioritizedReplayMemory(128)
    rows = []
    for k in range(100):
        row = (rng.normal(size=7), rng.normal(size=5).astype(np.float32), float(rng.normal()), rng.normal(size=7),
               bool(k % 9 == 0))
        rows.append(row)
        mem.add(*row)
    assert len(mem) == 100
    b_idx, b_memory, w = mem.sample(32)
    assert len(b_idx) == 32 and len(w) == 32 and isinstance(b_memory, (tuple, list)) and len(b_memory) == 5
    assert all(0 <= i < 100 for i in b_idx) and all(x == 1.0 for x in w)      # every new row at the top priority
    obs, act, rew, obs1, done = b_memory
    for j, i in enumerate(b_idx):
        np.testing.assert_allclose(obs[j], rows[i][0].astype(np.float32), rtol=0, atol=0)
        np.testing.assert_allclose(act[j], rows[i][1])
        assert rew[j] == np.float32(rows[i][2]) and done[j] == float(rows[i][4])
        np.testing.assert_allclose(obs1[j], rows[i][3].astype(np.float32))
    before = mem.priorities()
    assert (before == 1.0).all()
    err = rng.uniform(0, 0.5, 32).astype(np.float32)
    _, first = np.unique(b_idx, return_index=True)               # one error per distinct row
    mem.batch_update([b_idx[j] for j in first], err[first])
    after = mem.priorities()
    moved = np.zeros(100, bool)
    moved[[b_idx[j] for j in first]] = True
    assert (after[~moved] == 1.0).all()
    np.testing.assert_allclose(after[[b_idx[j] for j in first]], po.priority_from_error(err[first]), rtol=1e-6)
    assert abs(mem.beta - 0.401) < 1e-6


def test_facade_ring_wrap_resets_overwritten_rows():
    """rows added through the facade between two syncs: more than the capacity (with a
    remainder), exactly the capacity, and a few -- overwritten rows never keep the old priority"""
    from maddpg_amd.trainer.prioritized_replay_buffer import PrioritizedReplayMemory
    rng = np.random.default_rng(1)
    cap = 32
    mem = PrioritizedReplayMemory(cap)
    add = lambda k: [mem.add(rng.normal(size=4), rng.normal(size=5), 0.0, rng.normal(size=4), False)  # noqa: E731
                     for _ in range(k)]
    lower = lambda: mem.batch_update(list(range(len(mem))), np.full(len(mem), 0.05, np.float32))  # noqa: E731
    low = po.priority_from_error(np.float32(0.05))
    add(20)
    lower()
    assert (mem.priorities() == low).all()
    add(cap + 5)                                   # wraps once, remainder 5
    assert len(mem) == cap and (mem.priorities() == 1.0).all()
    lower()
    add(cap)                                       # the ring state looks unchanged
    assert (mem.priorities() == 1.0).all()
    lower()
    add(3)                                         # positions 25, 26, 27 only
    want = np.full(cap, low, np.float32)
    want[[25, 26, 27]] = 1.0
    assert (mem.priorities() == want).all()


def test_facade_new_rows_wrap_past_the_ring_end():
    """a few rows added between two syncs that cross the end of the ring (fewer than
    the capacity: no full reset): exactly positions 30, 31, 0, 1, 2 are new"""
    from maddpg_amd.trainer.prioritized_replay_buffer import PrioritizedReplayMemory
    rng = np.random.default_rng(2)
    cap = 32
    mem = PrioritizedReplayMemory(cap)
    add = lambda k: [mem.add(rng.normal(size=4), rng.normal(size=5), 0.0, rng.normal(size=4), False)  # noqa: E731
                     for _ in range(k)]
    low = po.priority_from_error(np.float32(0.05))
    add(30)
    mem.batch_update(list(range(30)), np.full(30, 0.05, np.float32))
    assert len(mem) == 30 and (mem.priorities() == low).all()
    add(5)
    assert len(mem) == cap
    want = np.full(cap, low, np.float32)
    want[[30, 31, 0, 1, 2]] = 1.0
    assert (mem.priorities() == want).all()
