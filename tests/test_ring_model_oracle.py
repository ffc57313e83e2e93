"""CPU: the host model of the replay ring and the episode log (tests/ring_model.py)
against ``oracle/replay.py``, a one-row-at-a-time ring, CPython's ``random.Random``
and ``struct Ctl`` -- and the conditions under which the GPU comparisons of
tests/test_ring_log_wrap_gpu.py can fail: they are asserted here, not assumed.
"""
import itertools
import os
import random

import numpy as np
import pytest

from oracle.replay import ReplayBuffer
from tests import ring_model as rm

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 4


def _serial(first, k, stride=STRIDE):
    """k rows that carry their own serial number (from `first`) in every column"""
    return np.repeat(np.arange(first, first + k, dtype=F32)[:, None], stride, 1)


def _sizes(cap):
    return [0, 1, cap - 1, cap, cap + 1, 2 * cap + 3]


# ------------------------------------------------------------------ the ring
@pytest.mark.parametrize("cap", [1, 2, 7, 50])
def test_ring_model_equals_oracle_replay_buffer(cap):
    """the same appends into oracle.replay.ReplayBuffer (add once per row) and into the
    model, from a head moved off 0, every order of the call sizes around cap"""
    orders = list(itertools.permutations(_sizes(cap)))
    rng = np.random.default_rng(cap)
    for pick in rng.choice(len(orders), size=12, replace=False):
        ref, ring, serial = ReplayBuffer(cap), rm.RingModel(cap, STRIDE), 1
        for k in [min(3, cap)] + list(orders[pick]):     # the first call moves the head
            rows = _serial(serial, k)
            serial += k
            for r in rows:
                ref.add(r, None, None, None, None)
            ring.append(rows)
            assert (ring.len, ring.next) == (len(ref), ref._next_idx)
            got = np.stack([s[0] for s in ref._storage]) if len(ref) else np.zeros((0, STRIDE), F32)
            assert np.array_equal(ring.storage[:ring.len], got)
            assert np.all(ring.storage[ring.len:] == 0)


@pytest.mark.parametrize("cap", [1, 3, 50])
def test_ring_model_equals_one_row_at_a_time_ring(cap):
    """from any valid (len, next), set included: a ring written one row at a time"""
    rng = np.random.default_rng(100 + cap)
    for _ in range(20):
        length, nxt = int(rng.integers(0, cap + 1)), int(rng.integers(0, cap))
        ring = rm.RingModel(cap, STRIDE)
        ring.append(_serial(1000, cap))                  # something under the moved head
        ring.set(length, nxt)
        store = ring.storage.copy()
        serial = 1
        for k in rng.permutation(_sizes(cap)):
            rows = _serial(serial, int(k))
            serial += int(k)
            for r in rows:
                store[nxt] = r
                nxt = (nxt + 1) % cap
                length = min(cap, length + 1)
            ring.append(rows)
            assert (ring.len, ring.next) == (length, nxt)
            assert np.array_equal(ring.storage, store)


def test_ring_model_lazy_stride_and_unwritten_rows():
    ring = rm.RingModel(5)
    assert ring.storage.shape == (5, 0)
    ring.append(_serial(1, 2, 3))
    assert ring.storage.shape == (5, 3) and np.all(ring.storage[2:] == 0) and ring.storage.dtype == F32


# ------------------------------------------------------------------- the log
def test_log_model_read_across_the_wrap_and_refusals():
    rows, n = 10, 3
    log = rm.LogModel(rows, n)
    ent = np.arange(27 * (1 + n), dtype=F32).reshape(27, 1 + n)
    with pytest.raises(IndexError):
        log.read(0, 1)                                   # nothing written yet
    assert log.read(0, 0).shape == (0, 1 + n)
    log.append(ent[:4])
    assert np.array_equal(log.read(0, 4), ent[:4]) and np.all(log.storage[4:] == 0)
    log.append(ent[4:27])
    assert log.count == 27                               # live: entries 17 .. 26, the wrap between 19 and 20
    for c in range(17, 27):
        assert np.array_equal(log.storage[c % rows], ent[c])
    for first, k in [(17, 3), (20, 7), (18, 5), (17, 10), (22, 0), (27, 0)]:
        assert np.array_equal(log.read(first, k), ent[first:first + k])
    for first, k in [(16, 1), (16, 10), (26, 2), (27, 1), (-1, 1), (17, 11), (0, 1), (20, -1)]:
        with pytest.raises(IndexError):
            log.read(first, k)


def test_episode_sums_is_the_step_order_fp32_sum():
    """1e8, 1, -1e8, 1 per step: the step-order fp32 sum is 1 (1e8 + 1 rounds to 1e8),
    fp64 or a pairwise order gives 2, the reverse order 0"""
    rew = np.array([[1e8, 3.0], [1.0, 0.5], [-1e8, 0.25], [1.0, 1.0]], F32)
    got = rm.episode_sums(rew)
    assert got.dtype == F32 and got.shape == (3,)
    assert got[1] == F32(1.0) and got[2] == F32(4.75)
    assert float(np.sum(rew[:, 0].astype(np.float64))) == 2.0
    assert rm.episode_sums(rew[::-1])[1] == F32(0.0)
    assert got[0] == F32(F32(0) + got[1]) + got[2]
    # tot adds the agents' sums in agent order, in fp32
    three = np.array([[1e8, 1.0, -1e8]], F32)
    assert rm.episode_sums(three)[0] == F32(0.0) and float(three.astype(np.float64).sum()) == 1.0


# ------------------------------------------------------------ the index draw
@pytest.mark.parametrize("length", [1, 2, 16, 83, 624, 65537])
def test_mt_restatement_equals_cpython_random(length):
    g = random.Random(length)
    for _ in range(length % 7):
        g.random()
    before = np.array(g.getstate()[1], np.uint32)
    idx, after = rm.mt_draws(before, length, 700)        # crosses a twist
    assert list(idx) == [g.randint(0, length - 1) for _ in range(700)]
    assert np.array_equal(after, np.array(g.getstate()[1], np.uint32))
    assert np.array_equal(rm.mt_state_after(before, length, 700), after)


def test_r4_fill_levels_distinguish_the_draw_length():
    """At every R4 fill level the MT state after the round's n B draws against the
    post-step length differs from the state after draws against the pre-step length
    (where the two lengths differ: at len == cap they are the same number) and, where
    len + E > cap, from the state after draws against the uncapped len + E: a step
    that drew against either wrong length cannot leave the state R4 expects."""
    c = rm.R4
    E, cap, nb = c["E"], c["cap"], c["n"] * c["B"]
    start = np.array(random.Random(c["py_seed"]).getstate()[1], np.uint32)
    chain = rm.r4_chain(start)
    assert [(ln + E < cap, ln + E == cap, ln + E > cap and ln < cap, ln == cap) for ln, _, _, _ in chain[1:]] == \
        [(True, False, False, False), (False, True, False, False), (False, False, True, False),
         (False, False, False, True)]
    seen = 0
    for length, nxt, before, after in chain:
        post = rm.draw_length(length, E, cap)
        assert post == min(cap, length + E) and 0 <= nxt < cap
        if 0 < length != post:
            assert not np.array_equal(after, rm.mt_state_after(before, length, nb)), length
            seen += 1
        if length + E > cap:
            assert not np.array_equal(after, rm.mt_state_after(before, length + E, nb)), length
            seen += 1
    assert seen == 3 + 2     # pre-step length at three levels, the uncapped one at two


# ------------------------------------------------------------- struct Ctl
def test_ctl_offsets_follow_the_struct():
    text = open(os.path.join(ROOT, "maddpg_amd", "csrc", "mdp_topo.h")).read()
    off = rm.ctl_offsets(text)
    assert (off["len"], off["next"], off["env_steps"], off["episodes"], off["ep_pending"], off["upd_ctr"]) == \
        (rm.CTL_LEN, rm.CTL_NEXT, rm.CTL_ENV_STEPS, rm.CTL_EPISODES, rm.CTL_EP_PENDING, rm.CTL_UPD_CTR)
    assert off["mt"] == 0 and off["mt_pos"] == 624 * 4
    # the constant tests/test_gpu_parity.py reads the update counter with
    parity = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    assert f"CTL_UPD_CTR_OFFSET = {off['upd_ctr']}" in parity
    blob = np.zeros(2700, np.uint8)
    blob[rm.CTL_NEXT:rm.CTL_NEXT + 8] = np.array([7], np.int64).view(np.uint8)
    blob[rm.CTL_EP_PENDING:rm.CTL_EP_PENDING + 4] = np.array([9], np.uint32).view(np.uint8)
    got = rm.ctl_read(blob)
    assert got == {"len": 0, "next": 7, "env_steps": 0, "episodes": 0, "ep_pending": 9}


# ------------------------------------------- the GPU cases can fail (mutations)
class _RingModuloCapPlus1(rm.RingModel):
    """the ring rule with the wrong modulus (a row past the end lands in a spare slot)"""

    def __init__(self, cap, stride):
        super().__init__(cap, stride)
        self._store = np.zeros((cap + 1, stride), F32)

    @property
    def storage(self):
        return self._store[:self.cap]

    def _slots(self, first, count):
        return (self.next + first + np.arange(count, dtype=np.int64)) % (self.cap + 1)


def test_mutation_ring_modulo_changes_every_wrapping_case():
    """ring modulo cap + 1: the expectation of every R2 ring and of every R5 ring differs"""
    def run(cls, cap, calls):
        ring, serial = cls(cap, STRIDE), 1
        for k in calls:
            ring.append(_serial(serial, k))
            serial += k
        return ring

    cases = [(cap, [E] * rm.r2_steps(E, cap)) for E in rm.R2["E"] for cap in rm.r2_caps(E)]
    cases += [(cap, [E] * (1 + 2 * k)) for E in rm.R5["E"] for k in rm.R5["k"] for cap in rm.r5_caps(E, k)]
    for cap, calls in cases:
        a, b = run(rm.RingModel, cap, calls), run(_RingModuloCapPlus1, cap, calls)
        assert a.next != b.next or not np.array_equal(a.storage, b.storage), (cap, calls[0], len(calls))


def test_mutation_uncapped_draw_length_changes_r4():
    """draw length len + E without the cap: the RNG state R4 expects differs at both
    levels with len + E > cap, and the uncapped draw holds an index >= cap there"""
    c = rm.R4
    E, cap, nb = c["E"], c["cap"], c["n"] * c["B"]
    start = np.array(random.Random(c["py_seed"]).getstate()[1], np.uint32)
    hit = 0
    for length, _nxt, before, after in rm.r4_chain(start):
        if length + E > cap:
            idx, state = rm.mt_draws(before, length + E, nb)
            assert not np.array_equal(state, after) and idx.max() >= cap
            hit += 1
    assert hit == 2


def _launch_log(log, steps_entries, use_ep_done):
    """the lockstep slot rule of one multi-step launch: ep_base + ep_done + e"""
    base, done = log.count, 0
    for ent in steps_entries:
        for e, row in enumerate(ent):
            log.storage[(base + (done if use_ep_done else 0) + e) % log.rows] = row
        done += len(ent)
    log.count = base + done


def test_mutation_log_slot_without_ep_done_changes_r5():
    """log slot ep_base + e, without the launch's earlier episode ends: the log R5 expects
    differs wherever a launch spans two episode ends (k = 7, 64; k = 2 spans at most one)"""
    T, n = rm.R5["T"], 3
    for E in rm.R5["E"]:
        for k in rm.R5["k"]:
            serial, t = 1, 0
            want, rule, mut = rm.LogModel(2 * E, n), rm.LogModel(2 * E, n), rm.LogModel(2 * E, n)
            for launch in [1, k, k]:
                steps = []
                for _ in range(launch):
                    t += 1
                    ent = np.zeros((0, 1 + n), F32)
                    if t % T == 0:
                        ent = _serial(serial, E, 1 + n)
                        serial += E
                    steps.append(ent)
                for ent in steps:
                    want.append(ent)
                _launch_log(rule, steps, True)
                _launch_log(mut, steps, False)
            assert rule.count == want.count == mut.count and np.array_equal(rule.storage, want.storage)
            assert np.array_equal(mut.storage, want.storage) == (k == 2), (E, k)
