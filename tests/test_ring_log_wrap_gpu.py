"""GPU: the replay ring and the finished-episode log across their wraps, against the
host model of tests/ring_model.py, bit for bit.

Placement is under test, content is not: a *twin* engine with the same seed,
parameters and injected inputs, whose ring and log are large enough never to
wrap, steps one ``env_step`` at a time with graphs off and records the linear
history of rows and log entries (that path is pinned against the oracle by
test_mpe_edges_gpu.py and test_gpu_parity.py).  The engine under test -- small
rings, step graphs, multi-step rollout launches, mixed writers -- must leave in
its rings exactly what ``RingModel`` / ``LogModel`` hold after the twin's
history.  Engines are created with lr = 0 and tau = 0, so a training step leaves
every parameter bit-unchanged and the rows do not depend on what was sampled.

After every call: ``replay_rows(0, cap)`` (unfilled rows exactly zero), the raw
episode log, ``buffer_len()`` (the host's head), and the device's ``Ctl.len`` /
``next`` / ``episodes`` / ``env_steps``, with ``ep_pending == 0``.  DESIGN.md 27.
"""
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd._lib import MdpError  # noqa: E402
from maddpg_amd.engine import Engine  # noqa: E402
from maddpg_amd.envs import spec  # noqa: E402
from tests import ring_model as rm  # noqa: E402
from tests.helpers import row_layout  # noqa: E402
from tests.mpe_edges import _softmax_actions  # noqa: E402

F32 = np.float32
SP = spec("simple_spread")
DIMS, N = SP.obs_dims, 3
LAY, STRIDE = row_layout(DIMS)
REW = [LAY[j]["rew"] for j in range(N)]
SEED, PARAM_SEED = 0x5EED0000A11CE, 4


def _engine(E, cap, T=25, log_rows=0, B=64):
    eng = Engine(DIMS, batch_size=B, capacity=cap, num_envs=E, scenario="simple_spread", max_episode_len=T,
                 seed=SEED, lr=0.0, tau=0.0, episode_log_rows=log_rows)
    assert eng.row_stride == STRIDE
    eng.init_params(PARAM_SEED)
    eng.env_reset()
    return eng


def _acts(E, steps, seed):
    rng = np.random.default_rng(seed)
    return [_softmax_actions(rng, E, N) for _ in range(steps)]


def _ends(E, T, step, ep_step0=None):
    """the envs whose episode ends in step `step` (0-based)"""
    ep0 = np.zeros(E, np.int64) if ep_step0 is None else np.asarray(ep_step0, np.int64)
    return np.flatnonzero((ep0 + step + 1) % T == 0)


def _twin_run(E, steps, T, acts):
    """the linear history: rows[step] [E, stride] and entries[step] [ends, 1 + n] in log order"""
    eng = _engine(E, steps * E, T=T, log_rows=max(2 * E, E * (steps // T + 1)))
    eng.set_graphs(False)
    for s in range(steps):
        eng.env_step(act_in=None if acts is None else torch.from_numpy(acts[s]))
    eng.synchronize()
    assert eng.buffer_len() == steps * E
    rows = eng.replay_rows(0, steps * E).cpu().numpy().reshape(steps, E, STRIDE).copy()
    # a misplaced row cannot hide: no two rows of the history are equal, none is zero
    flat = {r.tobytes() for r in rows.reshape(-1, STRIDE)}
    assert len(flat) == steps * E and bytes(4 * STRIDE) not in flat
    count = eng.episode_count()
    log = eng.episode_log(0, count)
    assert len({e.tobytes() for e in log}) == count       # nor a misplaced log entry
    entries, c = [], 0
    for s in range(steps):
        k = len(_ends(E, T, s))
        entries.append(log[c:c + k])
        c += k
    assert c == count
    rows.setflags(write=False)
    log.setflags(write=False)
    eng.close()
    return rows, entries


@functools.lru_cache(maxsize=None)
def _twin(E, steps, T):
    """the policies' own actions (what train_step plays)"""
    return _twin_run(E, steps, T, None)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _raw_log(eng, rows):
    return eng.region("eplog").cpu().numpy()[:rows * (1 + N)].reshape(rows, 1 + N)


def _check(eng, ring, log, env_steps, what):
    eng.synchronize()
    ctl = rm.ctl_read(eng.region("ctl", torch.uint8).cpu().numpy())
    assert eng.buffer_len() == ring.len, what
    assert (ctl["len"], ctl["next"]) == (ring.len, ring.next), what
    assert ctl["ep_pending"] == 0 and ctl["env_steps"] == env_steps, what
    got = eng.replay_rows(0, ring.cap).cpu().numpy()
    bad = np.flatnonzero(np.any(_bits(got) != _bits(ring.storage), axis=1))
    assert bad.size == 0, (what, "ring rows differ", bad[:8])
    if log is None:
        assert ctl["episodes"] == 0, what
        return
    assert ctl["episodes"] == log.count == eng.episode_count(), what
    bad = np.flatnonzero(np.any(_bits(_raw_log(eng, log.rows)) != _bits(log.storage), axis=1))
    assert bad.size == 0, (what, "log slots differ", bad[:8])


def _serial(first, k):
    return np.repeat(np.arange(first, first + k, dtype=F32)[:, None], STRIDE, 1)


# ------------------------------------------------------------------------ R1
def test_r1_add_rows_from_a_moved_head():
    cap = 50
    eng = Engine(DIMS, batch_size=16, capacity=cap)
    ring, serial = rm.RingModel(cap, eng.row_stride), 1
    for k in (7, 43, 1, 49, 50, 51, 103, 0):
        rows = _serial(serial, k)
        serial += k
        eng.add_rows(torch.from_numpy(rows))
        ring.append(rows)
        _check(eng, ring, None, 0, f"add_rows({k})")


# ------------------------------------------------------------------------ R2
@pytest.mark.parametrize("E", rm.R2["E"])
def test_r2_one_step_rollout_wraps(E):
    """one ragged tile, one full tile, three workgroups with a ragged last; every
    capacity from `the step overwrites the whole ring` to four steps per pass; the
    episode log (2 E rows) wraps on the way"""
    T = rm.R2["T"]
    most = max(rm.r2_steps(E, cap) for cap in rm.r2_caps(E))
    acts = _acts(E, most, 20 + E)
    rows, entries = _twin_run(E, most, T, acts)
    for cap in rm.r2_caps(E):
        eng = _engine(E, cap, T=T, log_rows=2 * E)
        ring, log = rm.RingModel(cap, STRIDE), rm.LogModel(2 * E, N)
        steps = rm.r2_steps(E, cap)
        assert steps * E >= 3 * cap
        for s in range(steps):
            eng.env_step(act_in=torch.from_numpy(acts[s]))
            ring.append(rows[s])
            log.append(entries[s])
            _check(eng, ring, log, s + 1, f"E={E} cap={cap} step {s}")
        eng.close()
    assert log.count == E * (steps // T) > log.rows       # at the largest capacity the log has wrapped


# ------------------------------------------------------------------------ R3
def test_r3_mixed_writers_keep_one_head():
    """env_step (the device's head), add_rows (the host's head) and set_ring (both) in
    one sequence: after each call the two heads equal the model's, so the next writer
    of either kind lands where the model puts it"""
    E, T = 37, 5
    cap = 3 * E + 7
    acts = _acts(E, 5, 77)
    rows, entries = _twin_run(E, 5, T, acts)
    eng = _engine(E, cap, T=T, log_rows=2 * E)
    ring, log = rm.RingModel(cap, STRIDE), rm.LogModel(2 * E, N)
    done = {"steps": 0, "serial": 1}

    def step():
        s = done["steps"]
        eng.env_step(act_in=torch.from_numpy(acts[s]))
        ring.append(rows[s])
        log.append(entries[s])
        done["steps"] += 1
        _check(eng, ring, log, done["steps"], f"env_step {s}")

    def add(k):
        r = _serial(done["serial"], k)
        done["serial"] += k
        eng.add_rows(torch.from_numpy(r))
        ring.append(r)
        _check(eng, ring, log, done["steps"], f"add_rows({k})")

    step()
    step()
    add(9)
    step()                                    # crosses the ring's end: 83 + 37 > 118
    eng.set_ring(60, 100)
    ring.set(60, 100)
    _check(eng, ring, log, done["steps"], "set_ring(60, 100)")
    step()                                    # from the set head, across the end again
    add(cap + 2)
    step()                                    # the lockstep episodes end here: E log entries
    assert log.count == E


# ------------------------------------------------------------------------ R4
def _r4():
    c = rm.R4
    E, B, cap = c["E"], c["B"], c["cap"]
    nb = N * B
    rows, entries = _twin(E, 1 + len(c["levels"]), 25)
    eng = _engine(E, cap, B=B, log_rows=2 * E)
    eng.seed_py_random(c["py_seed"])
    start = np.array(random.Random(c["py_seed"]).getstate()[1], np.uint32)
    chain = rm.r4_chain(start)
    ring, log = rm.RingModel(cap, STRIDE), rm.LogModel(2 * E, N)
    for i, (length, nxt, before, after) in enumerate(chain):
        what = f"len={length} next={nxt}"
        if i:
            eng.set_ring(length, nxt)
            ring.set(length, nxt)
        assert np.array_equal(eng.get_rng_state(), before), what
        eng.train_step(1)                     # i = 0 eager, then the step graph
        ring.append(rows[i])
        log.append(entries[i])
        _check(eng, ring, log, i + 1, what)
        L = rm.draw_length(length, E, cap)
        want_idx, want_state = rm.mt_draws(before, L, nb)
        assert np.array_equal(want_state, after)
        assert np.array_equal(eng.get_rng_state(), after), what
        idx = eng.region("index", torch.int32)[:nb].cpu().numpy()
        assert idx.min() >= 0 and idx.max() < L, (what, int(idx.max()), L)
        # the slot holds exactly the stream's n B draws against that length
        assert np.array_equal(np.sort(idx), np.sort(want_idx)), what
    eng.close()


def test_r4_step_graph_draw_length():
    """the first round's draw inside the rollout launch (len + E < cap ? len + E : cap)"""
    _r4()


def test_r4_step_graph_draw_length_own_launch(monkeypatch):
    monkeypatch.setenv("MDP_ROLLOUT_DRAW", "0")
    _r4()


def test_r4_step_graph_draw_length_general_kernels(monkeypatch):
    monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
    _r4()


# ------------------------------------------------------------------------ R5
@pytest.mark.parametrize("k", rm.R5["k"])
@pytest.mark.parametrize("E", rm.R5["E"])
def test_r5_multi_step_rollout_launches(E, k):
    """train_steps([0] * k): one k_rollout launch of k steps, replayed twice (the second
    replay starts from another head); the log (2 E rows, T = 3) wraps inside a launch"""
    T = rm.R5["T"]
    rows, entries = _twin(E, 1 + 2 * max(rm.R5["k"]), T)
    for cap in rm.r5_caps(E, k):
        eng = _engine(E, cap, T=T, log_rows=2 * E)
        ring, log = rm.RingModel(cap, STRIDE), rm.LogModel(2 * E, N)
        eng.train_step(1)                     # the one eager step: groups are graphs after it
        ring.append(rows[0])
        log.append(entries[0])
        s = 1
        _check(eng, ring, log, s, f"E={E} k={k} cap={cap} eager step")
        for rep in range(2):
            eng.train_steps([0] * k)
            for _ in range(k):
                ring.append(rows[s])
                log.append(entries[s])
                s += 1
            _check(eng, ring, log, s, f"E={E} k={k} cap={cap} replay {rep}")
        assert log.count == E * (s // T)
        eng.close()


# ------------------------------------------------------------------------ L1
def test_l1_lockstep_log_across_the_wrap():
    E, T, eps = 37, 2, 7
    R = 2 * E
    rows, entries = _twin(E, eps * T, T)
    # every entry is the step-order fp32 sum of the episode's rewards in the replay rows
    for p in range(eps):
        ent = entries[p * T + T - 1]
        assert ent.shape == (E, 1 + N) and entries[p * T].shape[0] == 0
        for e in range(E):
            want = rm.episode_sums(rows[p * T:(p + 1) * T, e][:, REW])
            assert np.array_equal(_bits(ent[e]), _bits(want)), (p, e, ent[e], want)
    eng = _engine(E, eps * T * E, T=T, log_rows=R)
    ring, log = rm.RingModel(eps * T * E, STRIDE), rm.LogModel(R, N)

    def spans(cases):
        for first, n in cases:
            assert np.array_equal(_bits(eng.episode_log(first, n)), _bits(log.read(first, n))), (first, n)

    for s in range(eps * T):
        eng.env_step()
        ring.append(rows[s])
        log.append(entries[s])
        _check(eng, ring, log, s + 1, f"step {s}")
        if log.count == 3 * E:                # live [37, 111), the wrap between entries 73 and 74
            spans([(E, 20), (80, 31), (60, 30), (E, R), (50, 0)])
    assert log.count == eps * E == 259        # live [185, 259), the wrap between 221 and 222
    spans([(190, 20), (230, 29), (210, 30), (185, R), (200, 0), (221, 2), (258, 1)])


# ------------------------------------------------------------------------ L2
def test_l2_arrival_order_log_across_the_wrap():
    """staggered episode ends: every step the new entries are, as a set, the ended envs'
    sums, in the slots count .. count + k - 1 modulo 2 E; everything else stays"""
    E, T = 37, 4
    R = 2 * E
    steps = 3 * R * T // E + T                # ~E / T entries per step: three wraps of the log
    eng = _engine(E, steps * E, T=T, log_rows=R)
    st = eng.env_state()
    ep0 = np.arange(E) % T
    eng.set_env_state(st["pos"], st["vel"], st["goal"], ep_step=ep0)
    log = rm.LogModel(R, N)
    open_rew = [[] for _ in range(E)]
    for s in range(steps):
        eng.env_step()
        eng.synchronize()
        row = eng.replay_rows(s * E, E).cpu().numpy()
        for e in range(E):
            open_rew[e].append(row[e, REW])
        term = _ends(E, T, s, ep0)
        assert len(term) in (9, 10)
        want = np.stack([rm.episode_sums(np.stack(open_rew[e])) for e in term])
        for e in term:
            open_rew[e] = []
        count = log.count
        assert eng.episode_count() == count + len(term)
        raw = _raw_log(eng, R)
        new = raw[(count + np.arange(len(term))) % R]
        key = [tuple(r) for r in _bits(want)]
        assert len(set(key)) == len(term)                 # distinct entries: the matching is one to one
        assert sorted(tuple(r) for r in _bits(new)) == sorted(key), (s, new, want)
        assert np.array_equal(_bits(eng.episode_log(count, len(term))), _bits(new))
        log.append(new)                                   # the device's order within the step
        assert np.array_equal(_bits(raw), _bits(log.storage)), s    # earlier live entries unchanged
        ctl = rm.ctl_read(eng.region("ctl", torch.uint8).cpu().numpy())
        assert ctl["episodes"] == log.count and ctl["ep_pending"] == 0 and ctl["len"] == (s + 1) * E
    assert log.count >= 3 * R


# ------------------------------------------------------------------------ L3
def test_l3_episode_log_refuses_ranges_outside_the_live_window():
    E, T = 5, 2
    R = 2 * E
    rows, entries = _twin(E, 4 * T, T)
    eng = _engine(E, 4 * T * E, T=T, log_rows=R)
    log = rm.LogModel(R, N)
    for s in range(3 * T):
        eng.env_step()
        log.append(entries[s])
    assert eng.episode_count() == log.count == 15         # live [5, 15)
    out = np.empty((R + 1, 1 + N), F32)
    ptr = out.ctypes.data_as(eng.lib.mdp_episode_log.argtypes[3])
    for first, n in [(5, R + 1), (-1, 1), (10, 6), (15, 1), (4, 1), (0, R), (4, R), (5, -1)]:
        with pytest.raises(IndexError):
            log.read(first, n)
        assert eng.lib.mdp_episode_log(eng.h, first, n, ptr) < 0, (first, n)
        assert "mdp_episode_log" in eng.lib.mdp_last_error(eng.h).decode(), (first, n)
        if n >= 0:
            with pytest.raises(MdpError, match="mdp_episode_log"):
                eng.episode_log(first, n)
    # the handle goes on working: the live window reads, the next episode logs
    assert np.array_equal(_bits(eng.episode_log(5, R)), _bits(log.read(5, R)))
    assert eng.lib.mdp_episode_log(eng.h, 15, 0, ptr) == 0
    for s in range(3 * T, 4 * T):
        eng.env_step()
        log.append(entries[s])
    assert eng.episode_count() == 20
    assert np.array_equal(_bits(eng.episode_log(10, R)), _bits(log.read(10, R)))
    with pytest.raises(MdpError, match="mdp_episode_log"):
        eng.episode_log(9, 1)
