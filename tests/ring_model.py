"""Host model of the replay ring and the finished-episode log (numpy only).

The device keeps two rings whose heads several writers move: the replay ring
(``mdp_buffer_add_rows`` at the host's head; ``k_rollout`` at the device's
``Ctl.next``; ``mdp_buffer_set_len`` sets both) and the finished-episode log
(``k_rollout`` at ``Ctl.episodes``).  The models here know nothing of those
writers: they are fed the *linear* history of rows and log entries and say what
the rings must hold after it.  tests/test_ring_model_oracle.py pins them against
``oracle/replay.py`` and a one-row-at-a-time ring; tests/test_ring_log_wrap_gpu.py
holds the device to them bit for bit.
"""
import re

import numpy as np

F32 = np.float32

# byte offsets inside ``struct Ctl`` (maddpg_amd/csrc/mdp_topo.h); ctl_offsets()
# re-derives them from the header's text and the oracle test compares
CTL_LEN, CTL_NEXT, CTL_ENV_STEPS, CTL_EPISODES = 2504, 2512, 2520, 2528
CTL_UPD_CTR, CTL_EP_PENDING = 2568, 2640

_SIZES = {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "uint64_t": 8, "float": 4}


def ctl_offsets(header_text):
    """{field: byte offset} of ``struct Ctl`` under the C layout rules (every member
    aligned to its own size)."""
    body = re.search(r"struct Ctl \{(.*?)\n\};", header_text, re.S).group(1)
    off, out = 0, {}
    for line in body.splitlines():
        m = re.match(r"\s*(\w+)\s+(\w+)(?:\[(\d+)\])?;", line)
        if not m:
            continue
        size = _SIZES[m.group(1)]
        off = (off + size - 1) // size * size
        out[m.group(2)] = off
        off += size * int(m.group(3) or 1)
    return out


def ctl_read(ctl_bytes):
    """the ring and log counters of a device control block read back as uint8"""
    b = np.ascontiguousarray(ctl_bytes, np.uint8)

    def i64(o):
        return int(b[o:o + 8].view(np.int64)[0])

    return {"len": i64(CTL_LEN), "next": i64(CTL_NEXT), "env_steps": i64(CTL_ENV_STEPS),
            "episodes": i64(CTL_EPISODES), "ep_pending": int(b[CTL_EP_PENDING:CTL_EP_PENDING + 4].view(np.uint32)[0])}


class RingModel:
    """The reference's ``ReplayBuffer`` as a ring of joint rows: ``append`` is ``add``
    once per row in order, so only the last ``cap`` rows of one call survive."""

    def __init__(self, cap, stride=None):
        self.cap = int(cap)
        self.len = 0
        self.next = 0
        self._store = None if stride is None else np.zeros((self.cap, int(stride)), F32)

    @property
    def storage(self):
        """[cap, stride] float32, zeros where nothing was written"""
        return np.zeros((self.cap, 0), F32) if self._store is None else self._store

    def _slots(self, first, count):
        """the slots of `count` consecutive rows whose first goes to the head + `first`"""
        return (self.next + first + np.arange(count, dtype=np.int64)) % self.cap

    def append(self, rows):
        rows = np.asarray(rows, F32)
        assert rows.ndim == 2
        if self._store is None:
            self._store = np.zeros((self.cap, rows.shape[1]), F32)
        k = rows.shape[0]
        skip = max(0, k - self.cap)                 # rows a later row of this call overwrites
        self._store[self._slots(skip, k - skip)] = rows[skip:]
        self.len = min(self.cap, self.len + k)
        self.next = int(self._slots(k, 1)[0])

    def set(self, length, next_idx):
        assert 0 <= length <= self.cap and 0 <= next_idx < self.cap
        self.len, self.next = int(length), int(next_idx)


class LogModel:
    """The finished-episode log: entry number c sits in slot c % rows; the last
    `rows` entries are live."""

    def __init__(self, rows, n_agents):
        self.rows, self.n = int(rows), int(n_agents)
        self.count = 0
        self.storage = np.zeros((self.rows, 1 + self.n), F32)

    def append(self, entries):
        entries = np.asarray(entries, F32).reshape(-1, 1 + self.n)
        for e in entries:
            self.storage[self.count % self.rows] = e
            self.count += 1

    def read(self, first, n):
        first, n = int(first), int(n)
        if n < 0 or n > self.rows or first < 0 or first + n > self.count or first < self.count - self.rows:
            raise IndexError(f"entries [{first}, {first + n}) are outside the live window "
                             f"[{max(0, self.count - self.rows)}, {self.count})")
        return self.storage[(first + np.arange(n, dtype=np.int64)) % self.rows].copy()


def episode_sums(rew_steps):
    """The log entry [tot | per agent] of one episode from its per-step rewards
    [T, n]: per agent the sequential fp32 sum in step order starting from 0.f, tot the
    sequential fp32 sum over agents of those sums (what k_rollout computes)."""
    rew = np.asarray(rew_steps, F32)
    acc = np.zeros(rew.shape[1], F32)
    for r in rew:
        acc = (acc + r).astype(F32)
    tot = F32(0)
    for a in acc:
        tot = F32(tot + a)
    return np.concatenate([[tot], acc]).astype(F32)


def draw_length(length, num_envs, cap):
    """the ring length the first round of a training step draws against: the one the
    step's rollout leaves"""
    return min(int(cap), int(length) + int(num_envs))


# ---- CPython's random.Random restated (Modules/_randommodule.c, Lib/random.py)
_N, _M = 624, 397


def _twist(mt):
    mt = [int(x) for x in mt]
    for k in range(_N):
        y = (mt[k] & 0x80000000) | (mt[(k + 1) % _N] & 0x7FFFFFFF)
        mt[k] = mt[(k + _M) % _N] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
    return mt


def _temper(y):
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    y ^= y >> 18
    return y & 0xFFFFFFFF


def mt_draws(state625, length, draws):
    """(`draws` calls of randint(0, length - 1), the state after them); the state is
    random.getstate()[1]: 624 words and the read position"""
    mt, pos = [int(x) for x in state625[:_N]], int(state625[_N])
    n = int(length)
    assert n >= 1
    k = n.bit_length()
    out = []
    for _ in range(int(draws)):
        while True:                                  # _randbelow_with_getrandbits
            if pos >= _N:
                mt, pos = _twist(mt), 0
            r = _temper(mt[pos]) >> (32 - k)         # getrandbits(k), k <= 32
            pos += 1
            if r < n:
                break
        out.append(r)
    return np.array(out, np.int64), np.array(mt + [pos], np.uint32)


def mt_state_after(state625, length, draws):
    return mt_draws(state625, length, draws)[1]


# ---- the cases of tests/test_ring_log_wrap_gpu.py that the CPU tests reason about
# R2: one-step rollouts; one ragged tile of 16 envs, one full tile, three workgroups
R2 = {"E": (5, 16, 37), "T": 3}


def r2_caps(E):
    return [E, E + 1, 2 * E - 1, 3 * E + 7, 4 * E]


def r2_steps(E, cap):
    """enough steps of E rows for three wraps of the ring, and one more"""
    return -(-3 * cap // E) + 1


# R4: the draw length of a step graph at four fill levels (len, next) set with set_ring
R4 = {"E": 16, "B": 64, "n": 3, "cap": 5 * 16 + 3, "py_seed": 20240,
      # len + E < cap, == cap, > cap (the row block straddles the ring's end), len == cap
      "levels": [(32, 32), (67, 67), (75, 75), (83, 40)]}
# R5: multi-step rollout launches; T = 3, episode log 2 E rows
R5 = {"E": (1, 8, 16), "k": (2, 7, 64), "T": 3}


def r5_caps(E, k):
    """the ring overwritten whole every step, a launch that crosses the ring's end, a
    launch that wraps more than once"""
    return sorted({E, 3 * E + 1, max(1, k * E - 1)})


def r4_chain(state625):
    """R4 on the host: [(len, next, state before the step, state after it)] for the
    eager step from the empty ring and then each fill level"""
    E, cap, nb = R4["E"], R4["cap"], R4["n"] * R4["B"]
    out, st = [], np.asarray(state625, np.uint32)
    for length, nxt in [(0, 0)] + R4["levels"]:
        after = mt_state_after(st, draw_length(length, E, cap), nb)
        out.append((length, nxt, st, after))
        st = after
    return out
