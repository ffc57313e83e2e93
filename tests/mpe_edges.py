"""Edge states for the MPE step (host side only).

The device steps the world in fp32 (``env_physics_tile``, ``env_reward``,
``env_bench``, ``env_obs`` in ``maddpg_amd/csrc/mdp_kernels.hip``); the oracle
(``oracle/mpe.py``) is fp64.  This module holds

* ``step_t`` / ``reward_t`` / ``bench_t``: the step, the rewards and the
  ``benchmark_data`` records restated in a chosen dtype *in the device's
  operation order* -- ``((100 d) / dist) pen``, ``softplus(x) = max(x, 0) +
  log1p(exp(-|x|))``, ``dmin = f32(size_a) + f32(size_b)``, damping by 0.75 and
  then ``+ F 0.1``, the clamp ``v / |v| ms``.  In float64 they are the oracle
  bit for bit (``tests/test_mpe_edges_oracle.py``); in float32 they are the
  yardstick: what a correct fp32 step may differ from the oracle by;
* the input families (``families()``): states placed on the contact depths,
  the clamp threshold, the boundary-penalty band edges and the collision /
  occupied indicators, every array float32 so that the device and the oracle
  read the same bits, laid out so that the sharpest cases sit on tile rows 0,
  15, 16 and the last row of a ragged E;
* ``YARD``: per family, case group and quantity, the worst error of the
  fp32 restatement against fp64 as ``measure()`` found it on the CPU;
* ``decided`` / ``integer_parts``: which cases have every indicator distance
  more than ``DECIDE`` from its threshold, and the indicator counts there.

Coincident colliding entities (0 / 0 in MPE itself) are out of scope: every
colliding pair is at least ``MIN_SEP`` apart.
"""
import math

import numpy as np

from oracle import mpe

F32 = np.float32
F64 = np.float64
ACT = 5
K = 1e-3             # contact_margin
MIN_SEP = 1e-3       # smallest distance of a colliding pair in any family
DECIDE = 1e-6        # an indicator distance further than this from its threshold is decided (~30 ulp at 0.3)
FACTOR = 4           # the device may be FACTOR x the fp32 restatement's own error away

T_GRID = (-250.0, -100.0, -20.0, -5.0, -1.0, -0.1, 0.0, 0.1, 1.0, 5.0, 20.0, 87.0, 104.0, 1000.0)
# unit directions of pos_a - pos_b: the four axis ones are exact (dx or dy exactly 0)
DIRS = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)] + [(math.cos(a), math.sin(a)) for a in
                                                              (math.pi / 4, 1.0, 2.5, 4.0)]
CONTACT_PAIRS = [("simple_spread", 3, 0, (0, 1)), ("simple_spread", 3, 0, (1, 2)),
                 ("simple_tag", 4, 3, (0, 1)), ("simple_tag", 4, 3, (0, 3)), ("simple_tag", 4, 3, (3, 4)),
                 ("simple_tag", 4, 3, (2, 5)), ("simple_tag", 6, 4, (4, 5))]
CLAMP_DELTAS = (0.5, -0.5, 1e-2, -1e-2, 1e-4, -1e-4, 1e-6, -1e-6, 1e-7, -1e-7, 0.0, 3.0, 30.0)
CLAMP_ANGLES = (0.0, math.pi / 2, math.pi / 4, 1.0, 2.5, 4.0, 5.5)
CAP_X = 1 + math.log(10.0) / 2     # where exp(2 x - 2) reaches the cap 10
BOUNDARY_X = (0.5, 0.9, 0.95, 1.0, 1.5, CAP_X - 1e-4, CAP_X + 1e-4, 3.0, 50.0,
              0.9 - 1e-6, 0.9 + 1e-6, 1 - 1e-6, 1 + 1e-6, 45.0, 1e4)
OCC_OFFSETS = (1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)
SWEEP_GAP0 = 5e-3                  # the collision sweeps start dmin + this apart
TIES = 5                           # cases of a collision sweep on the fp32 threshold itself
SWEEP_PAIRS = [("simple_spread", 3, 0, (0, 1)), ("simple_tag", 4, 3, (0, 3)), ("simple_tag", 4, 3, (0, 1))]
PLAIN = [("simple", 1, 0), ("simple_adversary", 3, 1), ("simple_adversary", 8, 1), ("simple_speaker_listener", 2, 0)]

# Worst |fp32 restatement - fp64| per family, case group and quantity, as measure()
# found them (tests/test_mpe_edges_oracle.py re-measures; numpy's fp32 exp / log1p
# differ by an ulp between SIMD builds).  pos / vel: one step from the family's
# inputs.  rew: the rewards, both forms on the fp32 restatement's post-step state;
# rec: the benchmark_data records, both forms on its post-state of the step with
# uniform actions that the records test takes; decided cases only.
YARD = {
    "contact-simple_spread3-01": {
        "apart": {"pos": 2.33e-07, "vel": 4.84e-08, "rew": 4.61e-06, "rec": 1.02e-06},
        "deep": {"pos": 2.36e-07, "vel": 3.84e-07, "rew": 4.28e-06, "rec": 1.01e-06},
        "knee": {"pos": 2.36e-07, "vel": 2.3e-07, "rew": 5.51e-06, "rec": 9.64e-07},
    },
    "contact-simple_spread3-12": {
        "apart": {"pos": 2.24e-07, "vel": 4.28e-08, "rew": 4.06e-06, "rec": 1.67e-06},
        "deep": {"pos": 2.35e-07, "vel": 3.98e-07, "rew": 6e-06, "rec": 1.73e-06},
        "knee": {"pos": 2.33e-07, "vel": 2.3e-07, "rew": 6.47e-06, "rec": 1.78e-06},
    },
    "contact-simple_tag4-01": {
        "apart": {"pos": 2.3e-07, "vel": 2.98e-08, "rew": 0.0, "rec": 0.0},
        "deep": {"pos": 2.35e-07, "vel": 1.74e-07, "rew": 0.0, "rec": 0.0},
        "knee": {"pos": 2.4e-07, "vel": 9.57e-08, "rew": 0.0, "rec": 0.0},
    },
    "contact-simple_tag4-03": {
        "apart": {"pos": 2.34e-07, "vel": 3.58e-08, "rew": 2.38e-07, "rec": 0.0},
        "deep": {"pos": 2.41e-07, "vel": 1.25e-07, "rew": 0.0, "rec": 0.0},
        "knee": {"pos": 2.36e-07, "vel": 5.63e-08, "rew": 0.0, "rec": 0.0},
    },
    "contact-simple_tag4-34": {
        "apart": {"pos": 2.34e-07, "vel": 3.28e-08, "rew": 0.0, "rec": 0.0},
        "deep": {"pos": 2.32e-07, "vel": 9.21e-08, "rew": 0.0, "rec": 0.0},
        "knee": {"pos": 2.34e-07, "vel": 1.2e-07, "rew": 0.0, "rec": 0.0},
    },
    "contact-simple_tag4-25": {
        "apart": {"pos": 2.37e-07, "vel": 3.04e-08, "rew": 0.0, "rec": 0.0},
        "deep": {"pos": 2.37e-07, "vel": 2e-07, "rew": 0.0, "rec": 0.0},
        "knee": {"pos": 2.38e-07, "vel": 2.05e-07, "rew": 0.0, "rec": 0.0},
    },
    "contact-simple_tag6-45": {
        "apart": {"pos": 2.38e-07, "vel": 3.32e-08, "rew": 2.8e-07, "rec": 0.0},
        "deep": {"pos": 2.32e-07, "vel": 9.22e-08, "rew": 0.0, "rec": 0.0},
        "knee": {"pos": 2.39e-07, "vel": 4.14e-08, "rew": 0.0, "rec": 0.0},
    },
    "cluster-simple_spread8": {
        "all": {"pos": 2.76e-07, "vel": 2.75e-06, "rew": 4.61e-06, "rec": 3.4e-07},
    },
    "clamp-simple_tag4": {
        "all": {"pos": 2.4e-07, "vel": 1.1e-07, "rew": 0.0, "rec": 0.0},
    },
    "boundary-simple_tag4": {
        "all": {"pos": 0.0, "vel": 0.0, "rew": 4.34e-07, "rec": 0.0},
    },
    "occupied-simple_spread3": {
        "all": {"pos": 0.0, "vel": 0.0, "rew": 3.05e-06, "rec": 1.02e-06},
    },
    "sweep-simple_spread3-01": {
        "all": {"pos": 1.76e-08, "vel": 2.72e-08, "rew": 4.71e-06, "rec": 1.3e-06},
    },
    "sweep-simple_tag4-03": {
        "all": {"pos": 1.42e-08, "vel": 2.7e-08, "rew": 0.0, "rec": 0.0},
    },
    "sweep-simple_tag4-01": {
        "all": {"pos": 1.56e-08, "vel": 2.7e-08, "rew": 0.0, "rec": 0.0},
    },
    "plain-simple1": {
        "far": {"pos": 2.73e-05, "vel": 1.83e-06, "rew": 0.0516},
        "near": {"pos": 2.24e-08, "vel": 3.35e-08, "rew": 3.01e-07},
    },
    "plain-simple_adversary3": {
        "far": {"pos": 2.98e-05, "vel": 1.91e-06, "rew": 0.109, "rec": 0.112},
        "near": {"pos": 2.91e-08, "vel": 6.71e-08, "rew": 1.44e-07, "rec": 4.46e-07},
    },
    "plain-simple_adversary8": {
        "far": {"pos": 2.95e-05, "vel": 1.87e-06, "rew": 0.186, "rec": 0.412},
        "near": {"pos": 5.81e-08, "vel": 5.96e-08, "rew": 2.53e-07, "rec": 1.58e-05},
    },
    "plain-simple_speaker_listener2": {
        "far": {"pos": 2.79e-05, "vel": 1.84e-06, "rew": 0.198},
        "near": {"pos": 2.92e-08, "vel": 2.61e-08, "rew": 6.19e-07},
    },
}


def scenario(name, n=None, na=None):
    if name == "simple_tag":
        return mpe.SimpleTag(n_adv=na, n_good=n - na)
    if name == "simple_adversary":
        return mpe.SimpleAdversary(n_good=n - na, n_adv=na)
    if name == "simple_spread":
        return mpe.SimpleSpread(n)
    if name == "simple_speaker_listener":
        from tests.speaker_listener import SimpleSpeakerListener
        return SimpleSpeakerListener()
    assert name == "simple"
    return mpe.Simple()


def has_records(sc):
    return sc.name in ("simple_spread", "simple_adversary", "simple_tag")


# ----------------------------------------------------------- restatements
def softplus_t(x):
    """max(x, 0) + log1p(exp(-|x|)) in x's dtype.  float64 goes through libm one
    element at a time: np.logaddexp, which the oracle uses, is that formula on
    libm's exp and log1p, while numpy's array exp may be a SIMD routine an ulp away."""
    m = -np.abs(x)
    if x.dtype == np.float64:
        t = np.array([math.log1p(math.exp(v)) for v in m.ravel()], F64).reshape(m.shape)
    else:
        t = np.log1p(np.exp(m))
    return np.maximum(x, x.dtype.type(0)) + t


def step_t(sc, pos, vel, act, dtype):
    """World.step in `dtype`, in env_physics_tile's order: (pos, vel) after one step"""
    dt = np.dtype(dtype).type
    pos, vel, act = np.array(pos, dtype), np.array(vel, dtype), np.asarray(act, dtype)
    E, n, ne = pos.shape[0], sc.n_agents, sc.n_entities
    k = dt(K)
    fx, fy = np.zeros((E, ne), dtype), np.zeros((E, ne), dtype)
    with np.errstate(all="ignore"):
        for e in range(ne):
            if e < n:
                acc = dt(5.0 if sc.accel[e] is None else sc.accel[e])
                fx[:, e] = (act[:, e, 1] - act[:, e, 2]) * acc
                fy[:, e] = (act[:, e, 3] - act[:, e, 4]) * acc
            if not (sc.collide[e] and sc.movable[e]):
                continue
            for o in range(ne):
                if o == e or not sc.collide[o]:
                    continue
                a, b = min(o, e), max(o, e)
                dx, dy = pos[:, a, 0] - pos[:, b, 0], pos[:, a, 1] - pos[:, b, 1]
                dist = np.sqrt(dx * dx + dy * dy)
                dmin = dt(sc.size[a]) + dt(sc.size[b])
                pen = softplus_t(-(dist - dmin) / k) * k
                sx, sy = dt(100) * dx / dist * pen, dt(100) * dy / dist * pen
                if e == a:
                    fx[:, e], fy[:, e] = sx + fx[:, e], sy + fy[:, e]
                else:
                    fx[:, e], fy[:, e] = -sx + fx[:, e], -sy + fy[:, e]
        for e in range(ne):
            if not sc.movable[e]:
                continue
            assert e < n                    # every movable entity of these scenarios is an agent: it has a force
            vx, vy = vel[:, e, 0] * dt(0.75), vel[:, e, 1] * dt(0.75)
            vx, vy = vx + fx[:, e] * dt(0.1), vy + fy[:, e] * dt(0.1)
            if sc.max_speed[e] is not None:
                ms = dt(sc.max_speed[e])
                spd = np.sqrt(vx * vx + vy * vy)
                over = spd > ms
                vx, vy = np.where(over, vx / spd * ms, vx), np.where(over, vy / spd * ms, vy)
            vel[:, e, 0], vel[:, e, 1] = vx, vy
            pos[:, e, 0] += vx * dt(0.1)
            pos[:, e, 1] += vy * dt(0.1)
    assert pos.dtype == vel.dtype == np.dtype(dtype)
    return pos, vel


def _dist(p, a, b):
    dx, dy = p[:, a, 0] - p[:, b, 0], p[:, a, 1] - p[:, b, 1]
    return np.sqrt(dx * dx + dy * dy)


def _sq(p, a, b):
    dx, dy = p[:, a, 0] - p[:, b, 0], p[:, a, 1] - p[:, b, 1]
    return dx * dx + dy * dy


def _goal_sel(cols, goal):
    """cols: list over landmarks of [E]; the goal landmark's entry per env"""
    return np.stack(cols, 1)[np.arange(len(goal)), goal]


def reward_t(sc, pos, goal, dtype, shared=True):
    """env_reward in `dtype`: [E, n], a collaborative world's shared sum included (the
    device adds the agents' rewards one after another; shared=False: spread's
    per-agent rewards before that sum)"""
    dt = np.dtype(dtype).type
    p = np.asarray(pos, dtype)
    E, n, L = p.shape[0], sc.n_agents, sc.n_landmarks
    goal = np.zeros(E, int) if goal is None else np.asarray(goal)
    rew = np.zeros((E, n), dtype)
    size = [dt(s) for s in sc.size]
    if sc.name == "simple":
        rew[:, 0] = -_sq(p, 0, 1)
    elif sc.name == "simple_speaker_listener":
        r = -_goal_sel([_sq(p, 1, n + l) for l in range(L)], goal)
        rew[:, 0] = rew[:, 1] = r + r
    elif sc.name == "simple_spread":
        base = np.zeros(E, dtype)
        for l in range(L):
            m = np.full(E, np.inf, dtype)
            for a in range(n):
                m = np.minimum(m, _dist(p, a, n + l))
            base = base - m
        tot = np.zeros(E, dtype)
        for i in range(n):
            r = base.copy()
            for a in range(n):
                r = r - (_dist(p, a, i) < size[a] + size[i]).astype(dtype)
            rew[:, i] = r
            tot = tot + r
        if shared:
            rew[:] = tot[:, None]
    elif sc.name == "simple_adversary":
        dg = [_goal_sel([_dist(p, a, n + l) for l in range(L)], goal) for a in range(n)]
        adv, mg = np.zeros(E, dtype), np.full(E, np.inf, dtype)
        for a in range(n):
            if sc.adversary[a]:
                adv = adv + dg[a]
            else:
                mg = np.minimum(mg, dg[a])
        for i in range(n):
            if sc.adversary[i]:
                rew[:, i] = -_goal_sel([_sq(p, i, n + l) for l in range(L)], goal)
            else:
                rew[:, i] = -mg + adv
    elif sc.name == "simple_tag":
        caught = np.zeros(E, dtype)
        for g in range(n):
            for a in range(n):
                if not sc.adversary[g] and sc.adversary[a]:
                    caught = caught + (_dist(p, g, a) < size[g] + size[a]).astype(dtype)
        for i in range(n):
            if sc.adversary[i]:
                rew[:, i] = dt(10) * caught
                continue
            r = np.zeros(E, dtype)
            for a in range(n):
                if sc.adversary[a]:
                    r = r - dt(10) * (_dist(p, a, i) < size[a] + size[i]).astype(dtype)
            for d in range(2):
                x = np.abs(p[:, i, d])
                with np.errstate(over="ignore"):
                    cap = np.minimum(np.exp(dt(2) * x - dt(2)), dt(10))
                r = r - np.where(x < dt(0.9), dt(0), np.where(x < dt(1.0), (x - dt(0.9)) * dt(10), cap))
            rew[:, i] = r
    else:
        raise ValueError(sc.name)
    assert rew.dtype == np.dtype(dtype)
    return rew


def bench_t(sc, pos, goal, dtype):
    """env_bench in `dtype`: a list over agents of [E, width] records"""
    dt = np.dtype(dtype).type
    p = np.asarray(pos, dtype)
    E, n, L = p.shape[0], sc.n_agents, sc.n_landmarks
    size = [dt(s) for s in sc.size]
    out = []
    if sc.name == "simple_spread":
        min_dists, occupied = np.zeros(E, dtype), np.zeros(E, dtype)
        for l in range(L):
            m = np.full(E, np.inf, dtype)
            for a in range(n):
                m = np.minimum(m, _dist(p, a, n + l))
            min_dists = min_dists + m
            occupied = occupied + (m < dt(0.1)).astype(dtype)
        for i in range(n):
            coll = np.zeros(E, dtype)
            for a in range(n):
                coll = coll + (_dist(p, a, i) < size[a] + size[i]).astype(dtype)
            out.append(np.stack([-min_dists - coll, coll, min_dists, occupied], 1))
    elif sc.name == "simple_adversary":
        goal = np.asarray(goal)
        for i in range(n):
            sq = [_sq(p, i, n + l) for l in range(L)]
            g = _goal_sel(sq, goal)
            out.append(g[:, None] if sc.adversary[i] else np.stack(sq + [g], 1))
    elif sc.name == "simple_tag":
        for i in range(n):
            c = np.zeros(E, dtype)
            if sc.adversary[i]:
                for a in range(n):
                    if not sc.adversary[a]:
                        c = c + (_dist(p, a, i) < size[a] + size[i]).astype(dtype)
            out.append(c[:, None])
    else:
        raise AttributeError(f"scenario {sc.name!r} has no benchmark_data")
    assert all(o.dtype == np.dtype(dtype) for o in out)
    return out


# ------------------------------------------------------------- the oracle
def oracle_state(pos, vel, goal=None, comm=None):
    st = {"pos": np.asarray(pos, F64), "vel": np.asarray(vel, F64)}
    if goal is not None:
        st["goal"] = np.asarray(goal)
    if comm is not None:
        st["comm"] = np.asarray(comm, F64)
    return st


def oracle_step(sc, pos, vel, act, goal=None):
    """oracle/mpe.py's Scenario.step on the fp32 inputs: (state, obs_n, rew [E, n]).
    (an agent at rest under the clamp is 0 / 0 in the branch np.where drops: quiet)"""
    with np.errstate(all="ignore"):
        return sc.step(oracle_state(pos, vel, goal), np.asarray(act, F64))


def oracle_reward(sc, pos, goal=None):
    """the oracle's rewards of a given post-physics state, shared as step() shares them"""
    with np.errstate(all="ignore"):
        st = oracle_state(pos, np.zeros_like(pos), goal)
        rew = sc.reward(st)
    if sc.collaborative:
        rew = np.repeat(rew.sum(1, keepdims=True), sc.n_agents, axis=1)
    return rew


def oracle_records(sc, pos, goal=None):
    return sc.benchmark_data(oracle_state(pos, np.zeros_like(pos), goal))


def copied_entries(sc):
    """per agent, a mask over its observation: True where the entry is a copy of a
    state entry or a constant (exact on the device), False where it is a difference"""
    rng = np.random.default_rng(0)
    ne, n = sc.n_entities, sc.n_agents
    st = {"pos": rng.uniform(1, 2, (1, ne, 2)), "vel": rng.uniform(3, 4, (1, ne, 2)), "goal": np.zeros(1, int)}
    if sc.name == "simple_speaker_listener":
        st["comm"] = rng.uniform(5, 6, (1, n, 3))
    vals = np.concatenate([np.ravel(v) for k, v in st.items() if k != "goal"] + [[0.0, 0.15, 0.65]])
    return [np.isin(o[0], vals) for o in sc.observation(st)]


# ---------------------------------------------------------- the indicators
def indicator_margins(sc, pos):
    """[E, m] fp64 distances minus thresholds of every indicator of the state (m may be 0)"""
    p = np.asarray(pos, F64)
    E, n = p.shape[0], sc.n_agents
    cols = []
    if sc.name == "simple_spread":
        for i in range(n):
            for a in range(i + 1, n):
                cols.append(_dist(p, a, i) - (sc.size[a] + sc.size[i]))
        for l in range(sc.n_landmarks):
            cols.append(np.min(np.stack([_dist(p, a, n + l) for a in range(n)], 1), 1) - 0.1)
    elif sc.name == "simple_tag":
        for g in range(n):
            for a in range(n):
                if not sc.adversary[g] and sc.adversary[a]:
                    cols.append(_dist(p, g, a) - (sc.size[g] + sc.size[a]))
    return np.stack(cols, 1) if cols else np.zeros((E, 0))


def decided(sc, pos):
    """[E] bool: every indicator distance of the state is more than DECIDE from its threshold"""
    return np.all(np.abs(indicator_margins(sc, pos)) > DECIDE, axis=1)


def integer_parts(sc, pos):
    """the oracle's indicator counts of a state: spread {"coll" [E, n] (self included),
    "occupied" [E]}; tag {"caught" [E], "hit" [E, n]: adversaries in contact with a
    good agent i, "tags" [E, n]: good agents in contact with adversary i}"""
    p = np.asarray(pos, F64)
    E, n = p.shape[0], sc.n_agents
    st = {"pos": p}
    if sc.name == "simple_spread":
        coll = np.stack([sum(sc.is_collision(st, a, i).astype(int) for a in range(n)) for i in range(n)], 1)
        occ = sum((np.min(np.stack([_dist(p, a, n + l) for a in range(n)], 1), 1) < 0.1).astype(int)
                  for l in range(sc.n_landmarks))
        return {"coll": coll, "occupied": occ}
    if sc.name == "simple_tag":
        hit, tags = np.zeros((E, n), int), np.zeros((E, n), int)
        for g in range(n):
            for a in range(n):
                if not sc.adversary[g] and sc.adversary[a]:
                    c = sc.is_collision(st, g, a).astype(int)
                    hit[:, g] += c
                    tags[:, a] += c
        return {"caught": hit.sum(1), "hit": hit, "tags": tags}
    return {}


# ------------------------------------------------------------ the families
def _softmax_actions(rng, E, n, widths=None):
    z = rng.normal(size=(E, n, ACT))
    if widths is not None:
        for j, w in enumerate(widths):
            z[:, j, w:] = -np.inf
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(F32)


def _uniform_actions(E, n, widths=None):
    """0.2 in every entry: no action force (a narrower agent: 1 / width, zeros in its pad)"""
    act = np.full((E, n, ACT), 0.2, F32)
    if widths is not None:
        for j, w in enumerate(widths):
            act[:, j, :w] = F32(1.0 / w)
            act[:, j, w:] = 0
    return act


def _far(j):
    """a parking place of entity j < 8: on a ring of radius 5 -- 3.8 from its neighbours
    and more than 3 from anything within 1.9 of the origin (a pair in the unit box)"""
    assert 0 <= j < 8
    return 5.0 * np.array([math.cos(2 * math.pi * j / 8 + 0.2), math.sin(2 * math.pi * j / 8 + 0.2)])


def _layout(M, sharp):
    """row -> case index: the cases in order, copies of the sharp ones on rows 0, 15,
    16 and the last row, E ragged (E % 16 != 0) and at least 18"""
    s = [int(x) for x in sharp]
    order = list(range(M))
    while len(order) < 15:
        order.append(s[len(order) % len(s)])
    order.insert(0, s[0])
    order.insert(15, s[1 % len(s)])
    order.insert(16, s[2 % len(s)])
    order.append(s[0])
    if len(order) % 16 == 0:
        order.append(s[1 % len(s)])
    return np.array(order)


def _family(kind, fid, scn, pos, vel, act, sharp, goal=None, group=None, meta=None):
    order = _layout(len(pos), sharp)
    E = len(order)
    fam = {"kind": kind, "id": fid, "scn": scn, "order": order, "sharp": [int(x) for x in sharp],
           "pos": np.ascontiguousarray(pos, F32)[order], "vel": np.ascontiguousarray(vel, F32)[order],
           "act": np.ascontiguousarray(act, F32)[order],
           "goal": (np.zeros(len(pos), np.int32) if goal is None else np.asarray(goal, np.int32))[order],
           "group": (np.full(len(pos), "all") if group is None else np.asarray(group))[order],
           "meta": {k: np.asarray(v)[order] for k, v in (meta or {}).items()}}
    assert E % 16 != 0 and E <= 208
    for r in (0, 15, 16, E - 1):
        assert order[r] in fam["sharp"]
    check_family(fam)
    return fam


def check_family(fam):
    """every array fp32 and finite, every colliding pair at least MIN_SEP apart"""
    sc = scenario(*fam["scn"])
    p = fam["pos"].astype(F64)
    for k in ("pos", "vel", "act"):
        assert fam[k].dtype == F32 and np.all(np.isfinite(fam[k]))
    assert fam["pos"].shape == fam["vel"].shape == (len(p), sc.n_entities, 2)
    assert fam["act"].shape == (len(p), sc.n_agents, ACT)
    for a in range(sc.n_entities):
        for b in range(a + 1, sc.n_entities):
            if sc.collide[a] and sc.collide[b]:
                assert _dist(p, a, b).min() >= MIN_SEP, (fam["id"], a, b)


def _t_group(t):
    return "deep" if t <= -20 else "knee" if t <= 5 else "apart"


def contact_family(idx):
    """pair (a, b) at dist = dmin + K t over T_GRID x DIRS; a at a random offset in the
    unit box, every other entity parked; random agent velocities and softmax actions.
    Groups by depth: deep (t <= -20), knee (|t| <= 5), apart (t >= 20)."""
    name, n, na, (a, b) = CONTACT_PAIRS[idx]
    sc = scenario(name, n, na)
    rng = np.random.default_rng(100 + idx)
    dmin = sc.size[a] + sc.size[b]
    cases = [(t, d) for t in T_GRID for d in range(len(DIRS)) if dmin + K * t >= MIN_SEP + 1e-6]
    M, ne = len(cases), sc.n_entities
    pos, vel = np.zeros((M, ne, 2)), np.zeros((M, ne, 2))
    for e in range(ne):
        pos[:, e] = _far(e)
    pos[:, a] = rng.uniform(-0.5, 0.5, (M, 2))
    for c, (t, d) in enumerate(cases):
        pos[c, b] = pos[c, a] - (dmin + K * t) * np.array(DIRS[d])
    vel[:, :n] = rng.uniform(-0.5, 0.5, (M, n, 2))
    ts = np.array([t for t, _ in cases])
    sharp = [cases.index((t, 5)) for t in (-1.0, 0.0, 1.0)]
    fam = _family("contact", f"contact-{name}{n}-{a}{b}", (name, n, na), pos, vel, _softmax_actions(rng, M, n), sharp,
                  group=[_t_group(t) for t in ts], meta={"t": ts, "dir": [d for _, d in cases]})
    fam["pair"] = (a, b)
    # the other entities are at least 3 from the pair and from each other
    p = fam["pos"].astype(F64)
    for x in range(ne):
        for y in range(x + 1, ne):
            assert (x, y) == (a, b) or _dist(p, x, y).min() >= 3
    return fam


def cluster_family():
    """spread N=8: the eight agents on a ring of radius 0.05 .. 0.149 with jitter
    +-0.01: every agent in contact with the seven others, the full 16-entity tile"""
    rng = np.random.default_rng(200)
    M, n = 40, 8
    r = np.concatenate([[0.05, 0.149], rng.uniform(0.05, 0.149, M - 2)])
    ang = 2 * np.pi * np.arange(n) / n
    pos, vel = np.zeros((M, 2 * n, 2)), np.zeros((M, 2 * n, 2))
    pos[:, :n, 0] = r[:, None] * np.cos(ang)
    pos[:, :n, 1] = r[:, None] * np.sin(ang)
    pos[:, :n] += rng.uniform(-0.01, 0.01, (M, n, 2)) + rng.uniform(-0.5, 0.5, (M, 1, 2))
    pos[:, n:] = rng.uniform(-1, 1, (M, n, 2))
    vel[:, :n] = rng.uniform(-0.5, 0.5, (M, n, 2))
    return _family("cluster", "cluster-simple_spread8", ("simple_spread", 8, 0), pos, vel, _softmax_actions(rng, M, n),
                   [0, 1, 2], meta={"r": r})


def clamp_family():
    """tag N=4, no force (uniform action, every entity parked): agent j's velocity is
    ms_j (1 + delta) / 0.75 along CLAMP_ANGLES[(i + j) % 7], so the damped speed is
    ms_j (1 + delta)"""
    sc = scenario("simple_tag", 4, 3)
    cases = [(d, i) for d in CLAMP_DELTAS for i in range(len(CLAMP_ANGLES))]
    M, n, ne = len(cases), 4, 6
    pos, vel = np.zeros((M, ne, 2)), np.zeros((M, ne, 2))
    for e in range(ne):
        pos[:, e] = _far(e)
    for c, (d, i) in enumerate(cases):
        for j in range(n):
            ang = CLAMP_ANGLES[(i + j) % len(CLAMP_ANGLES)]
            vel[c, j] = sc.max_speed[j] * (1 + d) / 0.75 * np.array([math.cos(ang), math.sin(ang)])
    sharp = [cases.index((d, 3)) for d in (0.0, 1e-7, -1e-7)]
    return _family("clamp", "clamp-simple_tag4", ("simple_tag", 4, 3), pos, vel, _uniform_actions(M, n), sharp,
                   meta={"delta": [d for d, _ in cases]})


def boundary_family():
    """tag N=4: the good agent (3) alone, at rest, uniform action, at |x| of BOUNDARY_X
    on each axis in both signs (the other coordinate 0.3: no penalty from it)"""
    cases = [(x, ax, sg) for x in BOUNDARY_X for ax in (0, 1) for sg in (1.0, -1.0)]
    M, n, ne = len(cases), 4, 6
    pos, vel = np.zeros((M, ne, 2)), np.zeros((M, ne, 2))
    for e in range(ne):
        pos[:, e] = np.array([-20.0 - 5 * e, 20.0 + 5 * e])
    for c, (x, ax, sg) in enumerate(cases):
        pos[c, 3, ax], pos[c, 3, 1 - ax] = sg * x, 0.3
    sharp = [cases.index((x, 0, 1.0)) for x in (1.0, 0.9, CAP_X + 1e-4)]
    return _family("boundary", "boundary-simple_tag4", ("simple_tag", 4, 3), pos, vel, _uniform_actions(M, n), sharp,
                   meta={"x": [x for x, _, _ in cases], "axis": [ax for _, ax, _ in cases]})


def occupied_family():
    """spread N=3, everyone at rest with a uniform action (nothing moves): agent 0 at
    0.1 + OCC_OFFSETS from landmark 0 along four directions, and exactly on it; the
    other agents and landmarks parked.  meta set: the direction; offset: nan = on it.
    The last case (set -1, meta tie) has the landmark at x = 0 and the agent at x =
    0.1f, same y: the fp32 distance *equals* the fp32 threshold, `<` says not occupied."""
    dirs = (0, 5, 6, 3)
    cases = [(s, off) for s in dirs for off in OCC_OFFSETS + (None,)] + [(-1, 0.0)]
    rng = np.random.default_rng(300)
    M, n, ne = len(cases), 3, 6
    pos, vel = np.zeros((M, ne, 2)), np.zeros((M, ne, 2))
    for e in range(ne):
        pos[:, e] = _far(e)
    pos[:, 3] = rng.uniform(-0.5, 0.5, (M, 2)).astype(F32)
    for c, (s, off) in enumerate(cases[:-1]):
        pos[c, 0] = pos[c, 3] if off is None else pos[c, 3] + (0.1 + off) * np.array(DIRS[s])
    pos[-1, 3], pos[-1, 0] = (0.0, 0.25), (F32(0.1), 0.25)
    sharp = [cases.index((5, off)) for off in (1e-5, -1e-5, None)]
    fam = _family("indicator", "occupied-simple_spread3", ("simple_spread", 3, 0), pos, vel, _uniform_actions(M, n),
                  sharp, meta={"set": [s for s, _ in cases], "tie": [s < 0 for s, _ in cases],
                               "offset": [np.nan if off is None else off for _, off in cases]})
    fam["pair"], fam["tie_thr"] = (0, 3), F32(0.1)
    return fam


def sweep_family(idx):
    """agents (a, b) dmin + SWEEP_GAP0 apart, closing head-on at speed s each, uniform
    action: after the step the gap is about SWEEP_GAP0 - 0.15 s.  s: 129 points on
    [0, 0.6], then 33 points that put the oracle's post-step gap on a line from
    -2e-3 to 2e-3 and 6 at +-3e-6, +-1e-5, +-3e-5 (the crossing found with the oracle).
    The spread sweep and tag's adversary-good sweep end with TIES cases along the x
    axis (dy = 0: the fp32 distance is |dx| exactly) whose speed is chosen so that the
    fp32 restatement's post-step distance *equals* the fp32 threshold size_a + size_b
    (0.3f; 0.125f): `<` says no collision there, `<=` says one (meta tie)."""
    name, n, na, (a, b) = SWEEP_PAIRS[idx]
    sc = scenario(name, n, na)
    ne, dmin = sc.n_entities, sc.size[a] + sc.size[b]
    u07 = np.array([math.cos(0.7), math.sin(0.7)])

    def build(s, u=u07, centre=(0.21, -0.13)):
        s = np.asarray(s, F64)
        pos, vel = np.zeros((len(s), ne, 2)), np.zeros((len(s), ne, 2))
        for e in range(ne):
            pos[:, e] = _far(e)
        pos[:, a] = np.array(centre) + (dmin + SWEEP_GAP0) / 2 * np.asarray(u)
        pos[:, b] = np.array(centre) - (dmin + SWEEP_GAP0) / 2 * np.asarray(u)
        vel[:, a], vel[:, b] = -s[:, None] * np.asarray(u), s[:, None] * np.asarray(u)
        return pos.astype(F32), vel.astype(F32)

    def gap(s):
        pos, vel = build(s)
        nst, _, _ = oracle_step(sc, pos, vel, _uniform_actions(len(pos), n))
        return _dist(nst["pos"], a, b) - dmin

    s0 = SWEEP_GAP0 / 0.15
    for _ in range(3):                                    # the gap is linear in s to first order: slope -0.15
        s0 = s0 + gap([s0])[0] / 0.15
    targets = np.concatenate([np.linspace(-2e-3, 2e-3, 33), [3e-6, -3e-6, 1e-5, -1e-5, 3e-5, -3e-5]])
    s = np.concatenate([np.linspace(0, 0.6, 129), s0 - targets / 0.15])
    pos, vel = build(s)
    tie = np.zeros(len(s), bool)
    thr = F32(sc.size[a]) + F32(sc.size[b])
    if sc.adversary[a] != sc.adversary[b] or name == "simple_spread":     # the pair is an indicator of the reward
        for k in range(TIES):
            centre = (0.1 * k - 0.2, 0.3)
            cand = s0 + np.linspace(-6e-7, 6e-7, 1201)
            cp, cv = build(cand, (1.0, 0.0), centre)
            p32, _ = step_t(sc, cp, cv, _uniform_actions(len(cand), n), F32)
            assert np.all(p32[:, a, 1] == p32[:, b, 1])
            hit = np.flatnonzero(p32[:, a, 0] - p32[:, b, 0] == thr)
            assert len(hit) >= 20, len(hit)               # a run of speeds: its middle is tens of ulps from either end
            m = hit[len(hit) // 2]
            pos, vel = np.concatenate([pos, cp[m:m + 1]]), np.concatenate([vel, cv[m:m + 1]])
            s, tie = np.append(s, cand[m]), np.append(tie, True)
    g = np.abs(gap(s[:len(targets) + 129]))
    near = [int(i) for i in np.argsort(g) if g[i] > 2 * DECIDE][:3]     # the sharpest decided cases
    fam = _family("indicator", f"sweep-{name}{n}-{a}{b}", (name, n, na), pos, vel, _uniform_actions(len(s), n),
                  near, meta={"s": s, "tie": tie})
    fam["pair"], fam["tie_thr"] = (a, b), thr
    return fam


def plain_family(idx):
    """the scenarios without contacts: four states with |p| up to 1e3 and |v| up to 50,
    four in the unit box, the goal on landmark 0 and on the last one, an agent
    exactly on the goal landmark (at rest: it stays), and -- simple_adversary -- two
    good agents at rest at mirrored offsets of the goal (the tie in the minimum).
    Groups: far (the first four), near."""
    name, n, na = PLAIN[idx]
    sc = scenario(name, n, na)
    rng = np.random.default_rng(400 + idx)
    ne, L = sc.n_entities, sc.n_landmarks
    widths = [3, 5] if name == "simple_speaker_listener" else None
    mover = 1 if name == "simple_speaker_listener" else 0     # the speaker does not move
    M = 14
    pos, vel = rng.uniform(-1, 1, (M, ne, 2)), np.zeros((M, ne, 2))
    vel[:, :n] = rng.uniform(-1, 1, (M, n, 2))
    pos[:4] = rng.uniform(-1e3, 1e3, (4, ne, 2))
    vel[:4, :n] = rng.uniform(-50, 50, (4, n, 2))
    if name == "simple_speaker_listener":
        vel[:, 0] = 0
    act = _softmax_actions(rng, M, n, widths)
    goal = rng.integers(0, L, M)
    goal[8:14] = [0, L - 1, 0, L - 1, 0, L - 1]
    pos = pos.astype(F32).astype(F64)
    # rows 10, 11: an agent on the goal landmark, everyone at rest; rows 12, 13: the tie
    vel[10:14] = 0
    act[10:14] = _uniform_actions(4, n, widths)
    for c in (10, 11):
        pos[c, mover] = pos[c, n + goal[c]]
        if name == "simple_adversary":
            pos[c, n - 1] = pos[c, n + goal[c]]           # a good agent on it too: the minimum is 0
    if name == "simple_adversary":
        for c in (12, 13):
            g = np.round(pos[c, n + goal[c]] * 64) / 64   # multiples of 1 / 64: g +- d is exact
            pos[c, n + goal[c]] = g
            d = np.array([5.0, -3.0]) / 64
            far = g + np.array([3.0, 3.0])
            for i in range(na, n):
                pos[c, i] = far + i                       # the other good agents are further away
            pos[c, na], pos[c, n - 1] = g + d, g - d
    fam = _family("plain", f"plain-{name}{n}", (name, n, na), pos, vel, act, [10, 11, 12], goal=goal,
                  group=["far"] * 4 + ["near"] * (M - 4))
    return fam


def families():
    """every family, by id"""
    fams = [contact_family(i) for i in range(len(CONTACT_PAIRS))]
    fams += [cluster_family(), clamp_family(), boundary_family(), occupied_family()]
    fams += [sweep_family(i) for i in range(len(SWEEP_PAIRS))]
    fams += [plain_family(i) for i in range(len(PLAIN))]
    return {f["id"]: f for f in fams}


_FAMILIES = None


def family(fid):
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = families()
    return _FAMILIES[fid]


FAMILY_IDS = ([f"contact-{nm}{n}-{a}{b}" for nm, n, _na, (a, b) in CONTACT_PAIRS]
              + ["cluster-simple_spread8", "clamp-simple_tag4", "boundary-simple_tag4", "occupied-simple_spread3"]
              + [f"sweep-{nm}{n}-{a}{b}" for nm, n, _na, (a, b) in SWEEP_PAIRS]
              + [f"plain-{nm}{n}" for nm, n, _na in PLAIN])


# ----------------------------------------------------------- the yardstick
def _worst(err, group, into, q):
    for g in np.unique(group):
        m = group == g
        if m.any():
            e = float(np.max(err[m])) if err[m].size else 0.0
            into.setdefault(str(g), {})
            into[str(g)][q] = max(into[str(g)].get(q, 0.0), e)


def measure(fam):
    """{group: {pos, vel, rew, rec}}: worst |fp32 restatement - fp64| of the family.
    rec is taken on the post-state of a step with uniform actions, the step that
    the records test takes (env_step_bench with all-zero actors)"""
    sc = scenario(*fam["scn"])
    p32, v32 = step_t(sc, fam["pos"], fam["vel"], fam["act"], F32)
    p64, v64 = step_t(sc, fam["pos"], fam["vel"], fam["act"], F64)
    out, grp = {}, fam["group"]
    E = len(grp)
    _worst(np.abs(p32 - p64).reshape(E, -1), grp, out, "pos")
    _worst(np.abs(v32 - v64).reshape(E, -1), grp, out, "vel")
    ok = decided(sc, p32)
    r32, r64 = reward_t(sc, p32, fam["goal"], F32), reward_t(sc, p32.astype(F64), fam["goal"], F64)
    _worst(np.abs(r32 - r64)[ok], grp[ok], out, "rew")
    if has_records(sc):
        u32, _ = step_t(sc, fam["pos"], fam["vel"], _uniform_actions(E, sc.n_agents), F32)
        ok = decided(sc, u32)
        b32, b64 = bench_t(sc, u32, fam["goal"], F32), bench_t(sc, u32.astype(F64), fam["goal"], F64)
        err = np.concatenate([np.abs(x - y) for x, y in zip(b32, b64)], 1)
        _worst(err[ok], grp[ok], out, "rec")
    return out


def bound(fam, q, ref):
    """max(FACTOR x the family's yardstick of each case's group, one fp32 spacing of |ref|):
    ref is [E, ...]; the bound has its shape"""
    ref = np.asarray(ref, F64)
    y = np.array([YARD[fam["id"]][g].get(q, 0.0) for g in fam["group"]])
    y = y.reshape((-1,) + (1,) * (ref.ndim - 1))
    return np.maximum(FACTOR * y, np.spacing(np.abs(ref).astype(F32)).astype(F64))
