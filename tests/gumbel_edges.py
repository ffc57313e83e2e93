"""Edge inputs for the Gumbel-softmax sample (host side only).

The device samples ``softmax(l - log(-log u))`` with the hardware
transcendentals (``gumbel_noise5`` / ``gumbel_softmax5_pre`` /
``gumbel_softmax_pre``, ``maddpg_amd/csrc/mdp_device.h``).  The builders here
put that function on the ends of its domain:

* ``exact_logit_actor``: actor parameters whose logits are ``s * obs[k]`` bit
  for bit in any fp32 summation order, so a table of logits can be handed to
  every kernel that runs an actor without the MLP's own rounding in the way;
* ``grid``: rows of 5 (or ``A`` live entries) over ``UNIFORMS`` x ``LOGITS``,
  the ends of the device's uniform grid (``u01``: k * 2^-23, 0 included) and
  logits of saturated policies;
* ``rollout_rows``: rows whose fifth logit is 0, the four others driven by an
  agent's own velocity and position observation entries;
* ``reference``: the sample in float64 on the fp32 inputs;
* ``E32_ABS`` / ``E32_REL``: the error of the fp32 restatement
  ``oracle.nets.gumbel_softmax`` against that reference on ``grid(5)`` -- the
  yardstick the device is held to (``tests/test_gumbel_edges_gpu.py``).
"""
import numpy as np

ACT = 5
F32 = np.float32
UNIFORMS = np.array([0.0, 2.0 ** -23, 2.0 ** -12, 0.25, 0.5, 1 - 2.0 ** -12, 1 - 2.0 ** -23], F32)
LOGITS = np.array([-80.0, -30.0, -4.0, 0.0, 0.5, 4.0, 30.0, 80.0], F32)
S = 128.0            # logit = S * obs entry: 80 / 128 and 0.5 / 128 are exact, and fit the MPE world
REL_FLOOR = 1e-30    # relative error is taken over entries whose reference probability exceeds this

# oracle.nets.gumbel_softmax (numpy fp32) against reference() on grid(5): worst
# absolute error and worst relative error over entries with p > REL_FLOOR, as
# baseline_e32() measured them (tests/test_gumbel_edges_oracle.py re-measures).
E32_ABS = 1.08e-7
E32_REL = 5.51e-6


def exact_logit_actor(obs_dim, H, act_w, s=S, drive=None):
    """Actor parameters (shapes of Engine.set_params) with logit_k = s * obs[drive[k]]
    exactly: W1 sends obs[drive[k]] to hidden units 2k (+1) and 2k + 1 (-1), W2 is
    the identity on those units, W3 has +s / -s, everything else is 0.  Then
    logit_k = s relu(x) - s relu(-x) with s a power of two, and every other
    product of the three layers is an exact zero.  drive[k] None: logit_k = 0."""
    drive = list(range(act_w)) if drive is None else list(drive)
    assert len(drive) == act_w and 2 * act_w <= H and float(s) == 2.0 ** round(np.log2(s))
    p = {"W1": np.zeros((obs_dim, H), F32), "b1": np.zeros(H, F32), "W2": np.zeros((H, H), F32),
         "b2": np.zeros(H, F32), "W3": np.zeros((H, act_w), F32), "b3": np.zeros(act_w, F32)}
    for k, d in enumerate(drive):
        if d is None:
            continue
        assert 0 <= d < obs_dim
        p["W1"][d, 2 * k], p["W1"][d, 2 * k + 1] = 1.0, -1.0
        p["W2"][2 * k, 2 * k] = p["W2"][2 * k + 1, 2 * k + 1] = 1.0
        p["W3"][2 * k, k], p["W3"][2 * k + 1, k] = s, -s
    return p


def obs_for(logits, obs_dim, s=S, drive=None):
    """[R, obs_dim] observations on which exact_logit_actor(.., drive) gives `logits`"""
    logits = np.asarray(logits, F32)
    drive = list(range(logits.shape[1])) if drive is None else list(drive)
    obs = np.zeros((logits.shape[0], obs_dim), F32)
    for k, d in enumerate(drive):
        if d is None:
            assert np.all(logits[:, k] == 0)
        else:
            obs[:, d] = logits[:, k] / F32(s)
    assert np.array_equal(obs[:, [d for d in drive if d is not None]] * F32(s),
                          logits[:, [k for k, d in enumerate(drive) if d is not None]])
    return obs


def reference(logits, u):
    """softmax(l - log(-log u)) in float64 on the fp32 inputs; an entry with u == 0
    (Gumbel noise +inf) has probability exactly 0"""
    l64, u64 = np.asarray(logits, np.float64), np.asarray(u, np.float64)
    assert not np.any(np.all(u64 == 0, -1)), "a row of zeros has no sample (NaN in TF1 too)"
    with np.errstate(divide="ignore"):
        z = l64 - np.log(-np.log(u64))
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    assert np.all(p[u64 == 0] == 0) and np.all(np.isfinite(p))
    return p


def errors(got, ref):
    """(worst |got - ref|, worst |got - ref| / ref over ref > REL_FLOOR)"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    m = ref > REL_FLOOR
    return float(d.max()), float((d[m] / ref[m]).max())


def special_rows():
    """rows the rotations of grid() do not hold: two tied maxima with a third entry
    0.5 below them; one entry at 1 - 1.7e-7 beside entries at 1.7e-7, 1.6e-9, 2.9e-22
    and one below 1e-30;
    the largest and the smallest uniform on the same logit; a zero uniform on the
    largest logit (the would-be winner is exactly 0)"""
    top, tiny = UNIFORMS[6], UNIFORMS[1]
    lg = np.array([[0.5, 0.0, 0.5, -4.0, -30.0],
                   [4.0, 4.0, -30.0, -80.0, 0.0],
                   [4.0, 4.0, 4.0, 4.0, 4.0],
                   [80.0, 30.0, 4.0, 0.0, -80.0]], F32)
    u = np.array([[0.5, 0.5, 0.5, 0.25, 0.25],
                  [top, 0.5, 0.5, 0.5, 0.25],
                  [top, tiny, 0.5, top, tiny],
                  [0.0, 0.5, 0.0, 0.25, top]], F32)
    return lg, u


def grid(width=ACT):
    """(logits [R, width], u [R, width]): rows (i, j) with entry k at
    LOGITS[(i + k) % 8] and UNIFORMS[(j + 2 k) % 7] -- entry 0 alone meets every
    (uniform, logit) pair, and the uniforms of a row are distinct, so no row is
    all zeros -- followed by special_rows().  width 1: a lone entry at u == 0 is
    the all-zeros row, so that uniform is left out there."""
    lg, u = [], []
    for i in range(len(LOGITS)):
        for j in range(len(UNIFORMS)):
            if width == 1 and UNIFORMS[j] == 0:
                continue
            lg.append([LOGITS[(i + k) % 8] for k in range(ACT)])
            u.append([UNIFORMS[(j + 2 * k) % 7] for k in range(ACT)])
    sl, su = special_rows()
    lg, u = np.concatenate([np.array(lg, F32), sl])[:, :width], np.concatenate([np.array(u, F32), su])[:, :width]
    if width == 1:
        keep = u[:, 0] != 0
        lg, u = lg[keep], u[keep]
    check_inputs(lg, u, pairs=True)
    return np.ascontiguousarray(lg), np.ascontiguousarray(u)


def rollout_rows(E, agent, width=ACT, driven=4):
    """(logits [E, width], u [E, width]) for one agent of a vector step: entry k <
    driven at LOGITS[(e + agent + 3 k) % 8], the rest at 0; uniforms
    UNIFORMS[(e + 2 agent + 3 k) % 7] (distinct within a row).  Positions made of
    entries 2 and 3 differ between the agents of one env (agent < 8).  The last
    row's first entry is the largest logit under the largest uniform (z = 95.9:
    exp overflows unless the row's maximum is subtracted first)."""
    e = np.arange(E)[:, None]
    k = np.arange(ACT)[None, :]
    lg = LOGITS[(e + agent + 3 * k) % 8]
    lg[:, driven:] = 0
    u = UNIFORMS[(e + 2 * agent + 3 * k) % 7]
    if driven:
        lg[-1, 0] = LOGITS[-1]
    u[-1, 0] = UNIFORMS[-1]
    lg, u = np.ascontiguousarray(lg[:, :width]), np.ascontiguousarray(u[:, :width])
    check_inputs(lg[:, :min(width, driven)], u)
    return lg, u


def check_inputs(lg, u, pairs=False):
    """the conditions on a set of rows: no row with every live uniform 0; every edge
    value present (a width-1 set cannot hold u == 0); with pairs, every uniform
    meets every logit in some entry, some row has two tied maxima and some row an
    entry above 1 - 1e-6"""
    assert not np.any(np.all(u == 0, -1))
    lone = u.shape[1] == 1
    assert set(np.unique(u)) == set(UNIFORMS[1:] if lone else UNIFORMS), np.unique(u)
    assert lg.shape[1] == 0 or set(LOGITS) <= set(np.unique(lg)), np.unique(lg)
    if pairs:
        w = min(lg.shape[1], u.shape[1])
        seen = {(float(a), float(b)) for a, b in zip(u[:, :w].ravel(), lg[:, :w].ravel())}
        want = {(float(a), float(b)) for a in UNIFORMS for b in LOGITS if not (lone and a == 0)}
        assert want <= seen
        p = reference(lg, u)
        assert (p > 1 - 1e-6).any()
        if not lone:
            top2 = np.sort(p, -1)[:, -2:]
            assert np.any((top2[:, 0] == top2[:, 1]) & (top2[:, 1] > 0.3))


def baseline_e32(width=ACT):
    """errors of the fp32 restatement on grid(width)"""
    from oracle import nets
    lg, u = grid(width)
    return errors(nets.gumbel_softmax(lg, u), reference(lg, u))


def ulp_sum_error(a):
    """|sum of a row - 1| in units of ulp(1) = 2^-23, the row summed in float64"""
    return np.abs(np.asarray(a, np.float64).sum(-1) - 1.0) / 2.0 ** -23


def saturate(params, s):
    """every actor's and target actor's W3 / b3 times the power of two s (in place):
    the logits of a trained, saturated policy on the case's Xavier nets"""
    assert float(s) == 2.0 ** round(np.log2(s))
    for p in params:
        for w in ("actor", "tgt_actor"):
            p[w]["W3"] = (p[w]["W3"] * F32(s)).astype(F32)
            p[w]["b3"] = (p[w]["b3"] * F32(s)).astype(F32)


# The update tests' factor on every actor's W3 / b3: the largest power of two at
# which, on the [18, 18, 18] case (B = 40, L = 300, seed SEED_UPDATE), (1) some
# batch row has a sampled probability above 1 - 1e-6, (2) the oracle's fp32
# gradients stay within a quarter of the update tests' gradient bound (1e-5 of
# the tensor's largest entry) of the same oracle in fp64, and (3) one ulp of
# the largest scaled weight is at most half the update tests' bound on a
# well-conditioned weight (1e-6 absolute, tests/test_gpu_parity.py).  (1) and
# (2) hold at every power of two from 1 to 2^30 -- the edge uniform 1 - 2^-23
# alone puts 15.9 on a logit, and a saturated softmax passes no gradient to
# round -- so (3) decides: two correct fp32 Adam steps may round a weight to
# neighbouring floats, and from |w| >= 16 that alone is 1.9e-6, more than the
# bound whatever the kernels do; half the bound for the rounding leaves the
# other half for the step's own error, which is what the bound was set for.
# Xavier W3 of a 64 -> 5 layer is within 0.295: 16 x 0.295 = 4.7 (ulp 4.8e-7),
# 32 x 0.295 = 9.4 (ulp 9.5e-7).  tests/test_gumbel_edges_oracle.py asserts all
# three at S_UPDATE and that (3) fails at 2 * S_UPDATE.
S_UPDATE = 16.0
SEED_UPDATE = 51
WEIGHT_BOUND = 1e-6  # tests/test_gpu_parity.py::_update_parity, conditioned weights, absolute
GRAD_BOUND = 1e-5    # ... and its gradient bound, of the tensor's largest entry


def largest_weight_ulp(c):
    """one fp32 ulp of the largest actor / target actor W3 or b3 entry of the case"""
    m = max(float(np.abs(p[w][k]).max()) for p in c["params"] for w in ("actor", "tgt_actor") for k in ("W3", "b3"))
    return float(np.spacing(F32(m)))


# batch rows that carry edge uniforms in the update tests, and what they carry
EDGE_ROWS = (1, 7, 16, 23, 39)       # both 16-row tiles and the ragged third of B = 40
EDGE_U = np.array([[0.0, 0.5, 0.25, UNIFORMS[5], UNIFORMS[2]],
                   [UNIFORMS[6], 0.25, 0.5, UNIFORMS[1], 0.5],
                   [0.5, 0.0, UNIFORMS[6], 0.0, UNIFORMS[1]],
                   [UNIFORMS[1], UNIFORMS[6], 0.0, 0.5, 0.0],
                   [UNIFORMS[2], UNIFORMS[5], UNIFORMS[6], 0.25, 0.0]], F32)


def put_edge_noise(c, widths=None, shift=0):
    """overwrite batch rows (EDGE_ROWS + shift) % B of every u_tgt[i][j] and u_act[i]
    with EDGE_U, each (i, j) starting at another of its rows; every agent then has
    a 0 and a 1 - 2^-23 in live entries (narrow agents within their first A_j
    columns; their pad columns are NaN in those rows: never used)"""
    n = len(c["params"])
    widths = [ACT] * n if widths is None else widths
    rows = (np.array(EDGE_ROWS) + shift) % c["u_act"].shape[1]
    for i in range(n):
        for j in range(n + 1):                      # j == n: the actor step's sample of agent i
            w = widths[i] if j == n else widths[j]
            blk = np.roll(EDGE_U, i + j, axis=0)
            tgt = c["u_act"][i] if j == n else c["u_tgt"][i][j]
            tgt[rows] = blk
            tgt[rows, w:] = np.nan
            live = tgt[rows][:, :w]
            assert not np.any(np.all(live == 0, -1))
            if w > 1:
                assert (live == 0).any() and (live == UNIFORMS[6]).any(), (i, j, w)
    return rows


def saturated_case(dims, B, L, seed, s, widths=None, H=64, local_q=None):
    """the update tests' case: synthetic_trainer_case (mixed_case with widths), the
    actors' last layers times s, edge uniforms in batch rows EDGE_ROWS + shift, then
    a batch with no ReLU input on the margin.  The cleaning may replace at most
    10 % of the n * B positions and must leave the edge rows' indices in place:
    the smallest shift at which it does is taken (c["shift"])."""
    from tests.helpers import relu_margin_clean_idx, synthetic_trainer_case
    for shift in range(B):
        if widths is None:
            c = synthetic_trainer_case(dims, B, L, seed, local_q, H)
        else:
            from tests import mixed_width as mw
            c = mw.mixed_case(dims, widths, B, L, seed, local_q, H)
        saturate(c["params"], s)
        rows = put_edge_noise(c, widths, shift)
        before = c["idx"][:, rows].copy()
        replaced = relu_margin_clean_idx(c)
        if np.array_equal(c["idx"][:, rows], before):
            break
    else:
        raise AssertionError("every choice of edge rows has one the cleaning replaces")
    assert replaced <= 0.1 * len(dims) * B, replaced
    c.update(replaced=replaced, shift=shift, edge_rows=rows)
    return c


def oracle_gap(c, widths=None, throughput=False):
    """(worst |g32 - g64| / max|g64| over every gradient tensor of one round of the
    oracle run in fp32 and in fp64, largest sampled probability and largest |logit|
    of the fp64 run)"""
    import copy

    from oracle import nets, trainer
    from tests.test_oracle_autograd import fp64_oracle
    n = len(c["params"])
    lq = c["local_q"]

    def run():
        agents = [trainer.AgentParams(**copy.deepcopy(p), local_q=lq[i]) for i, p in enumerate(c["params"])]
        out, top, lmax = [], 0.0, 0.0
        for i in range(n):
            batch_n = [tuple(x[c["idx"][i]] for x in c["data"][j]) for j in range(n)]
            for j in range(n):
                w = ACT if widths is None else widths[j]
                top = max(top, float(trainer.target_act(agents[j], batch_n[j][3], c["u_tgt"][i][j][:, :w]).max()))
                lmax = max(lmax, float(np.abs(nets.mlp_fwd(agents[j].tgt_actor, batch_n[j][3])[0]).max()))
            w = ACT if widths is None else widths[i]
            top = max(top, float(trainer.act(agents[i], batch_n[i][0], c["u_act"][i][:, :w]).max()))
            lmax = max(lmax, float(np.abs(nets.mlp_fwd(agents[i].actor, batch_n[i][0])[0]).max()))
            if throughput:
                from tests import mixed_width as mw
                u_t = c["u_tgt"][i] if widths is None else mw.narrow(c["u_tgt"][i], widths)
                gq = trainer.critic_grads(agents, i, batch_n, u_t)[0]
                gp = (trainer.actor_grads if widths is None else mw.actor_grads)(agents, i, batch_n, c["u_act"][i])[0]
                out.append({"grad_critic": gq, "grad_actor": gp})
            elif widths is None:
                out.append(trainer.update(agents, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i])[1])
            else:
                from tests import mixed_width as mw
                out.append(mw.update(agents, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], widths)[1])
        return out, top, lmax

    g32, _, _ = run()
    with fp64_oracle():
        g64, top, lmax = run()
    worst = 0.0
    for a, b in zip(g32, g64):
        for name in a:
            for k in a[name]:
                r64 = np.asarray(b[name][k], np.float64)
                scale = float(np.abs(r64).max()) or 1.0
                worst = max(worst, float(np.abs(np.asarray(a[name][k], np.float64) - r64).max()) / scale)
    return worst, top, lmax


# A seed at which the device's own first act() draw of agent ZERO_AGENT holds an
# exact 0: uniforms5(seed, 0x40000 | agent << 1, 0, row)[entry] with the word's
# top 23 bits zero.  Found by
#     for seed in range(2 ** 27 // 80):
#         u = philox.uniforms5(seed, 0x40000, 0, np.arange(16))
#         if (u == 0).any(): print(seed, np.argwhere(u == 0)); break
# (80 words per seed, one hit expected per 2^23 / 80 = 104,858 seeds).
ZERO_SEED, ZERO_AGENT, ZERO_ROW, ZERO_ENTRY = 295278, 0, 15, 4
