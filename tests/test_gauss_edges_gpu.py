"""GPU: the diagonal-Gaussian sample and its tanh squash (gauss_noise2 /
gauss_sample_pre / gauss_backward / the Box branch of policy_sample_pre,
mdp_device.h) on the ends of their inputs, at every kernel they are inlined
into, against the float64 reference of tests/gauss_edges.py.

Inputs: the grid of tests/gauss_edges.py (u0 and u1 on 0, 2^-23 .. 1 - 2^-23 and
the quarter turns, means -80 .. 80, logstd -100 .. 80), handed to the kernels
through an actor whose head is 128 * obs[k] bit for bit (exact_logit_actor).

On every site (_check): all outputs float32 and finite; pad columns [d:5]
exactly 0.0f; a row whose true eps_k is 0 (u0 = 0, or u1 on a quarter turn)
holds exactly mean_k, or, squashed, the one value tanhf(mean_k) that every such
row of that mean holds in the canonical run (_tanhf_table: no host tanhf is
bit-exact, so the absolute bound is what ties that value to the truth); rows at logstd = -100 likewise (on a zero
mean the sample is std * eps itself, a denormal: at most 2.2e-43); squashed:
|a| <= 1 and exactly +-1.0f where |z| >= 10; the error against the reference at
most 2 x e32 in each form, e32 being the error of the numpy float32 restatement
on the same grid (E32_PLAIN_REL = 1.43e-7 relative to |mean| + std |eps| where
that scale is at least FLT_MIN, E32_DENORM = 2.10 units of 2^-149 on the
denormal entries -- a zero mean at logstd -100 -- judged on their own,
E32_SQ_ABS = 2.34e-7, E32_T_ABS = 1.28e-7 for 1 - a^2 against sech^2: bounds
2.86e-7, 4.2 units, 4.68e-7, 2.56e-7).  The factor 2: the device's logf / expf / sincospif
/ tanhf are the precise forms, specified to 1-2 ulp where numpy's are within 1,
and the operation order is the restatement's.  The same (head, u) row must give
the same bits at every site, row position, row count and H.

Observed on MI355X (worst over the site's rows), against the bounds plain rel
2.86e-7 / denormal entries 4.2 x 2^-149 / squashed abs 4.68e-7 / 1 - a^2 abs 2.56e-7:
  k_mlp_eval d=2, H = 64 / 128 / 256, both nets       1.32e-7 / 2.10 / 2.35e-7 / 2.47e-7
  k_mlp_eval d=1, H = 64 / 128 / 256                  1.32e-7 / 2.10 / 2.35e-7 / 1.04e-7
  k_mlp_eval, the plain agent of a squashed handle    1.32e-7 / 2.10 / -       / -
  k_rollout wave per agent (spread N=3, H=64)         8.6e-8  / -    / 4.7e-8  / 8.5e-8
  k_rollout mlp_fwd_tile_pf (tag N=6, H=64)           1.02e-7 / -    / 4.7e-8  / 8.5e-8
  k_rollout mlp_fwd_tile (spread, tag N=6, H=128)     1.02e-7 / -    / 4.7e-8  / 8.5e-8
  k_mlp_eval, the device's own draw of u0 = 0         9.6e-8  / -    / 2.9e-8  / 8.5e-8
(the denormal entries are bit-equal to numpy's; the rollout rows and the own draw
hold none.)
(1 - a^2 carries the action's own error times 2 |a|, so the d = 2 figure, 2.47e-7,
sits beside the action's 2.35e-7; it is inside its bound, and is the same bits
on every run.)  The same bits at every site, row position, row count and H.
k_eval_episodes in mean mode: returns bit-equal to the step chain played with the
exact mode (largest |action| 0.9951 squashed, 1.5584 plain), logstd 89 included.
Strict round on the saturated cases (gradient / any weight): t2_t2_b40 2.0e-6 /
2.5e-5 with 64 actions at +-1.0f, box2_t2 1.6e-6 / 5.8e-5 with 3.  The
regulariser-only b3 gradient: within 2.2e-9 of the sum (tolerance 2.5e-9 .. 4.3e-8).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd.engine import Engine  # noqa: E402
from maddpg_amd.envs import spec  # noqa: E402
from tests import box_squash as bs  # noqa: E402
from tests import eval_oracle as eo  # noqa: E402
from tests import gauss_edges as gs  # noqa: E402
from tests import gumbel_edges as ge  # noqa: E402
from tests.helpers import row_layout  # noqa: E402

ACT = 5
OBS = 18
F32 = np.float32
BOUND_PLAIN, BOUND_SQ, BOUND_T = 2 * gs.E32_PLAIN_REL, 2 * gs.E32_SQ_ABS, 2 * gs.E32_T_ABS
BOUND_DENORM = 2 * gs.E32_DENORM       # units of 2^-149, the plain entries whose scale is below FLT_MIN
# the target actor reads its head from other observation entries than the actor
TGT_DRIVE = [OBS - 1 - k for k in range(4)]


def _check(site, got, head, u, d, squash):
    """the assertions every site must meet; got [R, 5] (pad columns included) or [R, d]"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and np.isfinite(got).all(), site
    live, mean, logstd = got[:, :d], head[:, :d], head[:, d:]
    assert np.all(got[:, d:] == 0), site
    rel, den, ab, tt = gs.errors(live, head, u, d, squash)
    print(f"GAUSS_EDGES {site}: plain rel {rel:.3e} denormal {den:.3f} x 2^-149 squashed abs {ab:.3e} "
          f"1-a^2 abs {tt:.3e} ({len(head)} rows)")
    lost = (logstd == -100) & (mean != 0)          # std = 3.7e-44: below half an ulp of every other mean
    exact = gs.eps_is_zero(u, d) | lost
    if not squash:
        assert np.array_equal(live[exact], mean[exact]), site
    else:
        tab = _tanhf_table()
        assert np.array_equal(live[exact], np.array([tab[float(m)] for m in mean[exact]], F32)), site
        assert np.abs(live).max() <= 1.0, site
        z64 = gs.reference(head, u, d, False)[0]
        assert np.array_equal(live[np.abs(z64) >= 10], np.sign(z64[np.abs(z64) >= 10]).astype(F32)), site
    tiny = (logstd == -100) & (mean == 0)
    assert np.all(np.abs(live[tiny]) <= 2.2e-43), site
    assert rel <= BOUND_PLAIN, (site, rel, BOUND_PLAIN)
    assert den <= BOUND_DENORM, (site, den, BOUND_DENORM)
    assert ab <= BOUND_SQ, (site, ab, BOUND_SQ)
    assert tt <= BOUND_T, (site, tt, BOUND_T)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _kw(n, d, squash):
    """Engine arguments of n Box(d) agents; squash: one bool for all, or one per agent"""
    sq = [squash] * n if isinstance(squash, bool) else list(squash)
    kw = dict(act_kinds=["box"] * n, act_dims=[d] * n)
    if any(sq):
        kw["act_squash"] = ["tanh" if s else "none" for s in sq]
    return kw


def _act_engine(H, d, squash, n=1, **kw):
    eng = Engine([OBS] * n, num_units=H, batch_size=16, capacity=64, **_kw(n, d, squash), **kw)
    eng.init_params(0)
    for j in range(n):
        eng.set_params(j, "actor", gs.head_actor(OBS, H, d))
        eng.set_params(j, "tgt_actor", gs.head_actor(OBS, H, d, drive=TGT_DRIVE[:2 * d]))
    return eng


def _obs(head, target):
    return torch.from_numpy(ge.obs_for(head, OBS, drive=TGT_DRIVE[:head.shape[1]] if target else None))


def _act_chunks(eng, agent, head, u, R, target):
    """act() on the whole set in calls of exactly R rows (the last one wraps round): [len, d]"""
    N, d = len(head), head.shape[1] // 2
    out = np.full((N, d), np.nan, np.float32)
    for start in range(0, N, R):
        rows = (start + np.arange(R)) % N
        got = eng.act(agent, _obs(head[rows], target), target=target, u=torch.from_numpy(u[rows])).cpu().numpy()
        assert got.shape == (R, d)
        fresh = rows[:min(R, N - start)]
        out[fresh] = got[:len(fresh)]
        again = rows[len(fresh):]           # a row seen before (the wrap) has the bits it had at its first position
        assert np.array_equal(_bits(got[len(fresh):]), _bits(out[again]))
    return out


@functools.lru_cache(maxsize=None)
def _canonical(d, squash):
    """the grid through act() at H = 64 in 40-row calls: what every other site must reproduce"""
    head, u = gs.grid(d)
    return _act_chunks(_act_engine(64, d, squash), 0, head, u, 40, False)


@functools.lru_cache(maxsize=None)
def _tanhf_table():
    """mean -> tanhf(mean) as the device gives it, for the grid's nine means: read from
    the canonical squashed run's rows whose eps is exactly 0 or whose std is lost,
    which must hold one value per mean.  No host tanhf is bit-exact, so the
    exactness check compares every site with this table; what ties the table to
    the truth is _check's absolute bound on the canonical run itself (2 x
    E32_SQ_ABS against tanh in float64), and tanhf(0) = 0, tanhf(+-80) = +-1."""
    head, u = gs.grid(2)
    got = _canonical(2, True)
    mean, logstd = head[:, :2], head[:, 2:]
    exact = gs.eps_is_zero(u, 2) | ((logstd == -100) & (mean != 0))
    tab = {}
    for m in gs.MEAN:
        vals = np.unique(got[exact & (mean == m)] + F32(0))
        assert len(vals) == 1, (m, vals)
        assert abs(float(vals[0]) - np.tanh(float(m))) <= BOUND_SQ
        tab[float(m)] = vals[0]
    assert tab[0.0] == 0 and tab[80.0] == 1 and tab[-80.0] == -1
    return tab


def _assert_head_table(eng, agent, head):
    """actor_logits returns the head table bit for bit (k_mlp_eval, current and target nets)"""
    for target in (False, True):
        for start in range(0, len(head), 40):
            rows = (start + np.arange(40)) % len(head)
            got = eng.actor_logits(agent, _obs(head[rows], target), target=target).cpu().numpy()
            assert got.shape == (40, head.shape[1]) and np.array_equal(got, head[rows]), (agent, target)
            nz = head[rows] != 0
            assert np.array_equal(_bits(got)[nz], _bits(head[rows])[nz])


@pytest.mark.parametrize("d", [2, 1])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_act_on_the_edge_grid(H, d):
    """k_mlp_eval through Engine.act: row counts 40, 17, 16 (ragged against the 16-row
    tile) and 1 (the facade's action()), current and target nets, on a plain and on
    a squashed handle; then a handle with one plain and one squashed agent -- the
    plain agent runs the SQ instantiation and its width mask, and must equal the
    all-plain handle bit for bit -- and the raw 5-wide slot"""
    head, u = gs.grid(d)
    for squash in (False, True):
        eng = _act_engine(H, d, squash)
        _assert_head_table(eng, 0, head)
        first = None
        for R in (40, 17, 16, 1):
            for target in (False, True):
                got = _act_chunks(eng, 0, head, u, R, target)
                if first is None:
                    first = got
                    _check(f"k_mlp_eval H={H} d={d} {'squashed' if squash else 'plain'}", got, head, u, d, squash)
                assert np.array_equal(_bits(got), _bits(first)), (H, d, squash, R, target)
        assert np.array_equal(_bits(first), _bits(_canonical(d, squash))), "H = 64 and this H differ in bits"
        # the raw 5-wide slot, NaN in the unread uniforms: pad columns exactly 0
        out = torch.full((40, ACT), 7.0, dtype=torch.float32, device=eng.device)
        rows = np.arange(len(head) - 40, len(head))                     # the special rows among them
        obs = _obs(head[rows], False).to(eng.device).contiguous()
        ud = torch.from_numpy(u[rows]).to(eng.device).contiguous()
        assert torch.isnan(ud[:, 2:]).all()
        eng.sync_in()
        eng._c("mdp_act", 0, 0, eng._ptr(obs), eng._ptr(out), 40, eng._ptr(ud))
        eng.sync_out()
        raw = out.cpu().numpy()
        assert np.all(raw[:, d:] == 0) and np.array_equal(_bits(raw[:, :d]), _bits(first[rows])), (H, d, squash)
        eng.close()
    mixed = _act_engine(H, d, [False, True], n=2)
    for agent, squash in ((0, False), (1, True)):
        _assert_head_table(mixed, agent, head)
        for R, target in ((40, False), (17, True)):
            got = _act_chunks(mixed, agent, head, u, R, target)
            assert np.array_equal(_bits(got), _bits(_canonical(d, squash))), (H, d, agent, R, target)
    _check(f"k_mlp_eval H={H} d={d} plain agent of a squashed handle", _act_chunks(mixed, 0, head, u, 40, False),
           head, u, d, False)
    mixed.close()


# ---------------------------------------------------------------- k_rollout
DRIVE = [0, 1, 2, 3]             # own velocity (obs 0, 1): the means; own position (obs 2, 3): the logstds


@pytest.mark.parametrize("squash", [True, False], ids=["squashed", "plain"])
@pytest.mark.parametrize("name,n,na,H,path", [
    ("simple_spread", 3, 0, 64, "wave per agent"),
    ("simple_tag", 6, 4, 64, "mlp_fwd_tile_pf"),
    ("simple_spread", 3, 0, 128, "mlp_fwd_tile"),
    ("simple_tag", 6, 4, 128, "mlp_fwd_tile"),
])
def test_rollout_on_the_edge_rows(name, n, na, H, path, squash):
    """k_rollout's policy forward through Engine.env_step(u=...) after set_env_state,
    E = 17, every agent Box(2): the heads driven by each agent's own velocity and
    position observation entries, the stored actions read from the replay rows.
    A plain handle's actions reach 3e35 and its next state may overflow (the
    reason the squash exists): only its observation and action columns are
    judged; a squashed handle's whole row is finite."""
    E = 17
    sp = spec(name, n, na if na else None)
    eng = Engine(sp.obs_dims, num_units=H, batch_size=16, capacity=64, num_envs=E, scenario=name,
                 num_adversaries=sp.num_adversaries, max_episode_len=25, seed=3, **_kw(n, 2, squash))
    eng.init_params(0)
    for j, o in enumerate(sp.obs_dims):
        eng.set_params(j, "actor", gs.head_actor(o, H, 2, drive=DRIVE))
    eng.env_reset()
    st = eng.env_state()
    pos, vel = st["pos"].copy(), st["vel"].copy()
    tab = [gs.rollout_rows(E, j) for j in range(n)]
    for j in range(n):
        vel[:, j] = tab[j][0][:, 0:2] / np.float32(gs.S)
        pos[:, j] = tab[j][0][:, 2:4] / np.float32(gs.S)
    for l in range(pos.shape[1] - n):                     # landmarks: apart from every agent
        pos[:, n + l] = (0.9, -0.9 + 0.2 * l)
    dd = pos[:, :, None] - pos[:, None]
    assert np.all(np.abs(dd).max(-1)[:, ~np.eye(pos.shape[1], dtype=bool)] > 0)
    eng.set_env_state(pos, vel, st["goal"], st["ep_step"])
    u = np.stack([t[1] for t in tab], 1)                  # [E, n, 5], NaN in the unread three
    eng.env_step(u=torch.from_numpy(u))
    rows = eng.replay_rows(0, E).cpu().numpy()
    lay, _ = row_layout(sp.obs_dims)
    canon = _act_engine(64, 2, squash)
    for j in range(n):
        head, uj = tab[j]
        lj, o = lay[j], sp.obs_dims[j]
        obs = rows[:, lj["obs"]:lj["obs"] + o]
        assert np.isfinite(obs).all()
        assert np.array_equal(obs[:, :4] * np.float32(gs.S), head), "the driven observation entries"
        assert np.array_equal(eng.actor_logits(j, torch.from_numpy(obs)).cpu().numpy(), head)
        got = rows[:, lj["act"]:lj["act"] + ACT]
        _check(f"k_rollout {path} {name} n={n} H={H} {'squashed' if squash else 'plain'} agent {j}",
               got, head, uj, 2, squash)
        # the same rows through act(): on this handle, and on the H = 64 canonical one at reversed row order
        same = eng.act(j, torch.from_numpy(obs), u=torch.from_numpy(uj)).cpu().numpy()
        assert np.array_equal(_bits(got[:, :2]), _bits(same)), (path, j)
        back = np.arange(E)[::-1].copy()
        other = canon.act(0, torch.from_numpy(ge.obs_for(head[back], OBS)), u=torch.from_numpy(uj[back])).cpu().numpy()
        assert np.array_equal(_bits(got[back, :2]), _bits(other)), (path, j)
    assert eng.buffer_len() == E
    if squash:
        assert np.isfinite(rows).all()


# ---------------------------------------------------------- k_eval_episodes
EVAL_LOGSTD = (-100.0, 80.0, 89.0)     # per agent; 89: std = inf, which mode() must never multiply by a zero eps
EP = 32
SEED = 0x0123456789ABCDEF


def _eval_engine(num_envs, squash, s):
    eng = eo.make_engine("spread3", num_envs, SEED, **_kw(3, 2, squash))
    for j, o in enumerate(eng.obs_dims):
        p = gs.head_actor(o, 64, 2, drive=[2, 3, None, None], s=s)          # mean = s * own position
        p["b3"][2:4] = EVAL_LOGSTD[j]                                        # logstd = b3 alone: 0 + b3
        eng.set_params(j, "actor", p)
    return eng


@pytest.mark.parametrize("squash,s", [(True, 2.0), (False, 1.0)], ids=["squashed", "plain"])
def test_evaluation_mean_mode_plays_the_mean_at_any_std(squash, s):
    """k_eval_episodes with mode="mean" on heads whose logstd is -100, 80 and 89 (std =
    inf): the returns are, bit for bit, those of the step chain on the same start
    states (as test_evaluation_is_the_step_chain_bit_for_bit observes them) stepped
    with act_in = exactly the mean, or tanhf(mean) as k_mlp_eval gives it under an
    eps of exactly 0; nothing is NaN; u is never read (the call refuses one)"""
    a = _eval_engine(4, squash, s)
    start = a.eval_initial_state(EP, 0)
    got = a.evaluate(EP, 0, mode="mean")["returns"].cpu().numpy()
    assert np.isfinite(got).all() and np.any(got != 0)
    from maddpg_amd._lib import MdpError
    with pytest.raises(MdpError, match="draws no noise"):          # u is never read: giving one is refused
        a.evaluate(EP, 0, mode="mean", u=torch.full((EP, eo.T, 3, ACT), float("nan")))
    again = a.evaluate(EP, 0, mode="mean")["returns"].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(again))
    b = _eval_engine(EP, squash, s)
    b.set_env_state(start["pos"], start["vel"], start["goal"])
    tanhf = _act_engine(64, 2, True) if squash else None
    seen = 0.0
    for t in range(eo.T):
        def mode(j, flat):
            assert np.all(flat[:, 2:] == EVAL_LOGSTD[j])
            mean = np.ascontiguousarray(flat[:, :2])
            if not squash:
                return mean
            # tanhf(mean) of the device: act() with u0 = 0 (eps = 0) under logstd = -100
            head = np.concatenate([mean, np.full_like(mean, -100.0)], 1)
            obs = np.zeros((len(head), OBS), F32)
            obs[:, :4] = head / F32(gs.S)
            assert np.array_equal(obs[:, :4] * F32(gs.S), head)
            u0 = torch.tensor([[0.0, 0.125]] * len(head))
            return tanhf.act(0, torch.from_numpy(obs), u=u0).cpu().numpy()
        act = eo.host_actions(b, mode)
        seen = max(seen, float(act.abs().max()))
        b.env_step(act_in=act)
    b.synchronize()
    assert b.episode_count() == EP
    want = b.episode_log(0, EP)[:, 1:].copy()
    print(f"GAUSS_EDGES k_eval_episodes mean mode {'squashed' if squash else 'plain'}: largest |action| {seen:.4f}")
    assert np.isfinite(want).all()
    np.testing.assert_array_equal(got, want)
    if squash:
        assert 0.5 < seen <= 1.0


# ------------------------------------------------- backward and the optimizer
def _all_finite(eng):
    """after the step: no NaN / Inf in any parameter, Adam slot, gradient or stat"""
    eng.synchronize()
    assert eng.check_finite() == 0
    for name in ("theta", "target", "adam_m", "adam_v", "grad"):
        assert np.isfinite(eng.region(name).cpu().numpy()[:eng.param_floats]).all(), name
    for i in range(eng.n):
        assert np.all(np.isfinite(eng.stats(i))), i


@pytest.mark.parametrize("name", list(gs.UPDATE_CASES))
def test_update_saturated_policies_with_edge_noise(name):
    """one strict round on actors scaled by S_UPDATE = 16 (squashed samples at exactly
    +-1.0f beside unsaturated rows) with the edge uniforms in five batch rows per
    noise array, by _check_agent and _check_adam at their bounds as written.  The
    restatement alone sits within a quarter of the gradient bound of its float64
    self on these cases (tests/test_gauss_edges_oracle.py)."""
    from tests.test_act_dims_gpu import _check_agent
    from tests.test_box_actions_gpu import _check_adam
    from tests.test_box_squash_gpu import _agents, _engine
    c = gs.saturated_case(name)
    B = c["B"]
    eng = _engine(c, B, 64)
    n = len(c["dims"])
    assert [eng.lib.mdp_grad_variant(eng.h, i) for i in range(n)] == [0] * n and eng.act_squash == c["squash"]
    agents = _agents(c)
    ones = 0
    for j in range(n):
        if bs.is_squashed(c["spaces"][j]):
            obs = torch.from_numpy(c["data"][j][0][c["idx"][j]])
            a = eng.act(j, obs, u=torch.from_numpy(c["u_act"][j])).cpu().numpy()
            assert np.isfinite(a).all() and np.abs(a).max() <= 1.0
            ones += int(np.count_nonzero(np.abs(a) == 1.0))
    assert ones >= 1, "no sampled action at exactly +-1.0f"
    wg = ww = 0.0
    for i in range(n):
        eng.update(i, idx=torch.from_numpy(c["idx"][i]), u_tgt=torch.from_numpy(c["u_tgt"][i]),
                   u_act=torch.from_numpy(c["u_act"][i]))
        got = eng.stats(i)
        with np.errstate(over="ignore"):
            want, og = bs.update(agents, i, c["data"], c["idx"][i], c["u_tgt"][i], c["u_act"][i], c["spaces"])
        g, w = _check_agent(eng, i, agents, got, want, og)
        _check_adam(eng, i, agents)
        wg, ww = max(wg, g), max(ww, w)
    print(f"GAUSS_EDGES strict round {name}: {ones} actions at +-1.0f, worst grad |diff|/max|g| = {wg:.3e}, "
          f"worst param |diff| = {ww:.3e}")
    _all_finite(eng)
    # throughput mode (k_grad_pair) does not admit a Box handle: the refusal, and the handle goes on
    assert eng.lib.mdp_set_update_mode(eng.h, 1) < 0 and b"Box action space" in eng.lib.mdp_last_error(eng.h)
    assert eng.lib.mdp_update_all(eng.h, None, None, None) < 0 and b"Box action space" in eng.lib.mdp_last_error(eng.h)
    _all_finite(eng)


def _set_head(c, agent, mean_b3, logstd_b3):
    """agent's actor: logstd = logstd_b3 on every row (its W3 columns 0), b3 of the means as given"""
    p = c["params"][agent]["actor"]
    d = c["widths"][agent]
    p["W3"][:, d:] = 0
    p["b3"][d:] = logstd_b3
    if mean_b3 is not None:
        p["b3"][:d] = mean_b3


def test_rows_at_the_bounds_pass_exactly_the_regulariser():
    """every row of agent 0's actor step saturated (means +-32 +- 13, std 0.14: a =
    (+1.0f, -1.0f) in all 40 rows): dz = da (1 - a a) is exactly 0, so the head
    gradient of each row is flat * 2 reg / (B 2 d) alone, and the b3 gradient its
    sum over the rows -- to the rounding of a 40-term float32 sum"""
    from tests.test_box_squash_gpu import _engine
    c = gs.saturated_case("t2_t2_b40")
    B = c["B"]
    _set_head(c, 0, [32.0, -32.0], -2.0)
    eng = _engine(c, B, 64)
    obs = torch.from_numpy(c["data"][0][0][c["idx"][0]])
    a = eng.act(0, obs, u=torch.from_numpy(c["u_act"][0])).cpu().numpy()
    assert np.array_equal(a, np.tile(F32([1.0, -1.0]), (B, 1)))
    flat = eng.actor_logits(0, obs).cpu().numpy()
    eng.update(0, idx=torch.from_numpy(c["idx"][0]), u_tgt=torch.from_numpy(c["u_tgt"][0]),
               u_act=torch.from_numpy(c["u_act"][0]))
    eng.synchronize()
    got = np.asarray(eng.get_grads(0)["actor"]["b3"], np.float64).ravel()
    scale = F32(2 * 1e-3 / (B * 4))
    terms = (flat * scale).astype(np.float64)
    want = terms.sum(0)
    tol = B * 2.0 ** -24 * np.abs(terms).sum(0) + np.abs(flat).max(0) * float(scale) * 2.0 ** -23 * B
    print(f"GAUSS_EDGES regulariser-only b3 gradient: |got - want| = {np.abs(got - want)}, tolerance {tol}")
    assert got.shape == (4,) and np.all(np.abs(got - want) <= tol), (got, want, tol)
    assert eng.check_finite() == 0


def test_an_infinite_std_is_the_restatements_nan():
    """logstd = 89 on every row of agent 0 (expf: inf).  Decided: as the restatement,
    no clamp (the reference has none).  act(): +-inf on a plain handle and +-1.0f
    squashed where eps != 0, NaN (inf * 0) where eps == 0; the squashed actor step:
    dz = 0 exactly and dlogstd = 0 * inf = NaN, so the clipped step writes NaN and
    mdp_check_finite counts it -- what test_gauss_edges_oracle.py records of the
    restatement (test_what_the_restatement_does_at_an_infinite_std)."""
    from tests.test_box_squash_gpu import _agents, _engine
    c = gs.saturated_case("box2_t2", 1.0)
    B = c["B"]
    for agent in (0, 1):                                   # the plain and the squashed agent
        _set_head(c, agent, None, 89.0)
    eng = _engine(c, B, 64)
    agents = _agents(c)
    for agent, squash in ((0, False), (1, True)):
        obs = c["data"][agent][0][c["idx"][agent]]
        u = c["u_act"][agent]
        a = eng.act(agent, torch.from_numpy(obs), u=torch.from_numpy(u)).cpu().numpy()
        with np.errstate(over="ignore", invalid="ignore"):
            want = bs.act(agents[agent], obs, u, c["spaces"][agent])
        zero = gs.eps_is_zero(u, 2)
        assert zero.any() and np.array_equal(np.isnan(a), zero) and np.array_equal(np.isnan(want), zero)
        assert np.array_equal(a[~zero], want[~zero]) and np.all(np.abs(a[~zero]) == (1.0 if squash else np.inf))
    assert eng.check_finite() == 0
    # the backward alone: no row of the actor step's noise with a zero eps, so the forward is finite
    c["u_act"][1][c["edge_rows"], :2] = (0.5, 0.125)
    eng.update(1, idx=torch.from_numpy(c["idx"][1]), u_tgt=torch.from_numpy(c["u_tgt"][1]),
               u_act=torch.from_numpy(c["u_act"][1]))
    eng.synchronize()
    with np.errstate(over="ignore", invalid="ignore"):
        st, og = bs.update(agents, 1, c["data"], c["idx"][1], c["u_tgt"][1], c["u_act"][1], c["spaces"])
    assert np.isfinite(st[1]) and np.isfinite(eng.stats(1)[1])                  # p_loss: the forward was finite
    dg = eng.get_grads(1)["actor"]
    for k in ("W3", "b3"):                  # dmean = 0 + the regulariser, dlogstd = 0 * inf
        got, ref = np.asarray(dg[k]), np.asarray(og["grad_actor"][k]).reshape(np.asarray(dg[k]).shape)
        assert np.isfinite(got[..., :2]).all() and np.isnan(got[..., 2:]).all(), k
        assert np.array_equal(np.isnan(got), np.isnan(ref)), k
    assert eng.check_finite() > 0


# ---------------------------------------------------- the device's own draws
@pytest.mark.parametrize("squash", [False, True], ids=["plain", "squashed"])
@pytest.mark.parametrize("H", [64, 128])
def test_device_draws_a_zero_radius(H, squash):
    """Engine(seed=ZERO_SEED).act(ZERO_AGENT, obs) without injected uniforms: the first
    draw of stream 0x40000 | agent << 1 has u0 == 0 in row ZERO_ROW (found on the CPU
    with oracle/philox.py, tests/gauss_edges.py), so r = -0 and that row's action is
    the mean exactly, under the largest std; the injected form of the same uniforms
    gives the same bits"""
    from oracle import philox
    R = 16
    u = philox.uniforms5(gs.ZERO_SEED, 0x40000 | (gs.ZERO_AGENT << 1), 0, np.arange(R))
    assert u[gs.ZERO_ROW, 0] == 0
    eng = _act_engine(H, 2, squash, seed=gs.ZERO_SEED)
    head = np.tile(F32([0.5, -4.0, 80.0, 80.0]), (R, 1))
    head[1::2] = F32([-0.5, 4.0, 0.0, -1.0])
    assert head[gs.ZERO_ROW, 2] == 80
    got = eng.act(gs.ZERO_AGENT, _obs(head, False)).cpu().numpy()
    assert not np.isnan(got).any()
    want = head[gs.ZERO_ROW, :2]
    if squash:
        inj0 = eng.act(0, _obs(head, False), u=torch.from_numpy(np.tile(F32([0.0, 0.125]), (R, 1)))).cpu().numpy()
        want = inj0[gs.ZERO_ROW]                             # tanhf(mean) under an injected zero
        assert np.abs(want.astype(np.float64) - np.tanh(head[gs.ZERO_ROW, :2].astype(np.float64))).max() <= BOUND_SQ
    assert np.array_equal(got[gs.ZERO_ROW], want)
    rel, den, ab, tt = gs.errors(got, head, u, 2, squash)
    print(f"GAUSS_EDGES k_mlp_eval own draw H={H} {'squashed' if squash else 'plain'}: rel {rel:.3e} abs {ab:.3e} "
          f"1-a^2 {tt:.3e}")
    assert rel <= BOUND_PLAIN and den == 0 and ab <= BOUND_SQ and tt <= BOUND_T
    inj = eng.act(gs.ZERO_AGENT, _obs(head, False), u=torch.from_numpy(u)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(inj))
