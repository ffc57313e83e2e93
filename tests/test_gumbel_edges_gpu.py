"""GPU: the Gumbel-softmax sample (gumbel_noise5 / gumbel_softmax5_pre /
gumbel_softmax_pre, mdp_device.h) on the ends of its inputs, at every kernel it
is inlined into, against the float64 reference of tests/gumbel_edges.py.

Inputs: the grid of tests/gumbel_edges.py (uniforms 0, 2^-23, 2^-12, 0.25, 0.5,
1 - 2^-12, 1 - 2^-23 against logits -80 .. 80), handed to the kernels through
an actor whose logits are 128 * obs[k] bit for bit (exact_logit_actor).

On every site: all outputs finite; an entry whose uniform is 0 is exactly 0.0f;
pad entries exactly 0.0f; width 1 exactly 1.0f; each row sums to 1 within 4 ulp;
the error against the reference at most 4 x e32 in the absolute and in the
relative form (relative over entries with reference probability > 1e-30), e32
being the error of the numpy fp32 restatement on the same grid (E32_ABS =
1.08e-7, E32_REL = 5.51e-6: bounds 4.32e-7 and 2.20e-5).  The factor 4: the
hardware log / exp / rcp are specified to about 1 ulp each where libm is below
1, and three of them are chained with the z - max subtraction.  The same
(logits, u) row must give the same bits at every site and row position.

Observed on MI355X (worst over the site's rows; abs / rel / row sum in ulp):
  k_mlp_eval A=5, H = 64 / 128 / 256, both nets      1.08e-7 / 5.30e-6 / 0.78
  k_mlp_eval A=3                                     7.0e-8  / 5.30e-6 / 0.60
  k_mlp_eval A=1                                     0 / 0 / 0
  k_rollout wave per agent (spread N=3, H=64)        5.3e-8  / 3.1e-6  / 0.44
  k_rollout mlp_fwd_tile_pf (tag N=6, H=64)          6.6e-8  / 4.0e-6  / 0.55
  k_rollout mlp_fwd_tile (spread, tag N=6, H=128)    6.6e-8  / 4.0e-6  / 0.55
  k_rollout speaker-listener, listener A=5           3.3e-8  / 2.8e-6  / 0.28
  k_rollout speaker-listener, speaker A=3            3.38e-7 / 8.7e-6  / 0.25
  k_mlp_eval, the device's own draw of a 0           6.1e-8  / 2.6e-6  / 0.58
(the speaker's logits, 128 x its colour observation = 83.2 / 19.2, lie off the
grid: the numpy fp32 restatement's own error on those rows is 3.7e-7 / 7.6e-6.)
The same bits at every site, row position, row count and H.
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
from tests import gumbel_edges as ge  # noqa: E402
from tests.helpers import row_layout  # noqa: E402

ACT = 5
OBS = 18
ABS_BOUND, REL_BOUND = 4 * ge.E32_ABS, 4 * ge.E32_REL
# the target actor reads its logits from other observation entries than the actor
TGT_DRIVE = [OBS - 1 - k for k in range(ACT)]


def _check(site, got, lg, u, width):
    """the assertions every site must meet; got [R, 5] (pad entries included) or [R, width]"""
    got = np.asarray(got)
    live, ref = got[:, :width], ge.reference(lg, u)
    a, r = ge.errors(live, ref) if np.isfinite(live).all() else (np.inf, np.inf)
    ulp = float(ge.ulp_sum_error(live).max())
    print(f"GUMBEL_EDGES {site}: abs {a:.3e} rel {r:.3e} row sum {ulp:.2f} ulp ({len(lg)} rows)")
    assert got.dtype == np.float32 and np.isfinite(got).all(), site
    assert np.all(live[u == 0] == 0), site
    assert np.all(got[:, width:] == 0), site
    if width == 1:
        assert np.all(live == 1.0), site
    assert ulp <= 4, (site, ulp)
    assert a <= ABS_BOUND, (site, a, ABS_BOUND)
    assert r <= REL_BOUND, (site, r, REL_BOUND)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _act_engine(H, width):
    eng = Engine([OBS], num_units=H, batch_size=16, capacity=64, act_dims=[width])
    eng.init_params(0)
    eng.set_params(0, "actor", ge.exact_logit_actor(OBS, H, width))
    eng.set_params(0, "tgt_actor", ge.exact_logit_actor(OBS, H, width, drive=TGT_DRIVE[:width]))
    return eng


def _obs(lg, target):
    return torch.from_numpy(ge.obs_for(lg, OBS, drive=TGT_DRIVE[:lg.shape[1]] if target else None))


def _act_chunks(eng, lg, u, R, target):
    """act() on the whole set in calls of exactly R rows (the last one wraps round): [len, width]"""
    N = len(lg)
    out = np.full(lg.shape, np.nan, np.float32)
    for start in range(0, N, R):
        rows = (start + np.arange(R)) % N
        got = eng.act(0, _obs(lg[rows], target), target=target, u=torch.from_numpy(u[rows])).cpu().numpy()
        assert got.shape == (R, lg.shape[1])
        fresh = rows[:min(R, N - start)]
        out[fresh] = got[:len(fresh)]
        # a row seen before (the wrap) has the bits it had at its first position
        again = rows[len(fresh):]
        assert np.array_equal(_bits(got[len(fresh):]), _bits(out[again]))
    return out


@functools.lru_cache(maxsize=None)
def _canonical(width):
    """the grid through act() at H = 64 in 40-row calls: what every other site must reproduce"""
    lg, u = ge.grid(width)
    return _act_chunks(_act_engine(64, width), lg, u, 40, False)


@pytest.mark.parametrize("width", [5, 3, 1])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_actor_logits_are_the_table_bit_for_bit(H, width):
    """the construction on the device (k_mlp_eval, current and target nets), before anything is judged"""
    lg, _ = ge.grid(width)
    eng = _act_engine(H, width)
    for target in (False, True):
        for start in range(0, len(lg), 40):
            rows = (start + np.arange(40)) % len(lg)
            got = eng.actor_logits(0, _obs(lg[rows], target), target=target).cpu().numpy()
            assert got.shape == (40, width) and np.array_equal(got, lg[rows]), (H, width, target)
            nz = lg[rows] != 0
            assert np.array_equal(_bits(got)[nz], _bits(lg[rows])[nz])


@pytest.mark.parametrize("width", [5, 3, 1])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_act_on_the_edge_grid(H, width):
    """k_mlp_eval through Engine.act: row counts 1 (the facade's action()), 16, 17
    and 40 (ragged against the 16-row tile), current and target nets"""
    lg, u = ge.grid(width)
    eng = _act_engine(H, width)
    first = None
    for R in (40, 17, 16, 1):
        for target in (False, True):
            got = _act_chunks(eng, lg, u, R, target)
            if first is None:
                first = got
                _check(f"k_mlp_eval H={H} A={width}", got, lg, u, width)
            assert np.array_equal(_bits(got), _bits(first)), (H, width, R, target)
    assert np.array_equal(_bits(first), _bits(_canonical(width))), "H = 64 and this H differ in bits"
    if width < ACT:
        # the raw 5-wide slot: pad entries exactly 0 whatever the pad uniforms hold
        u5 = np.full((len(lg), ACT), np.nan, np.float32)
        u5[:, :width] = u
        out = torch.empty((40, ACT), dtype=torch.float32, device=eng.device)
        obs = _obs(lg[:40], False).to(eng.device).contiguous()
        ud = torch.from_numpy(u5[:40]).to(eng.device).contiguous()
        eng.sync_in()
        eng._c("mdp_act", 0, 0, eng._ptr(obs), eng._ptr(out), 40, eng._ptr(ud))
        eng.sync_out()
        raw = out.cpu().numpy()
        _check(f"k_mlp_eval raw slot H={H} A={width}", raw, lg[:40], u[:40], width)
        assert np.array_equal(_bits(raw[:, :width]), _bits(first[:40]))


# ---------------------------------------------------------------- k_rollout
DRIVE = [0, 1, 2, 3, None]       # own velocity (obs 0, 1) and position (obs 2, 3); the fifth logit is 0


def _rollout_engine(name, n, na, H, E):
    sp = spec(name, n, na if na else None)
    eng = Engine(sp.obs_dims, num_units=H, batch_size=16, capacity=64, num_envs=E, scenario=name,
                 num_adversaries=sp.num_adversaries, max_episode_len=25, seed=3)
    eng.init_params(0)
    for j, o in enumerate(sp.obs_dims):
        eng.set_params(j, "actor", ge.exact_logit_actor(o, H, ACT, drive=DRIVE))
    eng.env_reset()
    return eng, sp


@pytest.mark.parametrize("name,n,na,H,path", [
    ("simple_spread", 3, 0, 64, "wave per agent"),
    ("simple_tag", 6, 4, 64, "mlp_fwd_tile_pf"),
    ("simple_spread", 3, 0, 128, "mlp_fwd_tile"),
    ("simple_tag", 6, 4, 128, "mlp_fwd_tile"),
])
def test_rollout_on_the_edge_grid(name, n, na, H, path):
    """k_rollout's policy forward through Engine.env_step(u=...) after set_env_state,
    E = 17: the logits driven by each agent's own velocity and position
    observation entries (exact copies of the state set), the stored actions read
    from the replay rows"""
    E = 17
    eng, sp = _rollout_engine(name, n, na, H, E)
    st = eng.env_state()
    pos, vel = st["pos"].copy(), st["vel"].copy()
    tab = [ge.rollout_rows(E, j) for j in range(n)]
    for j in range(n):
        vel[:, j] = tab[j][0][:, 0:2] / np.float32(ge.S)
        pos[:, j] = tab[j][0][:, 2:4] / np.float32(ge.S)
    for l in range(pos.shape[1] - n):                     # landmarks: apart from every agent
        pos[:, n + l] = (0.9, -0.9 + 0.2 * l)
    d = pos[:, :, None] - pos[:, None]
    assert np.all(np.abs(d).max(-1)[:, ~np.eye(pos.shape[1], dtype=bool)] > 0)
    eng.set_env_state(pos, vel, st["goal"], st["ep_step"])
    u = np.stack([t[1] for t in tab], 1)                  # [E, n, 5]
    eng.env_step(u=torch.from_numpy(u))
    rows = eng.replay_rows(0, E).cpu().numpy()
    lay, _ = row_layout(sp.obs_dims)
    canon = _act_engine(64, ACT)
    for j in range(n):
        lg, uj = tab[j]
        lj, o = lay[j], sp.obs_dims[j]
        obs = rows[:, lj["obs"]:lj["obs"] + o]
        assert np.array_equal(obs[:, :4] * np.float32(ge.S), lg[:, :4]), "the driven observation entries"
        assert np.array_equal(eng.actor_logits(j, torch.from_numpy(obs)).cpu().numpy(), lg)
        got = rows[:, lj["act"]:lj["act"] + ACT]
        _check(f"k_rollout {path} {name} n={n} H={H} agent {j}", got, lg, uj, ACT)
        # the same rows through act(): on this handle, and on the plain H = 64 one at other row positions
        same = eng.act(j, torch.from_numpy(obs), u=torch.from_numpy(uj)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(same)), (path, j)
        back = np.arange(E)[::-1].copy()
        other = canon.act(0, torch.from_numpy(ge.obs_for(lg[back], OBS)), u=torch.from_numpy(uj[back])).cpu().numpy()
        assert np.array_equal(_bits(got[back]), _bits(other)), (path, j)
    assert np.isfinite(rows).all() and eng.buffer_len() == E


@pytest.mark.parametrize("H", [64, 128])
def test_rollout_speaker_listener_on_edge_noise(H):
    """one simple_speaker_listener step (act_dims [3, 5]): the narrow form inside
    the rollout.  The speaker's logits are 128 x its goal-colour observation
    (83.2 / 19.2: saturated), the listener's are driven by its velocity and by
    the standing message."""
    E, name = 17, "simple_speaker_listener"
    sp = spec(name)
    eng = Engine(sp.obs_dims, num_units=H, batch_size=16, capacity=64, num_envs=E, scenario=name, seed=3)
    assert eng.act_dims == [3, 5]
    eng.init_params(0)
    ldrive = [0, 1, 8, 9, None]                            # listener obs: vel (2), landmarks (6), message (3)
    eng.set_params(0, "actor", ge.exact_logit_actor(3, H, 3))
    eng.set_params(1, "actor", ge.exact_logit_actor(11, H, ACT, drive=ldrive))
    eng.env_reset()
    st = eng.env_state()
    lg1, u1 = ge.rollout_rows(E, 1)
    _, u0 = ge.rollout_rows(E, 0, width=3, driven=0)
    vel, comm = st["vel"].copy(), np.zeros((E, 2, ACT), np.float32)
    vel[:, 1] = lg1[:, 0:2] / np.float32(ge.S)
    comm[:, 0, 0:2] = lg1[:, 2:4] / np.float32(ge.S)
    eng.set_env_state(st["pos"], vel, st["goal"], st["ep_step"], comm=comm)
    u = np.full((E, 2, ACT), np.nan, np.float32)           # the speaker's pad uniforms are never used
    u[:, 0, :3], u[:, 1] = u0, u1
    eng.env_step(u=torch.from_numpy(u))
    rows = eng.replay_rows(0, E).cpu().numpy()
    lay, _ = row_layout(sp.obs_dims)
    obs0 = rows[:, lay[0]["obs"]:lay[0]["obs"] + 3]
    lg0 = obs0 * np.float32(ge.S)
    assert set(np.unique(obs0)) == {np.float32(0.15), np.float32(0.65)}
    assert np.array_equal(eng.actor_logits(0, torch.from_numpy(obs0)).cpu().numpy(), lg0)
    got0 = rows[:, lay[0]["act"]:lay[0]["act"] + ACT]
    _check(f"k_rollout speaker A=3 H={H}", got0, lg0, u0, 3)
    same = eng.act(0, torch.from_numpy(obs0), u=torch.from_numpy(u0)).cpu().numpy()
    assert np.array_equal(_bits(got0[:, :3]), _bits(same))
    obs1 = rows[:, lay[1]["obs"]:lay[1]["obs"] + 11]
    assert np.array_equal(obs1[:, ldrive[:4]] * np.float32(ge.S), lg1[:, :4])
    assert np.array_equal(eng.actor_logits(1, torch.from_numpy(obs1)).cpu().numpy(), lg1)
    got1 = rows[:, lay[1]["act"]:lay[1]["act"] + ACT]
    _check(f"k_rollout listener A=5 H={H}", got1, lg1, u1, ACT)
    back = np.arange(E)[::-1].copy()
    other = _act_engine(64, ACT).act(0, torch.from_numpy(ge.obs_for(lg1[back], OBS)),
                                     u=torch.from_numpy(u1[back])).cpu().numpy()
    assert np.array_equal(_bits(got1[back]), _bits(other))
    # the message the listener hears next is the stored speaker action
    assert np.array_equal(rows[:, lay[1]["nobs"] + 8:lay[1]["nobs"] + 11], got0[:, :3])
    assert np.isfinite(rows).all()


# ------------------------------------------------- backward and the optimizer
def _all_finite(eng):
    """after the step: no NaN / Inf in any parameter, Adam slot, gradient or stat"""
    eng.synchronize()
    assert eng.check_finite() == 0
    for name in ("theta", "target", "adam_m", "adam_v", "grad"):
        assert np.isfinite(eng.region(name).cpu().numpy()[:eng.param_floats]).all(), name
    for i in range(eng.n):
        assert np.all(np.isfinite(eng.stats(i))), i


@pytest.mark.parametrize("path", ["register", "general"])
def test_update_saturated_policies_with_edge_noise(monkeypatch, path):
    """one strict round on actors scaled by S_UPDATE = 16 (|logit| up to 19.5, samples
    at probability 1.0f beside unsaturated rows) with the edge uniforms in five
    batch rows per noise array (a 0 and a 1 - 2^-23 for every agent), at
    _update_parity's own bounds: gradients 1e-5 of the tensor's largest entry,
    conditioned weights 1e-6, all weights 2e-4, loss 1e-5, stats, beta powers.
    The oracle alone sits within a quarter of the gradient bound of its fp64
    self on this case (tests/test_gumbel_edges_oracle.py).
    Observed on MI355X (gradient / conditioned weight / any weight): register
    kernels 1.0e-6 / 4.8e-7 / 9.4e-6, general 6.1e-7 / 2.4e-7 / 7.2e-6; the
    NARROW case below 6.3e-7 / - / 8.6e-7; the tag N=6 throughput round
    6.9e-7 / 3.6e-7 / 2.6e-5."""
    from tests.test_gpu_parity import _update_parity
    dims, B, L = [18, 18, 18], 40, 300
    if path == "general":
        monkeypatch.setenv("MDP_GENERAL_GRADS", "1")
    probe = Engine(dims, batch_size=B, capacity=B)
    assert [probe.lib.mdp_grad_variant(probe.h, i) for i in range(3)] == [0 if path == "general" else 1] * 3
    probe.close()
    c = ge.saturated_case(dims, B, L, ge.SEED_UPDATE, ge.S_UPDATE)
    _update_parity(dims, B=B, L=L, seed=ge.SEED_UPDATE, case=c, after=_all_finite)


def test_update_saturated_narrow_widths_with_edge_noise():
    """the same on dims [3, 11] with act_dims [3, 5]: the register kernels' NARROW
    instantiation, against tests/mixed_width.py at test_act_dims_gpu's bounds"""
    from tests.test_act_dims_gpu import _strict_round
    dims, widths, B, L = [3, 11], [3, 5], 40, 300
    c = ge.saturated_case(dims, B, L, ge.SEED_UPDATE + 1, ge.S_UPDATE, widths=widths)
    eng = _strict_round(c, B, L, variant=1)
    _all_finite(eng)


def test_throughput_round_saturated_tag6_h128_with_edge_noise(monkeypatch):
    """one throughput-mode round on tag N=6 at H = 128 (k_grad_pair: the general
    kernels' critic and actor steps in one launch), saturated actors and edge
    noise, at _throughput_round_parity's own bounds"""
    from tests.test_gpu_parity import _throughput_round_parity
    dims, B, L = [22, 22, 22, 22, 20, 20], 40, 300
    c = ge.saturated_case(dims, B, L, 61, ge.S_UPDATE, H=128)
    _throughput_round_parity(monkeypatch, dims, None, B, 128, False, L=L, case=c, after=_all_finite)


# ------------------------------------------------ the device's own draw of a 0
@pytest.mark.parametrize("H", [64, 128])
def test_device_draws_a_zero(H):
    """Engine(seed=ZERO_SEED).act(ZERO_AGENT, obs) without injected uniforms: the
    first draw of stream 0x40000 | agent << 1 has a word whose top 23 bits are
    zero at (ZERO_ROW, ZERO_ENTRY), found on the CPU with oracle/philox.py
        for seed in range(2 ** 27 // 80):
            u = philox.uniforms5(seed, 0x40000, 0, np.arange(16))
            if (u == 0).any(): print(seed, np.argwhere(u == 0)); break
    -> 295278 [[15, 4]].  u01 makes it an exact 0.0f, the sample must hold an
    exact 0.0f there and no NaN, and match the reference everywhere (the other
    uniforms are ordinary draws: the yardstick's bounds hold a fortiori)."""
    from oracle import philox
    R = 16
    u = philox.uniforms5(ge.ZERO_SEED, 0x40000 | (ge.ZERO_AGENT << 1), 0, np.arange(R))
    assert u[ge.ZERO_ROW, ge.ZERO_ENTRY] == 0
    eng = Engine([OBS], num_units=H, batch_size=16, capacity=64, seed=ge.ZERO_SEED)
    eng.init_params(0)
    eng.set_params(0, "actor", ge.exact_logit_actor(OBS, H, ACT))
    lg = np.tile(ge.LOGITS[[5, 4, 3, 2, 6]], (R, 1))       # 4, 0.5, 0, -4, 30: the zero lands on the largest logit
    lg[::2] = ge.LOGITS[[3, 4, 5, 2, 4]]                   # and rows with no saturated entry
    assert lg[ge.ZERO_ROW, ge.ZERO_ENTRY] == 30
    got = eng.act(ge.ZERO_AGENT, torch.from_numpy(ge.obs_for(lg, OBS))).cpu().numpy()
    assert got[ge.ZERO_ROW, ge.ZERO_ENTRY] == 0.0 and not np.isnan(got).any()
    _check(f"k_mlp_eval own draw H={H}", got, lg, u, ACT)
    # the injected form of the same uniforms gives the same bits
    inj = eng.act(ge.ZERO_AGENT, torch.from_numpy(ge.obs_for(lg, OBS)), u=torch.from_numpy(u)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(inj))
