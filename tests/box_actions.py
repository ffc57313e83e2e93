"""Restatements for Box action spaces: diagonal-Gaussian policies.

The reference sizes an actor with ``make_pdtype(act_space)``
(``distributions.py:408-422``): ``Box(d)`` maps to ``DiagGaussianPdType``.  Its
head is ``flat = [mean (d) | logstd (d)]`` and its sample ``mean + exp(logstd)
* eps`` (``distributions.py:343-371``); ``p_reg = mean(square(flat))``
(``trainer/maddpg.py:46``).  TF's ``random_normal`` was never reproducible: eps
is Box-Muller on the first two of the slot's five uniforms,

    r = sqrt(-2 ln(1 - u0)),  eps_0 = r cos(2 pi u1),  eps_1 = r sin(2 pi u1).

A *space* here is ``("discrete", A)`` or ``("box", d)``.  The action offsets of
the critic input are ``tests/mixed_width.py``'s (``concat(obs_n + act_n)`` with
agent j's action ``w_j`` wide: A_j, or d_j).  Everything takes ``dtype`` from
``oracle.trainer.F32`` at call time, as the other restatements do: float32
follows the device's operation order (every product and sum rounded on its own;
sin / cos of 2 pi u1 reduced exactly, as ``sincospi(2 u1)`` does), float64 is
the other end of the yardstick.
"""
import numpy as np

from oracle import nets, trainer
from tests import mixed_width as mw
from tests.golden.make_golden import make_data

ACT = 5


def is_box(space):
    return space[0] == "box"


def act_w(space):
    """width of the action: A for Discrete(A), d for Box(d)"""
    return space[1]


def head_w(space):
    """width of the actor's head: A logits, or mean | logstd"""
    return 2 * space[1] if is_box(space) else space[1]


def box_muller(u, dtype=None):
    """[..., >= 2] uniforms in [0, 1) -> eps [..., 2]; u[..., 2:] is never read"""
    dt = dtype or trainer.F32
    u0, u1 = np.asarray(u[..., 0]).astype(dt), np.asarray(u[..., 1]).astype(dt)
    r = np.sqrt(dt(-2) * np.log(dt(1) - u0))
    c, s = sincospi2(u1)
    return np.stack([r * c.astype(dt), r * s.astype(dt)], -1).astype(dt)


def sincospi2(u1):
    """(cos, sin) of 2 pi u1 in float64, reduced as sincospi(2 u1) reduces it: x = 2 u1
    (exact) is split into the nearest multiple k / 2 of a quarter turn and a rest in
    [-1/4, 1/4] (exact too), sin and cos are taken of pi * rest and rotated by k.
    u1 in {0, 1/4, 1/2, 3/4} gives exact 0 and +-1, where cos(pi * 0.5) is 6.1e-17."""
    x = 2.0 * np.asarray(u1).astype(np.float64)
    k = np.rint(2.0 * x)
    t = np.pi * (x - 0.5 * k)
    c0, s0 = np.cos(t), np.sin(t)
    q = k.astype(np.int64) & 3
    c = np.choose(q, [c0, -s0, -c0, s0])
    s = np.choose(q, [s0, c0, -s0, -c0])
    return c + 0.0, s + 0.0                          # (-0 + 0 = +0: a quarter turn's zero carries no sign)


def gaussian_sample(flat, u, d, dtype=None):
    """(a [B, d], std * eps [B, d]) of flat [B, 2 d]"""
    dt = dtype or trainer.F32
    flat = flat.astype(dt)
    eps = box_muller(u, dt)[..., :d]
    se = (np.exp(flat[:, d:2 * d]) * eps).astype(dt)
    return (flat[:, :d] + se).astype(dt), se


def gaussian_bwd(flat, da, se, d, reg_scale, dtype=None):
    """dflat = [da | da * std * eps] + flat * reg_scale"""
    dt = dtype or trainer.F32
    flat, da, se = flat.astype(dt), da.astype(dt), se.astype(dt)
    g = np.concatenate([da, (da * se).astype(dt)], 1)
    return (g + (flat * dt(reg_scale)).astype(dt)).astype(dt)


def sample(space, head, u):
    """the policy's sample from its head: u [B, 5] as the device takes it"""
    if is_box(space):
        return gaussian_sample(head, u, space[1])[0]
    return nets.gumbel_softmax(head, u[:, :space[1]])


def act(ag, obs, u, space, target=False):
    head, _ = nets.mlp_fwd(ag.tgt_actor if target else ag.actor, obs)
    return sample(space, head, u)


def target_act(ag, obs, u, space):
    return act(ag, obs, u, space, target=True)


def critic_grads(agents, i, batch_n, u_tgt, spaces, gamma=0.95):
    """trainer.critic_grads with every target actor sampled by its own kind"""
    F32 = trainer.F32
    n = len(agents)
    ag = agents[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    obs_next_n = [b[3].astype(F32) for b in batch_n]
    rew = np.asarray(batch_n[i][2], np.float64)
    done = np.asarray(batch_n[i][4], np.float64)
    B = len(rew)
    tgt_act_n = [target_act(agents[j], obs_next_n[j], np.asarray(u_tgt[j]), spaces[j]) for j in range(n)]
    xq_t = trainer.critic_input(obs_next_n, tgt_act_n, i, ag.local_q)
    target_q_next = nets.mlp_fwd(ag.tgt_critic, xq_t)[0][:, 0]
    target_q = rew + gamma * (1.0 - done) * target_q_next.astype(np.float64)
    y = target_q.astype(F32)
    xq = trainer.critic_input(obs_n, act_n, i, ag.local_q)
    q, cache = nets.mlp_fwd(ag.critic, xq)
    q = q[:, 0]
    q_loss = np.mean((q.astype(np.float64) - y.astype(np.float64)) ** 2)
    dq = ((F32(2) * (q - y)) * F32(1.0 / B)).astype(F32)[:, None]
    g = nets.mlp_bwd(ag.critic, cache, dq)
    stats = {"q_loss": float(q_loss), "target_q": target_q, "rew": rew, "target_q_next": target_q_next}
    return g, stats


def actor_grads(agents, i, batch_n, u_act, spaces, actor_reg=1e-3):
    """mixed_width.actor_grads with agent i's own kind of head"""
    F32 = trainer.F32
    ag, sp = agents[i], spaces[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    B = obs_n[0].shape[0]
    head, pcache = nets.mlp_fwd(ag.actor, obs_n[i])
    Hw, w = head_w(sp), act_w(sp)
    assert head.shape[1] == Hw
    se = None
    if is_box(sp):
        a_i, se = gaussian_sample(head, u_act, w)
    else:
        a_i = nets.gumbel_softmax(head, u_act[:, :w])
    act_in = list(act_n)
    act_in[i] = a_i
    xp = trainer.critic_input(obs_n, act_in, i, ag.local_q)
    qp, qcache = nets.mlp_fwd(ag.critic, xp)
    qp = qp[:, 0]
    p_reg = np.mean(head.astype(np.float64) ** 2)                  # over B * head width entries
    p_loss = -np.mean(qp.astype(np.float64)) + actor_reg * p_reg
    dqp = np.full((B, 1), -1.0 / B, F32)
    dx = nets.input_grad(ag.critic, qcache, dqp)
    if ag.local_q:
        off = obs_n[i].shape[1]
    else:
        off = sum(o.shape[1] for o in obs_n) + sum(a.shape[1] for a in act_n[:i])
    da = dx[:, off:off + w]
    scale = 2 * actor_reg / (B * Hw)
    if is_box(sp):
        dhead = gaussian_bwd(head, da, se, w, scale)
    else:
        dhead = (nets.softmax_bwd(a_i, da) + head * F32(scale)).astype(F32)
    return nets.mlp_bwd(ag.actor, pcache, dhead), float(p_loss)


def update(agents, i, buffers, idx, u_tgt, u_act, spaces, gamma=0.95, grad_clip=0.5, tau=1e-2, actor_reg=1e-3):
    """one strict update of agent i; u_tgt [n, B, 5], u_act [B, 5] as the device takes them"""
    n = len(agents)
    ag = agents[i]
    batch_n = [tuple(x[idx] for x in buffers[j]) for j in range(n)]
    gq, st = critic_grads(agents, i, batch_n, u_tgt, spaces, gamma)
    trainer.apply_grads(ag.opt_critic, ag.critic, gq, grad_clip)
    gp, p_loss = actor_grads(agents, i, batch_n, u_act, spaces, actor_reg)
    trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
    nets.polyak(ag.tgt_actor, ag.actor, tau)
    nets.polyak(ag.tgt_critic, ag.critic, tau)
    return trainer.reference_stats(st, p_loss), {"grad_critic": gq, "grad_actor": gp}


def box_case(dims, spaces, B, L, seed, local_q=None, H=64):
    """mixed_width.mixed_case with kinds: a Discrete agent's stored actions are
    probability vectors, a Box agent's N(0, 1)-scale floats; the nets have the
    reference's shapes (actor out = the head width, critic in counts the action
    widths); idx [n, B], u_tgt [n, n, B, 5], u_act [n, B, 5] (device layout)"""
    rng = np.random.default_rng(seed)
    n, S = len(dims), sum(dims)
    local_q = [False] * n if local_q is None else list(local_q)
    widths = [act_w(s) for s in spaces]
    data = []
    for j, (o, a, r, on, d) in enumerate(make_data(seed + 77, L, dims)):
        if is_box(spaces[j]):
            a = rng.normal(size=(L, widths[j])).astype(np.float32)
        else:
            a = np.asarray(a, np.float32)[:, :widths[j]]
            a = (a / a.sum(1, keepdims=True)).astype(np.float32)
        data.append((o, a, r, on, d))
    params = []
    for i in range(n):
        cin = dims[i] + widths[i] if local_q[i] else S + sum(widths)
        hw = head_w(spaces[i])
        params.append(dict(actor=nets.xavier_init(rng, dims[i], hw, H),
                           critic=nets.xavier_init(rng, cin, 1, H),
                           tgt_actor=nets.xavier_init(rng, dims[i], hw, H),
                           tgt_critic=nets.xavier_init(rng, cin, 1, H)))
        for k in ("actor", "tgt_actor"):     # biases off zero, so that logstd is not centred on 0
            params[-1][k]["b3"] = rng.uniform(-0.5, 0.5, hw).astype(np.float32)
    idx = rng.integers(0, L, size=(n, B)).astype(np.int32)
    top = np.nextafter(np.float32(1), np.float32(0))
    u_tgt = np.minimum(rng.uniform(0.0, 1.0, size=(n, n, B, ACT)).astype(np.float32), top)
    u_act = np.minimum(rng.uniform(0.0, 1.0, size=(n, B, ACT)).astype(np.float32), top)
    # a Discrete agent's Gumbel noise needs u > 0 (log(-log u)); a Box agent takes u0 = 0
    u_tgt, u_act = np.maximum(u_tgt, np.float32(1e-6)), np.maximum(u_act, np.float32(1e-6))
    return dict(data=data, params=params, idx=idx, u_tgt=u_tgt, u_act=u_act, local_q=local_q,
                dims=list(dims), spaces=list(spaces), widths=widths,
                kinds=[s[0] for s in spaces], heads=[head_w(s) for s in spaces])


def to_mpe5(a):
    """(ux, uy) -> the one-hot-style vector [0, ux, 0, uy, 0], which oracle/mpe.py's
    step turns into exactly the force (ux, uy) * sensitivity"""
    a = np.asarray(a)
    out = np.zeros(a.shape[:-1] + (ACT,), a.dtype)
    out[..., 1] = a[..., 0]
    out[..., 3] = a[..., 1]
    return out


def pad_masks(eng, c):
    """boolean mask over one param-space region: True at every pad entry -- head
    columns >= the head width of the actors' W3 / b3, action-slot rows >= the
    action width of the critics' W1"""
    mask = np.zeros(eng.param_floats, bool)
    for i in range(eng.n):
        off, _r, _c, dr, dc = eng.net_tensors(i, 0)[4]          # actor W3 [H][5]
        m = np.zeros((dr, dc), bool)
        m[:, c["heads"][i]:] = True
        mask[off:off + dr * dc] = m.ravel()
        off, _r, _c, dr, dc = eng.net_tensors(i, 0)[5]          # actor b3 [5]
        mask[off + c["heads"][i]:off + dc] = True
        off, _r, _c, dr, dc = eng.net_tensors(i, 1)[0]          # critic W1 [cin][H]
        m = np.zeros((dr, dc), bool)
        m[mw.pad_columns(c["dims"], c["widths"], c["local_q"][i], i), :] = True
        mask[off:off + dr * dc] = m.ravel()
    return mask
