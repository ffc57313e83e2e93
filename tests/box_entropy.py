"""Restatements for entropy-regularised Box policies (mdp_set_act_entropy), on
top of tests/box_squash.py.

Agent i, Box(d), plain or squashed, carries a coefficient ``alphas[i] >= 0``.
Sampling is box_squash's.  For a sample with noise eps, pre-squash value z and
action a, in the operation order of include/maddpg_hip.h (every product and sum
rounded on its own):

    g_k = ((-0.5 * (eps_k * eps_k)) - logstd_k) - 0.5 ln(2 pi)
    squashed:  w = |z_k|;  g_k = g_k - 2 * ((ln 2 - w) - log1p(exp(-2 * w)))
    lp = g_0 (+ g_1)

critic step:  qs = q' - alpha_i * lp'_i  (float), then the fp64 TD line
actor step:   loss += alpha_i * mean_b(lp_b); with ab = alpha_i / B, after the
              regulariser,  plain: dlogstd_k += -ab;  squashed: dmean_k += ab *
              (2 * a_k), dlogstd_k += ab * ((2 * a_k) * se_k - 1)

``alphas[i] == 0`` runs box_squash's own functions: bit for bit today's update.
``dtype`` comes from ``oracle.trainer.F32`` at call time: float32 follows the
device, float64 is the yardstick.
"""
import numpy as np

from oracle import nets, trainer
from tests import box_actions as ba
from tests import box_squash as bs

HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)
LN_2 = np.log(2.0)


def sample_lp(flat, u, d, squash, dtype=None):
    """(a [B, d], std * eps [B, d], lp [B], z [B, d], eps [B, d]) of flat [B, 2 d]"""
    dt = dtype or trainer.F32
    flat = flat.astype(dt)
    eps = ba.box_muller(u, dt)[..., :d]
    z, se = ba.gaussian_sample(flat, u, d, dt)
    a = np.tanh(z).astype(dt) if squash else z
    g = ((dt(-0.5) * (eps * eps).astype(dt)).astype(dt) - flat[:, d:2 * d]).astype(dt)
    g = (g - dt(HALF_LN_2PI)).astype(dt)
    if squash:
        w = np.abs(z)
        c = ((dt(LN_2) - w).astype(dt) - np.log1p(np.exp((dt(-2) * w).astype(dt)).astype(dt)).astype(dt)).astype(dt)
        g = (g - (dt(2) * c).astype(dt)).astype(dt)
    lp = g[:, 0] if d == 1 else (g[:, 0] + g[:, 1]).astype(dt)
    return a, se, lp, z, eps


def entropy_bwd(flat, da, se, a, d, squash, reg_scale, ab, dtype=None):
    """box_squash's backward output + the gradient of alpha * mean(lp); ab = alpha / B"""
    dt = dtype or trainer.F32
    base = bs.squashed_bwd(flat, da, se, a, d, reg_scale, dt) if squash else ba.gaussian_bwd(flat, da, se, d,
                                                                                               reg_scale, dt)
    ab = dt(ab)
    out = base.copy()
    if squash:
        a2 = (dt(2) * a.astype(dt)).astype(dt)
        out[:, :d] = (base[:, :d] + (ab * a2).astype(dt)).astype(dt)
        e = ((a2 * se.astype(dt)).astype(dt) - dt(1)).astype(dt)
        out[:, d:2 * d] = (base[:, d:2 * d] + (ab * e).astype(dt)).astype(dt)
    else:
        out[:, d:2 * d] = (base[:, d:2 * d] + (-ab)).astype(dt)
    return out


def critic_grads(agents, i, batch_n, u_tgt, spaces, alphas, gamma=0.95):
    """box_squash.critic_grads with the soft target of agent i; (grads, stats, mean lp')"""
    if alphas[i] == 0:
        g, st = bs.critic_grads(agents, i, batch_n, u_tgt, spaces, gamma)
        return g, st, 0.0
    F32 = trainer.F32
    n = len(agents)
    ag = agents[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    obs_next_n = [b[3].astype(F32) for b in batch_n]
    rew = np.asarray(batch_n[i][2], np.float64)
    done = np.asarray(batch_n[i][4], np.float64)
    B = len(rew)
    tgt_act_n = [bs.act(agents[j], obs_next_n[j], np.asarray(u_tgt[j]), spaces[j], target=True) for j in range(n)]
    head, _ = nets.mlp_fwd(ag.tgt_actor, obs_next_n[i])
    a_own, _se, lp_t, _z, _e = sample_lp(head, np.asarray(u_tgt[i]), spaces[i][1], bs.is_squashed(spaces[i]))
    assert np.array_equal(a_own, tgt_act_n[i])                     # the sample the launch already draws
    xq_t = trainer.critic_input(obs_next_n, tgt_act_n, i, ag.local_q)
    q_next = nets.mlp_fwd(ag.tgt_critic, xq_t)[0][:, 0]
    qs = (q_next - (F32(alphas[i]) * lp_t).astype(F32)).astype(F32)
    target_q = rew + gamma * (1.0 - done) * qs.astype(np.float64)
    y = target_q.astype(F32)
    xq = trainer.critic_input(obs_n, act_n, i, ag.local_q)
    q, cache = nets.mlp_fwd(ag.critic, xq)
    q = q[:, 0]
    q_loss = np.mean((q.astype(np.float64) - y.astype(np.float64)) ** 2)
    dq = ((F32(2) * (q - y)) * F32(1.0 / B)).astype(F32)[:, None]
    g = nets.mlp_bwd(ag.critic, cache, dq)
    stats = {"q_loss": float(q_loss), "target_q": target_q, "rew": rew, "target_q_next": qs}
    return g, stats, float(np.mean(lp_t.astype(np.float64)))


def actor_grads(agents, i, batch_n, u_act, spaces, alphas, actor_reg=1e-3):
    """box_squash.actor_grads with alpha_i * mean(lp) in the loss; (grads, p_loss, mean lp)"""
    if alphas[i] == 0:
        g, p_loss = bs.actor_grads(agents, i, batch_n, u_act, spaces, actor_reg)
        return g, p_loss, 0.0
    F32 = trainer.F32
    ag, sp = agents[i], spaces[i]
    squash = bs.is_squashed(sp)
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    B = obs_n[0].shape[0]
    head, pcache = nets.mlp_fwd(ag.actor, obs_n[i])
    Hw, w = ba.head_w(sp), ba.act_w(sp)
    a_i, se, lp, _z, _e = sample_lp(head, u_act, w, squash)
    act_in = list(act_n)
    act_in[i] = a_i
    xp = trainer.critic_input(obs_n, act_in, i, ag.local_q)
    qp, qcache = nets.mlp_fwd(ag.critic, xp)
    qp = qp[:, 0]
    p_reg = np.mean(head.astype(np.float64) ** 2)
    mean_lp = float(np.mean(lp.astype(np.float64)))
    p_loss = -np.mean(qp.astype(np.float64) - float(F32(alphas[i])) * lp.astype(np.float64)) + actor_reg * p_reg
    dqp = np.full((B, 1), -1.0 / B, F32)
    dx = nets.input_grad(ag.critic, qcache, dqp)
    if ag.local_q:
        off = obs_n[i].shape[1]
    else:
        off = sum(o.shape[1] for o in obs_n) + sum(a.shape[1] for a in act_n[:i])
    da = dx[:, off:off + w]
    ab = F32(alphas[i]) / F32(B)                                  # the host's float division
    dhead = entropy_bwd(head, da, se, a_i, w, squash, 2 * actor_reg / (B * Hw), ab)
    return nets.mlp_bwd(ag.actor, pcache, dhead), float(p_loss), mean_lp


def update(agents, i, buffers, idx, u_tgt, u_act, spaces, alphas, gamma=0.95, grad_clip=0.5, tau=1e-2,
           actor_reg=1e-3):
    """one strict update of agent i -> (stats, grads, {"lp", "lp_t", "y"})"""
    n = len(agents)
    ag = agents[i]
    batch_n = [tuple(x[idx] for x in buffers[j]) for j in range(n)]
    gq, st, lp_t = critic_grads(agents, i, batch_n, u_tgt, spaces, alphas, gamma)
    trainer.apply_grads(ag.opt_critic, ag.critic, gq, grad_clip)
    gp, p_loss, lp = actor_grads(agents, i, batch_n, u_act, spaces, alphas, actor_reg)
    trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
    nets.polyak(ag.tgt_actor, ag.actor, tau)
    nets.polyak(ag.tgt_critic, ag.critic, tau)
    ent = {"lp": lp, "lp_t": lp_t, "y": np.asarray(st["target_q"], np.float64)}
    return trainer.reference_stats(st, p_loss), {"grad_critic": gq, "grad_actor": gp}, ent
