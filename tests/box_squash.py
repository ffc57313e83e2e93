"""Restatements for tanh-squashed Box policies (mdp_set_act_squash), on top of
tests/box_actions.py.

A *space* is box_actions' ``("discrete", A)`` / ``("box", d)`` or, squashed,
``("box", d, "tanh")``: box_actions' ``is_box`` / ``act_w`` / ``head_w`` answer
for the three-entry form what they answer for ``("box", d)``.  The head, its
width, the Box-Muller noise and the regulariser are the plain Box's; only the
last step differs:

    z = mean + exp(logstd) * eps        (box_actions.gaussian_sample, unchanged)
    a = tanh(z)
    dz = da * (1 - a * a);  dmean = dz;  dlogstd = dz * std * eps

with every product and difference rounded on its own in float32, as the device
does.  ``dtype`` comes from ``oracle.trainer.F32`` at call time.
"""
import numpy as np

from oracle import nets, trainer
from tests import box_actions as ba

BOX2T, BOX1T = ("box", 2, "tanh"), ("box", 1, "tanh")


def is_squashed(space):
    return ba.is_box(space) and len(space) > 2 and space[2] == "tanh"


def squashed_sample(flat, u, d, dtype=None):
    """(a [B, d] = tanh(z), std * eps [B, d]) of flat [B, 2 d]"""
    dt = dtype or trainer.F32
    z, se = ba.gaussian_sample(flat, u, d, dt)
    return np.tanh(z).astype(dt), se


def squashed_bwd(flat, da, se, a, d, reg_scale, dtype=None):
    """dflat = [dz | dz * std * eps] + flat * reg_scale, dz = da * (1 - a * a)"""
    dt = dtype or trainer.F32
    a, da = a.astype(dt), da.astype(dt)
    t = (dt(1) - (a * a).astype(dt)).astype(dt)
    return ba.gaussian_bwd(flat, (da * t).astype(dt), se, d, reg_scale, dt)


def sample(space, head, u):
    """the policy's sample from its head: u [B, 5] as the device takes it"""
    if is_squashed(space):
        return squashed_sample(head, u, space[1])[0]
    return ba.sample(space, head, u)


def mode(space, head):
    """what MDP_EVAL_MEAN plays: tanh(mean) / the mean / the noise-free softmax"""
    if is_squashed(space):
        return np.tanh(head[:, :space[1]])
    if ba.is_box(space):
        return head[:, :space[1]]
    z = head - head.max(1, keepdims=True)
    return np.exp(z) / np.exp(z).sum(1, keepdims=True)


def act(ag, obs, u, space, target=False):
    head, _ = nets.mlp_fwd(ag.tgt_actor if target else ag.actor, obs)
    return sample(space, head, u)


def critic_grads(agents, i, batch_n, u_tgt, spaces, gamma=0.95):
    """box_actions.critic_grads with every target actor sampled by its own kind and squash"""
    F32 = trainer.F32
    n = len(agents)
    ag = agents[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    obs_next_n = [b[3].astype(F32) for b in batch_n]
    rew = np.asarray(batch_n[i][2], np.float64)
    done = np.asarray(batch_n[i][4], np.float64)
    B = len(rew)
    tgt_act_n = [act(agents[j], obs_next_n[j], np.asarray(u_tgt[j]), spaces[j], target=True) for j in range(n)]
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
    """box_actions.actor_grads; a squashed agent's own action and backward go through tanh"""
    if not is_squashed(spaces[i]):
        return ba.actor_grads(agents, i, batch_n, u_act, spaces, actor_reg)
    F32 = trainer.F32
    ag, sp = agents[i], spaces[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    B = obs_n[0].shape[0]
    head, pcache = nets.mlp_fwd(ag.actor, obs_n[i])
    Hw, w = ba.head_w(sp), ba.act_w(sp)
    assert head.shape[1] == Hw
    a_i, se = squashed_sample(head, u_act, w)
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
    dhead = squashed_bwd(head, da, se, a_i, w, 2 * actor_reg / (B * Hw))
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


def squash_case(dims, spaces, B, L, seed, local_q=None, H=64):
    """box_actions.box_case; a squashed agent's stored actions are tanh of the
    draw, so that replay holds what the policy can emit.  c["squash"]: per agent
    "tanh" / "none"."""
    c = ba.box_case(dims, [s[:2] for s in spaces], B, L, seed, local_q, H)
    for j, s in enumerate(spaces):
        if is_squashed(s):
            o, a, r, on, d = c["data"][j]
            c["data"][j] = (o, np.tanh(a).astype(np.float32), r, on, d)
    c["spaces"] = list(spaces)
    c["squash"] = ["tanh" if is_squashed(s) else "none" for s in spaces]
    return c
