"""CPU restatement of the device-side prioritized replay (DESIGN.md "Prioritized
replay"; include/maddpg_hip.h, mdp_per_*), written from the semantics, in numpy
fp32 with every operation rounded separately:

* ``build(leaves, P)``         the {sum, min} tree as a pure function of its leaves
* ``sample(tree, B, u)``       the stratified descent -> ring positions
* ``weights(tree, idx, beta)`` importance-sampling weights
* ``priority_from_error``      min(|err| + eps, upper) ** alpha
* ``beta_after(k)``            beta after k sample calls (fp32 accumulation)
* ``device_uniforms``          the device Philox draw of one sample call
* ``critic_grads`` / ``update_batch``  ``oracle.trainer``'s critic step with the
  per-row weight at the loss and at its seed
"""
import numpy as np

from oracle import nets, philox, trainer

F32 = np.float32
ALPHA, BETA0, BETA_INC, EPS, UPPER = F32(0.6), F32(0.4), F32(0.001), F32(0.01), F32(1.0)
STREAM = 0x50000   # MDP_PER_STREAM | agent


def tree_leaves(capacity):
    P = 1
    while P < capacity:
        P *= 2
    return P


def empty_leaves(P):
    lv = np.zeros((P, 2), F32)
    lv[:, 1] = np.inf
    return lv


def build(prio, P, filled=None):
    """tree [2 P, 2] {sum, min}: leaf i = {prio[i], prio[i]} where filled (default:
    every given priority) and positive, {0, +inf} elsewhere; node 0 unused and zero"""
    prio = np.asarray(prio, F32)
    filled = np.ones(len(prio), bool) if filled is None else np.asarray(filled, bool)
    t = np.zeros((2 * P, 2), F32)
    t[P:] = empty_leaves(P)
    k = len(prio)
    t[P:P + k, 0] = np.where(filled, prio, F32(0))
    t[P:P + k, 1] = np.where(filled & (prio > 0), prio, F32(np.inf))   # a zero priority: like an unfilled leaf
    w = P // 2
    while w >= 1:
        l, r = t[2 * w:4 * w:2], t[2 * w + 1:4 * w:2]
        t[w:2 * w, 0] = (l[:, 0] + r[:, 0]).astype(F32)
        t[w:2 * w, 1] = np.minimum(l[:, 1], r[:, 1])
        w //= 2
    return t


def sample(tree, B, u):
    """ring positions of the stratified draw: seg = total / B, v_i = (i + u_i) seg;
    right (v -= left.sum) iff v >= left.sum and right.sum > 0"""
    P = len(tree) // 2
    u = np.asarray(u, F32)
    total = tree[1, 0]
    seg = F32(total / F32(B))
    out = np.empty(B, np.int32)
    for i in range(B):
        v = F32(F32(F32(i) + u[i]) * seg)
        node = 1
        while node < P:
            ls, rs = tree[2 * node, 0], tree[2 * node + 1, 0]
            if v >= ls and rs > 0:
                v = F32(v - ls)
                node = 2 * node + 1
            else:
                node = 2 * node
        out[i] = node - P
    return out


def beta_after(k, beta0=BETA0, inc=BETA_INC):
    b = F32(beta0)
    for _ in range(k):
        b = min(F32(1.0), F32(b + F32(inc)))
    return F32(b)


def weights(tree, idx, beta):
    """w_i = (p_i / p_min) ** -beta with p_min = root.min (filled leaves only)"""
    P = len(tree) // 2
    p = tree[P + np.asarray(idx, np.int64), 0]
    return np.power((p / tree[1, 1]).astype(F32), -F32(beta)).astype(F32)


def priority_from_error(abs_err, alpha=ALPHA, eps=EPS, upper=UPPER):
    e = (np.asarray(abs_err, F32) + F32(eps)).astype(F32)
    return np.power(np.minimum(e, F32(upper)), F32(alpha)).astype(F32)


def device_uniforms(seed, agent, sample_count, B):
    """u_i of a sample call without injected noise: word 0 of philox4x32_10 at
    counter (i, samples drawn so far by this agent, 0x50000 | agent, 0), key =
    the engine seed, through u01"""
    rows = np.arange(B, dtype=np.uint64)
    c = np.stack([rows, np.full_like(rows, sample_count), np.full_like(rows, STREAM | agent),
                  np.zeros_like(rows)], -1)
    key = np.array([seed & philox.MASK, (seed >> 32) & philox.MASK], np.uint64)
    return philox.u01(philox.philox4x32_10(c, key)[:, 0])


def critic_grads(agents, i, batch_n, u_tgt, w, gamma=0.95):
    """``oracle.trainer.critic_grads`` with the loss mean_b(w_b (q_b - y_b)^2): seed
    dL/dq_b = 2 w_b (q_b - y_b) / B.  Also returns |q - y|."""
    n = len(agents)
    ag = agents[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    obs_next_n = [b[3].astype(F32) for b in batch_n]
    rew = np.asarray(batch_n[i][2], np.float64)
    done = np.asarray(batch_n[i][4], np.float64)
    B = len(rew)
    w = np.asarray(w, F32)
    tgt_act_n = [trainer.target_act(agents[j], obs_next_n[j], u_tgt[j]) for j in range(n)]
    xq_t = trainer.critic_input(obs_next_n, tgt_act_n, i, ag.local_q)
    target_q_next = nets.mlp_fwd(ag.tgt_critic, xq_t)[0][:, 0]
    target_q = rew + gamma * (1.0 - done) * target_q_next.astype(np.float64)
    y = target_q.astype(F32)
    xq = trainer.critic_input(obs_n, act_n, i, ag.local_q)
    q, cache = nets.mlp_fwd(ag.critic, xq)
    q = q[:, 0]
    d64 = q.astype(np.float64) - y.astype(np.float64)
    q_loss = np.mean(w.astype(np.float64) * d64 ** 2)
    dq = (((F32(2) * (q - y)) * w) * F32(1.0 / B)).astype(F32)[:, None]
    g = nets.mlp_bwd(ag.critic, cache, dq)
    stats = {"q_loss": float(q_loss), "target_q": target_q, "rew": rew, "target_q_next": target_q_next,
             "td": np.abs(q - y).astype(F32), "q": q, "y": y}
    return g, stats


def update_batch(agents, i, batch_n, u_tgt, u_act, w, gamma=0.95, grad_clip=0.5, tau=1e-2, actor_reg=1e-3):
    """``oracle.trainer.update_batch`` with the weighted critic step (the actor step is unweighted)"""
    ag = agents[i]
    gq, st = critic_grads(agents, i, batch_n, u_tgt, w, gamma)
    trainer.apply_grads(ag.opt_critic, ag.critic, gq, grad_clip)
    gp, p_loss = trainer.actor_grads(agents, i, batch_n, u_act, actor_reg)
    trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
    nets.polyak(ag.tgt_actor, ag.actor, tau)
    nets.polyak(ag.tgt_critic, ag.critic, tau)
    return trainer.reference_stats(st, p_loss), {"grad_critic": gq, "grad_actor": gp}, st
