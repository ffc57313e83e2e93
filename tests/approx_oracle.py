"""MADDPG with inferred policies (Lowe et al. 2017, section 4.2), restated in numpy on
top of oracle.trainer (test oracle of mdp_approx_enable).

Every agent i with a MADDPG critic keeps, for every other agent j, an
approximator phi_i^j of agent j's actor shape with its own target network and
Adam optimizer.  Agent i's update on its minibatch:

1. the critic step of oracle.trainer, with the target action of every j != i
   drawn from the TARGET approximator of (i, j) on o'_j (same noise u_tgt[j]);
   agent i's own target action still comes from its target actor;
2. the actor step, then Polyak of actor and critic, unchanged;
3. for every j != i one step of phi_i^j on the same rows:
     p = softmax(l), l the logits of phi_i^j(o_j); a = agent j's replayed action
     loss = mean_b[ -sum_c a_c log p_c - lambda H(p) ],  H(p) = -sum_c p_c log p_c
     log p_c = (l_c - max) - log sum exp(l - max)      (never the log of a probability)
     dL/dl_c = [ p_c sum_c' a_c' - a_c + lambda p_c (log p_c + H) ] / B
   raw gradients, per-tensor clip_by_norm, Adam, then target <- Polyak(target, phi).

All shapes are the reference's (logical) ones: agent j's actions and logits
are A_j wide.  The per-row arithmetic is fp32 in the device's operation order;
the cross-entropy, entropy and loss are float64 means of the fp32 row values.
"""
import numpy as np

from oracle import nets, trainer
from tests import mixed_width

F32 = np.float32
LAMBDA = 1e-3


class Approx:
    def __init__(self, net, tgt, lr=1e-2):
        self.net, self.tgt = net, tgt
        self.opt = nets.Adam(net, lr=lr)


def add_approx(agents, approx, lr=1e-2):
    """approx[i][j] = dict(net=, tgt=) for every MADDPG-critic agent i and j != i"""
    for i, ag in enumerate(agents):
        ag.approx = {}
        if ag.local_q:
            continue
        for j in range(len(agents)):
            if j != i:
                ag.approx[j] = Approx(approx[i][j]["net"], approx[i][j]["tgt"], lr)
    return agents


def head(logits, a, lam, B):
    """(per-row cross-entropy, per-row entropy, dL/dlogits) in fp32"""
    l = logits.astype(F32)
    a = a.astype(F32)
    z = l - l.max(1, keepdims=True)
    e = np.exp(z)
    se = e.sum(1, keepdims=True, dtype=F32)
    lp = (z - np.log(se)).astype(F32)
    p = (e / se).astype(F32)
    sa = a.sum(1, keepdims=True, dtype=F32)
    ce = -(a * lp).sum(1, dtype=F32)
    en = -(p * lp).sum(1, dtype=F32)
    seed = (((p * sa - a) + F32(lam) * (p * (lp + en[:, None]))) * F32(1.0 / B)).astype(F32)
    return ce, en, seed


def approx_grads(phi, obs, act, lam=LAMBDA):
    """raw gradients of one approximator's loss on the rows (obs, act), and its stats"""
    logits, cache = nets.mlp_fwd(phi, obs.astype(F32))
    ce, en, seed = head(logits, act, lam, len(obs))
    ce64, en64 = float(np.mean(ce.astype(np.float64))), float(np.mean(en.astype(np.float64)))
    return nets.mlp_bwd(phi, cache, seed), dict(cross_entropy=ce64, entropy=en64, loss=ce64 - float(F32(lam)) * en64)


def approx_step(ap, obs, act, lam=LAMBDA, grad_clip=0.5, tau=1e-2):
    g, st = approx_grads(ap.net, obs, act, lam)
    trainer.apply_grads(ap.opt, ap.net, g, grad_clip)
    nets.polyak(ap.tgt, ap.net, tau)
    return g, st


def approx_steps(agents, i, batch_n, lam=LAMBDA, grad_clip=0.5, tau=1e-2):
    """step 3 for every pair of observer i; {j: (raw gradients, stats)}"""
    return {j: approx_step(ap, batch_n[j][0], batch_n[j][1], lam, grad_clip, tau)
            for j, ap in sorted(agents[i].approx.items())}


class _TargetView:
    def __init__(self, tgt_actor):
        self.tgt_actor = tgt_actor


def critic_grads(agents, i, batch_n, u_tgt, gamma=0.95):
    """trainer.critic_grads with the others' target actions from agent i's target approximators"""
    ag = agents[i]
    view = [agents[j] if (j == i or j not in ag.approx) else _TargetView(ag.approx[j].tgt) for j in range(len(agents))]
    return trainer.critic_grads(view, i, batch_n, u_tgt, gamma)


def update(agents, i, buffers, idx, u_tgt, u_act, widths, lam=LAMBDA, gamma=0.95, grad_clip=0.5, tau=1e-2,
           actor_reg=1e-3):
    """agent i's update; u_tgt [n, B, 5], u_act [B, 5] as the device takes them.
    Returns (the six stats, extras with the raw gradients and the pairs' stats)."""
    n = len(agents)
    ag = agents[i]
    batch_n = [tuple(x[idx] for x in buffers[j]) for j in range(n)]
    gq, st = critic_grads(agents, i, batch_n, mixed_width.narrow(u_tgt, widths), gamma)
    trainer.apply_grads(ag.opt_critic, ag.critic, gq, grad_clip)
    gp, p_loss = mixed_width.actor_grads(agents, i, batch_n, u_act, actor_reg)
    trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
    nets.polyak(ag.tgt_actor, ag.actor, tau)
    nets.polyak(ag.tgt_critic, ag.critic, tau)
    pairs = approx_steps(agents, i, batch_n, lam, grad_clip, tau)
    return trainer.reference_stats(st, p_loss), {"grad_critic": gq, "grad_actor": gp, "approx": pairs}


def approx_case(c, dims, seed, H=64):
    """independently drawn approximators and targets for a trainer case: [i][j] -> dict(net, tgt)"""
    rng = np.random.default_rng(seed + 4242)
    n = len(dims)
    widths = c.get("widths", [5] * n)
    return [{j: dict(net=nets.xavier_init(rng, dims[j], widths[j], H), tgt=nets.xavier_init(rng, dims[j], widths[j], H))
             for j in range(n) if j != i} for i in range(n)]


# ---- the frozen-policy fit: replayed actions are Gumbel-softmax samples of fixed,
# far-from-uniform policies (xavier weights x 3); an approximator trained on them
# must move towards the policy that produced them
FIT_DIMS, FIT_L, FIT_B, FIT_STEPS, FIT_H = [6, 5, 4], 4000, 64, 100, 64


def fit_case(seed=5):
    rng = np.random.default_rng(seed)
    n = len(FIT_DIMS)
    actors = []
    for j in range(n):
        p = nets.xavier_init(rng, FIT_DIMS[j], 5, FIT_H)
        actors.append({k: (v * F32(3)).astype(F32) for k, v in p.items()})
    top = np.nextafter(F32(1), F32(0))
    data = []
    for j in range(n):
        obs = rng.normal(size=(FIT_L, FIT_DIMS[j])).astype(F32)
        u = np.minimum(rng.uniform(1e-6, 1.0, size=(FIT_L, 5)).astype(F32), top)
        act = nets.gumbel_softmax(nets.mlp_fwd(actors[j], obs)[0], u)
        data.append((obs, act, rng.normal(size=FIT_L).astype(F32), rng.normal(size=(FIT_L, FIT_DIMS[j])).astype(F32),
                     np.zeros(FIT_L, F32)))
    phi = {j: nets.xavier_init(rng, FIT_DIMS[j], 5, FIT_H) for j in range(1, n)}   # observer 0's approximators
    idx = rng.integers(0, FIT_L, size=(FIT_STEPS, FIT_B)).astype(np.int32)
    return dict(actors=actors, data=data, phi=phi, idx=idx)


def mean_kl(actor, phi, obs):
    """mean over the rows of KL(softmax(actor(obs)) || softmax(phi(obs))), float64"""
    def logp(p):
        l = nets.mlp_fwd(p, obs)[0].astype(np.float64)
        l = l - l.max(1, keepdims=True)
        return l - np.log(np.exp(l).sum(1, keepdims=True))
    lp, lq = logp(actor), logp(phi)
    return float((np.exp(lp) * (lp - lq)).sum(1).mean())


def fit_run(fc, lam=LAMBDA):
    """FIT_STEPS approximator steps of observer 0 on the case's index draws;
    {j: (KL at the start, KL at the end)} over the ring's rows"""
    out = {}
    for j, phi in fc["phi"].items():
        ap = Approx({k: v.copy() for k, v in phi.items()}, {k: v.copy() for k, v in phi.items()})
        obs, act = fc["data"][j][0], fc["data"][j][1]
        kl0 = mean_kl(fc["actors"][j], ap.net, obs)
        for idx in fc["idx"]:
            approx_step(ap, obs[idx], act[idx], lam)
        out[j] = (kl0, mean_kl(fc["actors"][j], ap.net, obs))
    return out
