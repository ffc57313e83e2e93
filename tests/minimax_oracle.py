"""M3DDPG ("minimax MADDPG", Li et al., AAAI 2019) on this project's policies,
restated in numpy on top of oracle.trainer (test oracle of mdp_minimax_enable;
DESIGN.md section 20).  The authors' source is not at hand: parity with it is
UNPINNED, the definition is the one in include/maddpg_hip.h.

eps_row[j] >= 0 is the updating agent i's perturbation rate for agent j's action
(eps_row[i] is ignored).  For a critic input x = [obs | a_0 .. a_{n-1}] and a
critic Q, per batch row b and agent j != i:

    g_j   = d Q(x)[b] / d a_j[b]            (rows independent: no batch mean)
    ss    = sum_k g_j[k]^2                  (agent j's k_j logical entries, index order)
    ghat  = g_j * (1 / sqrt(max(ss, 1e-12)))            (TF's l2_normalize)
    a^_j  = a_j - eps_row[j] * ghat         (neither clipped nor renormalised)

Critic step: x = [o' | a~] with the target actors' samples, Q the target critic;
q' = Q'([o' | a^]) enters today's TD line.  Actor step: x = [o | a] with a_i the
fresh sample, Q the critic after its step; p_loss = -mean Q([o | a^_{-i}, a_i])
+ the regulariser, differentiated through a_i only with a^ held constant.

Every function takes dt = float32 (the device's arithmetic, built from
oracle.nets so that eps = 0 is oracle.trainer's update exactly) or float64 (the
same step without any fp32 rounding: the reference of the error budget).
``sign`` = -1 moves the actions the wrong way (the tests show it cannot pass).
All shapes are the logical ones: agent j's action is k_j = widths[j] wide.

``torch_step`` is the second derivation: the same step in float64 with
torch.autograd forming the perturbation direction and every gradient.
"""
import numpy as np

from oracle import nets, trainer

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------ dtype-generic nets
def _p(p, dt):
    return p if dt is F32 else {k: np.asarray(v, dt) for k, v in p.items()}


def fwd(p, x, dt=F32):
    if dt is F32:
        return nets.mlp_fwd(p, x)
    p = _p(p, dt)
    x = np.asarray(x, dt)
    h1 = np.maximum(x @ p["W1"] + p["b1"], 0)
    h2 = np.maximum(h1 @ p["W2"] + p["b2"], 0)
    return h2 @ p["W3"] + p["b3"], (x, h1, h2)


def bwd(p, cache, dy, dt=F32):
    if dt is F32:
        return nets.mlp_bwd(p, cache, dy)
    p = _p(p, dt)
    x, h1, h2 = cache
    g = {"W3": h2.T @ dy, "b3": dy.sum(0)}
    dh2 = (dy @ p["W3"].T) * (h2 > 0)
    g["W2"], g["b2"] = h1.T @ dh2, dh2.sum(0)
    dh1 = (dh2 @ p["W2"].T) * (h1 > 0)
    g["W1"], g["b1"] = x.T @ dh1, dh1.sum(0)
    return g


def in_grad(p, cache, dy, dt=F32):
    if dt is F32:
        return nets.input_grad(p, cache, dy)
    p = _p(p, dt)
    x, h1, h2 = cache
    dh2 = (dy @ p["W3"].T) * (h2 > 0)
    dh1 = (dh2 @ p["W2"].T) * (h1 > 0)
    return dh1 @ p["W1"].T


def gsm(logits, u, dt=F32):
    if dt is F32:
        return nets.gumbel_softmax(logits, u)
    with np.errstate(divide="ignore"):
        z = logits - np.log(-np.log(np.asarray(u, F32).astype(dt)))
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def cin(obs_n, act_n, i, local_q, dt=F32):
    """trainer.critic_input in dt"""
    if dt is F32:
        return trainer.critic_input(obs_n, act_n, i, local_q)
    return np.concatenate([obs_n[i], act_n[i]] if local_q else list(obs_n) + list(act_n), 1).astype(dt)


def act_offsets(obs_n, act_n):
    """column of every agent's action in concat(obs_n + act_n)"""
    o = sum(x.shape[1] for x in obs_n)
    offs = []
    for a in act_n:
        offs.append(o)
        o += a.shape[1]
    return offs


# ---------------------------------------------------------------- perturbation
def perturb(p, x, offs, widths, i, eps_row, dt=F32, sign=1):
    """x^ of the definition above for critic p at input x; also ss [n, B] (nan for j = i)"""
    B = x.shape[0]
    _, cache = fwd(p, x, dt)
    dx = in_grad(p, cache, np.ones((B, 1), dt), dt)
    xh = np.array(cache[0], dt, copy=True)
    ss_n = np.full((len(widths), B), np.nan)
    for j, (o, k) in enumerate(zip(offs, widths)):
        if j == i:
            continue
        g = dx[:, o:o + k]
        ss = np.zeros(B, dt)
        for c in range(k):
            ss = ss + g[:, c] * g[:, c]
        inv = dt(1) / np.sqrt(np.maximum(ss, dt(1e-12)))
        xh[:, o:o + k] = xh[:, o:o + k] - dt(sign * float(eps_row[j])) * (g * inv[:, None])
        ss_n[j] = ss
    return xh, ss_n


def _split(xh, offs, widths):
    return [xh[:, o:o + k] for o, k in zip(offs, widths)]


def critic_grads(agents, i, batch_n, u_tgt, eps_row, gamma=0.95, dt=F32, sign=1):
    """trainer.critic_grads with q' at the perturbed target actions"""
    n = len(agents)
    ag = agents[i]
    obs_n = [b[0].astype(F32).astype(dt) for b in batch_n]
    act_n = [b[1].astype(F32).astype(dt) for b in batch_n]
    obs_next_n = [b[3].astype(F32).astype(dt) for b in batch_n]
    rew = np.asarray(batch_n[i][2], F64)
    done = np.asarray(batch_n[i][4], F64)
    B = len(rew)
    tgt_act_n = [gsm(fwd(agents[j].tgt_actor, obs_next_n[j], dt)[0], u_tgt[j], dt) for j in range(n)]
    widths = [a.shape[1] for a in tgt_act_n]
    xq_t = cin(obs_next_n, tgt_act_n, i, ag.local_q, dt)
    ss = None
    adv = tgt_act_n
    if not ag.local_q and n > 1:
        offs = act_offsets(obs_next_n, tgt_act_n)
        xq_t, ss = perturb(ag.tgt_critic, xq_t, offs, widths, i, eps_row, dt, sign)
        adv = _split(xq_t, offs, widths)
    target_q_next = fwd(ag.tgt_critic, xq_t, dt)[0][:, 0]
    target_q = rew + gamma * (1.0 - done) * target_q_next.astype(F64)
    y = target_q.astype(dt)
    xq = cin(obs_n, act_n, i, ag.local_q, dt)
    q, cache = fwd(ag.critic, xq, dt)
    q = q[:, 0]
    q_loss = np.mean((q.astype(F64) - y.astype(F64)) ** 2)
    dq = ((dt(2) * (q - y)) * dt(F32(1.0 / B) if dt is F32 else 1.0 / B)).astype(dt)[:, None]
    g = bwd(ag.critic, cache, dq, dt)
    stats = {"q_loss": float(q_loss), "target_q": target_q, "rew": rew, "target_q_next": target_q_next,
             "adv": adv, "ss": ss}
    return g, stats


def actor_grads(agents, i, batch_n, u_act, eps_row, actor_reg=1e-3, dt=F32, sign=1):
    """tests.mixed_width.actor_grads with the critic evaluated and differentiated at the
    perturbed replayed actions (the perturbation a constant of the backward)"""
    n = len(agents)
    ag = agents[i]
    obs_n = [b[0].astype(F32).astype(dt) for b in batch_n]
    act_n = [b[1].astype(F32).astype(dt) for b in batch_n]
    B = obs_n[0].shape[0]
    logits, pcache = fwd(ag.actor, obs_n[i], dt)
    A = logits.shape[1]
    a_i = gsm(logits, np.asarray(u_act)[:, :A], dt)
    act_in = list(act_n)
    act_in[i] = a_i
    xp = cin(obs_n, act_in, i, ag.local_q, dt)
    ss = None
    adv = act_in
    if ag.local_q:
        off = obs_n[i].shape[1]
    else:
        offs = act_offsets(obs_n, act_in)
        off = offs[i]
        if n > 1:
            widths = [a.shape[1] for a in act_in]
            xp, ss = perturb(ag.critic, xp, offs, widths, i, eps_row, dt, sign)
            adv = _split(xp, offs, widths)
    qp, qcache = fwd(ag.critic, xp, dt)
    qp = qp[:, 0]
    p_reg = np.mean(logits.astype(F64) ** 2)
    p_loss = -np.mean(qp.astype(F64)) + actor_reg * p_reg
    dqp = np.full((B, 1), -1.0 / B, dt)
    dx = in_grad(ag.critic, qcache, dqp, dt)
    da = dx[:, off:off + A]
    dz = nets.softmax_bwd(a_i, da) if dt is F32 else (da - (da * a_i).sum(-1, keepdims=True)) * a_i
    reg = F32(2 * actor_reg / (B * A)) if dt is F32 else 2 * actor_reg / (B * A)
    dlogits = (dz + logits * reg).astype(dt)
    return bwd(ag.actor, pcache, dlogits, dt), float(p_loss), {"adv": adv, "ss": ss}


def update_batch(agents, i, batch_n, u_tgt, u_act, eps_row, gamma=0.95, grad_clip=0.5, tau=1e-2, actor_reg=1e-3,
                 sign=1):
    """agent i's M3DDPG update on gathered batches (fp32; mutates agents[i]); returns
    (stats list, extras) as trainer.update_batch, extras also holding both steps' a^ and ss"""
    ag = agents[i]
    gq, st = critic_grads(agents, i, batch_n, u_tgt, eps_row, gamma, F32, sign)
    trainer.apply_grads(ag.opt_critic, ag.critic, gq, grad_clip)
    gp, p_loss, ex = actor_grads(agents, i, batch_n, u_act, eps_row, actor_reg, F32, sign)
    trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
    nets.polyak(ag.tgt_actor, ag.actor, tau)
    nets.polyak(ag.tgt_critic, ag.critic, tau)
    return trainer.reference_stats(st, p_loss), {"grad_critic": gq, "grad_actor": gp, "adv_critic": st["adv"],
                                                 "ss_critic": st["ss"], "adv_actor": ex["adv"], "ss_actor": ex["ss"]}


def update(agents, i, buffers, idx, u_tgt, u_act, eps_row, **kw):
    n = len(agents)
    batch_n = [tuple(x[idx] for x in buffers[j]) for j in range(n)]
    return update_batch(agents, i, batch_n, u_tgt, u_act, eps_row, **kw)


def pad5(a_n):
    """[n] x [B, k_j] logical actions -> [B, n, 5] as the device lays them out"""
    out = np.zeros((a_n[0].shape[0], len(a_n), 5), np.asarray(a_n[0]).dtype)
    for j, a in enumerate(a_n):
        out[:, j, :a.shape[1]] = a
    return out


# ---------------------------------------------- the second derivation (autograd)
def torch_step(agents, i, batch_n, u_tgt, u_act, eps_row, gamma=0.95, actor_reg=1e-3, detach=True, sign=1):
    """critic_grads + actor_grads (both against agents' present weights, float64) with
    torch.autograd forming the perturbation direction and every gradient.
    detach=False lets the actor loss differentiate through the perturbation too."""
    import torch
    T = lambda a: torch.tensor(np.asarray(a, F32).astype(F64))  # noqa: E731
    n = len(agents)
    ag = agents[i]

    def net(p, leaf=False):
        return {k: T(v).requires_grad_(leaf) for k, v in p.items()}

    def mlp(p, x):
        h1 = torch.relu(x @ p["W1"] + p["b1"])
        h2 = torch.relu(h1 @ p["W2"] + p["b2"])
        return h2 @ p["W3"] + p["b3"]

    def sample(logits, u):
        return torch.softmax(logits - torch.log(-torch.log(T(u))), -1)

    def move(q_fn, x, offs, widths, keep):
        x = x if x.requires_grad else x.clone().requires_grad_(True)
        (dx,) = torch.autograd.grad(q_fn(x).sum(), x, create_graph=not keep)
        parts, o0 = [], 0
        for j, (o, k) in enumerate(zip(offs, widths)):
            if j == i:
                continue
            g = dx[:, o:o + k]
            ghat = g / torch.sqrt(torch.clamp((g * g).sum(-1, keepdim=True), min=1e-12))
            parts += [x[:, o0:o], x[:, o:o + k] - sign * float(eps_row[j]) * ghat]
            o0 = o + k
        xh = torch.cat(parts + [x[:, o0:]], 1)
        return xh.detach() if keep else xh

    obs_n = [T(b[0]) for b in batch_n]
    act_n = [T(b[1]) for b in batch_n]
    nobs_n = [T(b[3]) for b in batch_n]
    rew, done = torch.tensor(np.asarray(batch_n[i][2], F64)), torch.tensor(np.asarray(batch_n[i][4], F64))
    moved = not ag.local_q and n > 1
    # critic step
    with torch.no_grad():
        at = [sample(mlp(net(agents[j].tgt_actor), nobs_n[j]), u_tgt[j]) for j in range(n)]
    tq = net(ag.tgt_critic)
    xt = torch.cat([nobs_n[i], at[i]], 1) if ag.local_q else torch.cat(nobs_n + at, 1)
    widths = [a.shape[1] for a in at]
    if moved:
        xt = move(lambda x: mlp(tq, x), xt, act_offsets(nobs_n, at), widths, True)
    with torch.no_grad():
        qn = mlp(tq, xt)[:, 0]
        y = rew + gamma * (1.0 - done) * qn
    cq = net(ag.critic, True)
    xq = torch.cat([obs_n[i], act_n[i]], 1) if ag.local_q else torch.cat(obs_n + act_n, 1)
    q_loss = ((mlp(cq, xq)[:, 0] - y) ** 2).mean()
    gq = torch.autograd.grad(q_loss, [cq[k] for k in nets.NAMES])
    # actor step
    pa = net(ag.actor, True)
    cq = net(ag.critic)
    logits = mlp(pa, obs_n[i])
    a_i = sample(logits, np.asarray(u_act)[:, :logits.shape[1]])
    a_in = list(act_n)
    a_in[i] = a_i
    xp = torch.cat([obs_n[i], a_i], 1) if ag.local_q else torch.cat(obs_n + a_in, 1)
    if moved:
        offs = act_offsets(obs_n, a_in)
        xh = move(lambda x: mlp(cq, x), xp, offs, widths, detach)
        if detach:  # the others' actions constants at the moved point, a_i live
            o, k = offs[i], widths[i]
            xp = torch.cat([xh[:, :o], a_i, xh[:, o + k:]], 1)
        else:
            xp = xh
    p_loss = -mlp(cq, xp)[:, 0].mean() + actor_reg * (logits ** 2).mean()
    gp = torch.autograd.grad(p_loss, [pa[k] for k in nets.NAMES])
    npy = lambda gs: {k: g.numpy() for k, g in zip(nets.NAMES, gs)}  # noqa: E731
    return {"grad_critic": npy(gq), "grad_actor": npy(gp), "q_loss": float(q_loss.detach()), "p_loss": float(p_loss.detach()),
            "target_q_next": qn.numpy(), "adv_critic": xt.detach().numpy(), "adv_actor": xp.detach().numpy()}


# ------------------------------------------------------------- fixture hygiene
def clean_idx(c, widths, eps, margin=1e-5, max_iter=40):
    """tests.helpers.relu_margin_clean_idx for the M3DDPG step: agent by agent, replace
    every batch position whose row puts a ReLU input of a net the step evaluates --
    at the unperturbed AND at the perturbed critic inputs -- within margin x (the
    layer's largest |input| over the batch) of zero.  A mask of the first forward
    now also steers the perturbation direction.  float64, round-start weights;
    modifies c["idx"] in place, returns the number of positions replaced."""
    data, n = c["data"], len(c["params"])
    lq = c["local_q"]
    rng = np.random.default_rng(4321)
    L = data[0][0].shape[0]
    ags = [trainer.AgentParams(**{w: c["params"][j][w] for w in ("actor", "critic", "tgt_actor", "tgt_critic")},
                               local_q=lq[j]) for j in range(n)]

    def pre(p, x):
        p = _p(p, F64)
        z1 = x @ p["W1"] + p["b1"]
        z2 = np.maximum(z1, 0) @ p["W2"] + p["b2"]
        # a row with every layer-1 unit inactive has h1 == 0 and z2 == b2 exactly in any
        # arithmetic: its layer 2 has no rounding to keep a margin from (section 28, case A)
        dead = (z1 < 0).all(1)
        if dead.any():
            z2[dead] = 1.0 if dead.all() else np.abs(z2[~dead]).max()
        return [z1, z2]

    def bad(zs):
        out = np.zeros(zs[0].shape[0], bool)
        for z in zs:
            out |= (np.abs(z) < margin * np.abs(z).max()).any(1)
        return out

    replaced = 0
    for i in range(n):
        for _ in range(max_iter):
            rows = c["idx"][i]
            batch_n = [tuple(x[rows] for x in data[j]) for j in range(n)]
            obs = [b[0].astype(F32).astype(F64) for b in batch_n]
            act = [b[1].astype(F32).astype(F64) for b in batch_n]
            nobs = [b[3].astype(F32).astype(F64) for b in batch_n]
            u_t = [np.asarray(c["u_tgt"][i][j])[:, :widths[j]] for j in range(n)]
            zs = []
            at = []
            for j in range(n):
                zs += pre(ags[j].tgt_actor, nobs[j])
                at.append(gsm(fwd(ags[j].tgt_actor, nobs[j], F64)[0], u_t[j], F64))
            xt = cin(nobs, at, i, lq[i], F64)
            zs += pre(ags[i].tgt_critic, xt)
            xc = np.concatenate([obs[i], act[i]], 1) if lq[i] else np.concatenate(obs + act, 1)
            zs += pre(ags[i].critic, xc)
            zs += pre(ags[i].actor, obs[i])
            a_in = list(act)
            a_in[i] = gsm(fwd(ags[i].actor, obs[i], F64)[0], np.asarray(c["u_act"][i])[:, :widths[i]], F64)
            xp = np.concatenate([obs[i], a_in[i]], 1) if lq[i] else np.concatenate(obs + a_in, 1)
            zs += pre(ags[i].critic, xp)
            if not lq[i] and n > 1:
                zs += pre(ags[i].tgt_critic, perturb(ags[i].tgt_critic, xt, act_offsets(nobs, at), widths, i,
                                                     eps[i], F64)[0])
                zs += pre(ags[i].critic, perturb(ags[i].critic, xp, act_offsets(obs, a_in), widths, i, eps[i],
                                                 F64)[0])
            b = bad(zs)
            if not b.any():
                break
            replaced += int(b.sum())
            c["idx"][i][b] = rng.integers(0, L, size=int(b.sum())).astype(np.int32)
        else:
            raise RuntimeError(f"agent {i}: no ReLU-margin-clean batch after {max_iter} resamplings")
    return replaced


def ill_conditioned(ss_n):
    """rows whose ss lies below 1e-6 of the batch median for some perturbed agent (the
    normalised direction amplifies the gradient's rounding error there)"""
    out = np.zeros(ss_n.shape[1], bool)
    for ss in ss_n:
        if not np.isnan(ss).all():
            out |= ss < 1e-6 * np.median(ss)
    return out
