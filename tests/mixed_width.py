"""Restatements for agents of different action widths (Discrete(A_i), A_i <= 5).

``oracle/trainer.py:106-107`` places agent i's action slice of the critic
input at ``A * i``, which holds only when every agent has the same width.
The reference itself concatenates ``act_ph_n`` (``maddpg.py:85``), so a_i
starts at ``sum_obs + sum_{j<i} A_j``.  ``actor_grads`` here is that; the
rest of the trainer oracle (``critic_grads``, ``nets.*``, ``apply_grads``) is
width-agnostic and is reused.  All shapes here are the reference's (logical)
ones: actions, logits and uniforms of agent j are A_j wide.

The device keeps every action slot 5 wide (zero pad entries): ``joint_rows_w``
and ``pad5`` build its rows and noise arrays from the logical ones.
"""
import numpy as np

from oracle import nets, trainer
from tests.golden.make_golden import make_data
from tests.helpers import row_layout

ACT = 5


def actor_grads(agents, i, batch_n, u_act, actor_reg=1e-3):
    """maddpg.py:37-58 raw actor gradients; a_i sits after the narrower or wider
    actions of agents j < i in concat(obs_n + act_n)"""
    F32 = trainer.F32
    ag = agents[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    B = obs_n[0].shape[0]
    logits, pcache = nets.mlp_fwd(ag.actor, obs_n[i])
    A = logits.shape[1]
    a_i = nets.gumbel_softmax(logits, u_act[:, :A])                # :49 fresh sample
    act_in = list(act_n)
    act_in[i] = a_i
    xp = trainer.critic_input(obs_n, act_in, i, ag.local_q)
    qp, qcache = nets.mlp_fwd(ag.critic, xp)
    qp = qp[:, 0]
    p_reg = np.mean(logits.astype(np.float64) ** 2)               # :46 (mean over B * A_i entries)
    p_loss = -np.mean(qp.astype(np.float64)) + actor_reg * p_reg   # :54-56
    dqp = np.full((B, 1), -1.0 / B, F32)
    dx = nets.input_grad(ag.critic, qcache, dqp)
    if ag.local_q:
        off = obs_n[i].shape[1]
    else:
        off = sum(o.shape[1] for o in obs_n) + sum(a.shape[1] for a in act_n[:i])
    dz = nets.softmax_bwd(a_i, dx[:, off:off + A])
    dlogits = (dz + logits * F32(2 * actor_reg / (B * A))).astype(F32)
    return nets.mlp_bwd(ag.actor, pcache, dlogits), float(p_loss)


def narrow(u_n, widths):
    """[n][B, 5] uniforms -> the list of [B, A_j] the width-agnostic oracle takes"""
    return [np.asarray(u_n[j])[:, :widths[j]] for j in range(len(widths))]


def update(agents, i, buffers, idx, u_tgt, u_act, widths, weights=None, gamma=0.95, grad_clip=0.5, tau=1e-2,
           actor_reg=1e-3):
    """trainer.update for mixed widths; u_tgt [n, B, 5], u_act [B, 5] as the device takes them"""
    n = len(agents)
    ag = agents[i]
    batch_n = [tuple(x[idx] for x in buffers[j]) for j in range(n)]
    gq, st = trainer.critic_grads(agents, i, batch_n, narrow(u_tgt, widths), gamma)
    trainer.apply_grads(ag.opt_critic, ag.critic, gq, grad_clip)
    gp, p_loss = actor_grads(agents, i, batch_n, u_act, actor_reg)
    trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
    nets.polyak(ag.tgt_actor, ag.actor, tau)
    nets.polyak(ag.tgt_critic, ag.critic, tau)
    return trainer.reference_stats(st, p_loss), {"grad_critic": gq, "grad_actor": gp}


def update_round_throughput(agents, buffers, idx_n, u_tgt_n, u_act_n, widths, gamma=0.95, grad_clip=0.5):
    """trainer.update_round_throughput for mixed widths"""
    n = len(agents)
    grads, stats = [], []
    for i in range(n):
        batch_n = [tuple(x[idx_n[i]] for x in buffers[j]) for j in range(n)]
        gq, st = trainer.critic_grads(agents, i, batch_n, narrow(u_tgt_n[i], widths), gamma)
        gp, p_loss = actor_grads(agents, i, batch_n, u_act_n[i])
        grads.append((gq, gp))
        stats.append(trainer.reference_stats(st, p_loss))
    for i, ag in enumerate(agents):
        gq, gp = grads[i]
        trainer.apply_grads(ag.opt_critic, ag.critic, gq, grad_clip)
        trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
        nets.polyak(ag.tgt_actor, ag.actor)
        nets.polyak(ag.tgt_critic, ag.critic)
    return stats, grads


def mixed_case(dims, widths, B, L, seed, local_q=None, H=64):
    """tests.helpers.synthetic_trainer_case with per-agent widths: stored actions
    of agent j are A_j-wide probability vectors, the nets have the reference's
    shapes; idx [n, B], u_tgt [n, n, B, 5], u_act [n, B, 5] (device layout)"""
    rng = np.random.default_rng(seed)
    n, S = len(dims), sum(dims)
    local_q = [False] * n if local_q is None else list(local_q)
    data = []
    for j, (o, a, r, on, d) in enumerate(make_data(seed + 77, L, dims)):
        a = np.asarray(a, np.float32)[:, :widths[j]]
        a = (a / a.sum(1, keepdims=True)).astype(np.float32)
        data.append((o, a, r, on, d))
    params = []
    for i in range(n):
        cin = dims[i] + widths[i] if local_q[i] else S + sum(widths)
        params.append(dict(actor=nets.xavier_init(rng, dims[i], widths[i], H),
                           critic=nets.xavier_init(rng, cin, 1, H),
                           tgt_actor=nets.xavier_init(rng, dims[i], widths[i], H),
                           tgt_critic=nets.xavier_init(rng, cin, 1, H)))
    idx = rng.integers(0, L, size=(n, B)).astype(np.int32)
    top = np.nextafter(np.float32(1), np.float32(0))
    u_tgt = np.minimum(rng.uniform(1e-6, 1.0, size=(n, n, B, ACT)).astype(np.float32), top)
    u_act = np.minimum(rng.uniform(1e-6, 1.0, size=(n, B, ACT)).astype(np.float32), top)
    return dict(data=data, params=params, idx=idx, u_tgt=u_tgt, u_act=u_act, local_q=local_q,
                dims=list(dims), widths=list(widths))


def joint_rows_w(data, dims):
    """tests.helpers.joint_rows for A_j-wide actions: each goes to the head of its
    5-wide slot, the pad entries stay zero"""
    lay, stride = row_layout(dims)
    L = data[0][0].shape[0]
    rows = np.zeros((L, stride), np.float32)
    for j, (o, a, r, on, d) in enumerate(data):
        lj = lay[j]
        rows[:, lj["obs"]:lj["obs"] + dims[j]] = o
        rows[:, lj["act"]:lj["act"] + a.shape[1]] = a
        rows[:, lj["nobs"]:lj["nobs"] + dims[j]] = on
        rows[:, lj["rew"]] = r
        rows[:, lj["done"]] = d
    return rows


def pad_columns(dims, widths, local_q_i=None, agent=None):
    """device rows of a critic W1 block that are padding (interior, per action slot)"""
    if local_q_i:
        return [dims[agent] + k for k in range(widths[agent], ACT)]
    S = sum(dims)
    return [S + ACT * j + k for j in range(len(dims)) for k in range(widths[j], ACT)]
