"""MATD3 on this project's policies, restated in numpy on top of oracle.trainer
(test oracle of mdp_td3_enable).

Agent i's k-th update since enable (k = 1, 2, ...):

1. target actions a~_j = gumbel_softmax(target_actor_j(o'_j), u_tgt[j]) -- the
   MADDPG critic step's, unchanged;
2. q1' = Q1_tgt(x'), q2' = Q2_tgt(x') on the same x' = [o' | a~];
   qn = min(q1', q2') in fp32; y64 = r + gamma (1 - done) (double)qn, y = (float)y64;
3. for c = 1, 2: loss_c = mean_b (Q_c(x_b) - y_b)^2, dL/dq = 2 (q - y) / B, raw
   gradients, per-tensor clip_by_norm, Adam of critic c's own optimizer;
4. if k % d == 0: the MADDPG actor step on Q1 after its step, then Polyak of
   the target actor, target Q1 and target Q2;
5. otherwise the actor, its optimizer and all three target nets stay as they are.

The stats are update()'s list with [0] critic 1's loss, [1] p_loss of the
agent's most recent actor step (0 before the first) and [4] the mean of qn.
"""
import numpy as np

from oracle import nets, trainer


def add_twin(ag, critic2, tgt_critic2, lr=1e-2):
    """give an AgentParams object its second critic, target and optimizer, and the update counters"""
    ag.critic2, ag.tgt_critic2 = critic2, tgt_critic2
    ag.opt_critic2 = nets.Adam(critic2, lr=lr)
    ag.td3_k = 0
    ag.td3_actor_steps = 0
    ag.td3_p_loss = 0.0
    return ag


def target_inputs(agents, i, batch_n, u_tgt):
    """x' = [o' | a~] of agent i's target critics"""
    n = len(agents)
    F32 = trainer.F32
    obs_next_n = [b[3].astype(F32) for b in batch_n]
    tgt_act_n = [trainer.target_act(agents[j], obs_next_n[j], u_tgt[j]) for j in range(n)]
    return trainer.critic_input(obs_next_n, tgt_act_n, i, agents[i].local_q)


def target_qs(agents, i, batch_n, u_tgt):
    """(q1', q2') of agent i's two target critics on the same x'"""
    ag = agents[i]
    xq_t = target_inputs(agents, i, batch_n, u_tgt)
    return nets.mlp_fwd(ag.tgt_critic, xq_t)[0][:, 0], nets.mlp_fwd(ag.tgt_critic2, xq_t)[0][:, 0]


def critic_grads(agents, i, batch_n, u_tgt, gamma=0.95):
    """raw gradients of both critics against the clipped double-Q target"""
    F32 = trainer.F32
    ag = agents[i]
    obs_n = [b[0].astype(F32) for b in batch_n]
    act_n = [b[1].astype(F32) for b in batch_n]
    rew = np.asarray(batch_n[i][2], np.float64)
    done = np.asarray(batch_n[i][4], np.float64)
    B = len(rew)
    q1n, q2n = target_qs(agents, i, batch_n, u_tgt)
    qn = np.minimum(q1n, q2n).astype(F32)
    target_q = rew + gamma * (1.0 - done) * qn.astype(np.float64)
    y = target_q.astype(F32)
    xq = trainer.critic_input(obs_n, act_n, i, ag.local_q)
    out = []
    for p in (ag.critic, ag.critic2):
        q, cache = nets.mlp_fwd(p, xq)
        q = q[:, 0]
        loss = np.mean((q.astype(np.float64) - y.astype(np.float64)) ** 2)
        dq = ((F32(2) * (q - y)) * F32(1.0 / B)).astype(F32)[:, None]
        out.append((nets.mlp_bwd(p, cache, dq), float(loss)))
    (g1, l1), (g2, l2) = out
    stats = {"q_loss": l1, "q_loss2": l2, "target_q": target_q, "rew": rew, "target_q_next": qn,
             "take_q1": q1n <= q2n}
    return g1, g2, stats


def update_batch(agents, i, batch_n, u_tgt, u_act, d=2, gamma=0.95, grad_clip=0.5, tau=1e-2, actor_reg=1e-3,
                 actor_grads=None):
    """agent i's next update on gathered batches; returns (stats list, extras).
    actor_grads: another restatement of the actor step's raw gradients
    (tests.mixed_width.actor_grads for agents of different action widths)"""
    ag = agents[i]
    actor_grads = actor_grads or trainer.actor_grads
    ag.td3_k += 1
    g1, g2, st = critic_grads(agents, i, batch_n, u_tgt, gamma)
    trainer.apply_grads(ag.opt_critic, ag.critic, g1, grad_clip)
    trainer.apply_grads(ag.opt_critic2, ag.critic2, g2, grad_clip)
    extra = {"grad_critic": g1, "grad_critic2": g2, "q_loss2": np.float32(st["q_loss2"]),
             "take_q1": st["take_q1"], "actor_step": ag.td3_k % d == 0}
    if ag.td3_k % d == 0:
        gp, p_loss = actor_grads(agents, i, batch_n, u_act, actor_reg)
        trainer.apply_grads(ag.opt_actor, ag.actor, gp, grad_clip)
        nets.polyak(ag.tgt_actor, ag.actor, tau)
        nets.polyak(ag.tgt_critic, ag.critic, tau)
        nets.polyak(ag.tgt_critic2, ag.critic2, tau)
        ag.td3_p_loss = p_loss
        ag.td3_actor_steps += 1
        extra["grad_actor"] = gp
    return trainer.reference_stats(st, ag.td3_p_loss), extra


def update(agents, i, buffers, idx, u_tgt, u_act, **kw):
    n = len(agents)
    batch_n = [tuple(x[idx] for x in buffers[j]) for j in range(n)]
    return update_batch(agents, i, batch_n, u_tgt, u_act, **kw)


def balanced_twin_targets(agents, params2, data, idx, u_tgt):
    """The parity fixtures' rule: two independently drawn target critics can split
    a batch anywhere from 0 % to 100 %, so after drawing agent i's second target
    critic the batch median of q1' - q2' (on that agent's rows and target
    actions) is added to its b3 -- about half the rows then take each branch
    of the min.  params2[i] = dict(critic2=, tgt_critic2=); modified in place."""
    n = len(agents)
    for i in range(n):
        batch_n = [tuple(x[idx[i]] for x in data[j]) for j in range(n)]
        xq_t = target_inputs(agents, i, batch_n, u_tgt[i])
        q1 = nets.mlp_fwd(agents[i].tgt_critic, xq_t)[0][:, 0]
        q2 = nets.mlp_fwd(params2[i]["tgt_critic2"], xq_t)[0][:, 0]
        med = np.median((q1 - q2).astype(np.float64))
        params2[i]["tgt_critic2"]["b3"] = (params2[i]["tgt_critic2"]["b3"] + np.float32(med)).astype(np.float32)
    return params2


def twin_case(c, dims, seed, H=64):
    """second critics and targets for a helpers.synthetic_trainer_case (same shapes as its critics)"""
    rng = np.random.default_rng(seed + 9001)
    n = len(dims)
    out = []
    for i in range(n):
        cin = c["params"][i]["critic"]["W1"].shape[0]
        out.append(dict(critic2=nets.xavier_init(rng, cin, 1, H), tgt_critic2=nets.xavier_init(rng, cin, 1, H)))
    return out
