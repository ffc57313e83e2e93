// mdp_kernels.h -- what the host needs to start the kernels: their argument
// blocks, the dynamic-LDS size of every launch (summed from the kernels' own
// buffer lists, mdp_carve.h), the launch helpers the kernel files share and the
// mdp_launch_* entry points they define.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <type_traits>

#include "mdp_carve.h"
#include "mdp_topo.h"

// Argument blocks: the scalars and pointers a kernel reads first come first and
// the (1.7 KB) Topo last, so a kernel's opening kernarg reads share a few 64-B
// scalar-cache lines (its early branches otherwise chained one miss each).
struct CriticArgs {
  int agent, B;
  const float* theta;
  const float* target;
  const float* replay;
  const int32_t* idx;
  const float* u_tgt;   // [n][B][5] or null
  uint64_t seed;
  const Ctl* ctl;
  double gamma;
  float inv_b;
  float* slab;          // [nwg][slab_stride] partial critic grads (net-relative)
  int slab_stride;
  double* slab_stat;    // [nwg][8]
  double* y_out;        // [B]
  int group;            // target actors run concurrently per pass (LDS budget)
  // k_critic_grad_r only: workgroups per critic row tile, 1 or 2.  With 2 (twins,
  // strict mode when the doubled grid still has a CU per workgroup) both run the
  // tile's step up to B5 from the same inputs and each forms half of its
  // weight-gradient tiles; every slab word keeps its one writer and its chain
  // (here: the word was padding, every other field keeps its offset)
  int twin;
  // k_critic_grad_r only: one extra workgroup draws the NEXT round's indices
  // (pf_count draws into pf_out) while this kernel runs (0: none)
  Ctl* pf_ctl;
  int32_t* pf_out;
  int pf_count;
  // throughput mode (fast kernels): `multi` agents in one launch, agent =
  // workgroup / (B/16); idx, u_tgt, slab, slab_stat, y_out are then bases with
  // per-agent strides and the noise counter is upd_ctr + agent
  int multi;
  int64_t slab_agent_stride;
  // k_critic_grad_r only: B/16 extra workgroups run the SAME agent's actor
  // forward + policy sample of the coming actor step (it needs only the actor
  // weights, which the critic step does not touch) into apre [B][MDP_APRE_W];
  // u_act: injected uniforms of that sample or null (0: no extra workgroups)
  float* apre;
  float* apre_rows;     // the replay rows it gathered, [B][row_stride] (the actor step reads them contiguously)
  const float* u_act;
  // critic_post mode (k_critic_grad_r): the work of this critic step that does
  // not depend on the previous agent's update (target actors j != cpre_prev,
  // the critic forward, the target critic's layer-1 accumulator over obs' and
  // those target actions) was done by extra workgroups of that agent's actor
  // launch into cpre [B][MDP_CPRE_W]; only target actor cpre_prev (Polyak-
  // updated since) and the rest of the step remain (null: the full step)
  const float* cpre;
  const float* cpre_rows;  // the replay rows the critic_pre gathered, [B][row_stride]
  int cpre_prev;
  Topo topo;
};
// prioritized replay (strict mode): the argument block of the critic kernels'
// PER twins (k_critic_grad_r_per, k_critic_grad_per -- the same body with the
// weight at the seed and in the loss).  The uniform kernels keep CriticArgs and
// every instruction they had.  is_w [B] importance-sampling weights: the loss
// is mean_b(w_b (q_b - y_b)^2), dL/dq_b = 2 w_b (q_b - y_b) / B; td_out [B]
// receives |q_b - y_b|
struct CriticArgsPer : CriticArgs {
  const float* is_w;
  float* td_out;
};
// a handle with a squashed Box agent (mdp_set_act_squash): the same
// block under another type, which selects the instantiation whose samplers know
// tanh; every other handle keeps the kernel it had
struct CriticArgsSq : CriticArgs {};
// agent's critic step with an entropy coefficient alpha != 0 (mdp_set_act_entropy,
// DESIGN 29): the soft target, qs = q' - alpha * log pi'(a~_agent | o'_agent).  Its
// samplers know the squash bit (one instantiation serves plain and squashed
// agents); an agent whose coefficient is 0 keeps the kernel it had.  The tile's
// sum of log pi' goes to slot 4 of its slab_stat record
struct CriticArgsEnt : CriticArgs {
  float alpha;
};

// MATD3 (strict mode, general kernels): the argument block of the critic
// kernel's twin instantiation.  theta2 / target2 are param-space bases of the
// second critic and its target (the NDesc offsets of the arena's), slab2 /
// slab_stat2 its partials [nwg][slab_stride] and records [nwg][8]; all four in
// the caller's TD3 buffer.  The TD target is r + gamma (1 - done) min(q1', q2')
struct CriticArgsTwin : CriticArgs {
  const float* theta2;
  const float* target2;
  float* slab2;
  double* slab_stat2;
};

// M3DDPG (strict mode, general kernels): the argument blocks of the
// gradient kernels' minimax instantiations.  eps[j] is this agent's
// perturbation rate for agent j's action (row `agent` of the handle's matrix;
// eps[agent] is ignored).  The critic step moves the other agents' target
// actions, the actor step their replayed actions, by -eps[j] ghat_j, ghat_j
// the l2-normalised gradient of this agent's (target) Q to that action, then
// evaluates the step at the moved point.  adv_out [B][n][MDP_ACT_DIM] (or null)
// receives every agent's action as the second forward reads it
struct CriticArgsMm : CriticArgs {
  float eps[MDP_MAX_AGENTS];
  float* adv_out;
};

// Inferred policies (strict mode, general kernels): the argument block
// of the critic kernel's approximator instantiation.  apx_target is the
// param-space base of the observing agent's target approximators (each in the
// approximated agent's actor span, the arena's NDesc offsets): the target
// action of every agent j != agent comes from it instead of `target`
struct CriticArgsApx : CriticArgs {
  const float* apx_target;
};

// k_approx_grad: one workgroup per (pair, 16-row tile), pair p = workgroup / nwg
// approximates agent agents[p] for one observing agent.  phi: param-space base
// of the observer's approximators; slab [m][nwg][slab_stride] partial gradients
// (net-relative); slab_stat [n][nwg][8] of this observer, indexed by the
// approximated agent: {sum of cross-entropies, sum of entropies} of the tile
struct ApproxArgs {
  int B, m, nwg;
  int agents[MDP_MAX_AGENTS];
  const float* phi;
  const float* replay;
  const int32_t* idx;
  float inv_b, lambda;
  float* slab;
  int slab_stride;
  double* slab_stat;
  Topo topo;
};

// precomputed critic-step work of one batch row (k_actor_grad_r's extra
// workgroups -> k_critic_grad_r in critic_post mode):
//   h1 [64] | h2 [64] (critic forward) | target-critic L1 accumulator [64] | q | pad 3 | a~ [16]
// The accumulator stops at the first MFMA k-step holding a target action of
// the previous agent; critic_post resumes the chain there with every a~ (the
// stored ones + the fresh one), so the result is bit-identical to the
// unsplit critic step
#define MDP_CPRE_W 212

// precomputed actor forward of one batch row (k_critic_grad_r's extra
// workgroups -> k_actor_grad_r): h1 [64] | h2 [64] | logits [8] | sample [8]
#define MDP_APRE_W 144

// (the fields without the Topo: the gradient-pair launch passes ONE Topo for both steps)
struct ActorArgsHead {
  int agent, B;
  const float* theta;
  const float* replay;
  const int32_t* idx;
  const float* u_act;   // [B][5] or null
  uint64_t seed;
  const Ctl* ctl;
  float neg_inv_b;      // dL/dq = -1/B
  float reg_scale;      // 2 * actor_reg / (B * 5) (an agent narrower than 5: Topo::reg_scale_w)
  float* slab;
  int slab_stride;
  double* slab_stat;
  int multi;                  // throughput mode, as CriticArgs
  int64_t slab_agent_stride;
  const float* apre;          // k_actor_grad_r: the forward precomputed by the critic launch, or null
  const float* apre_rows;     // ... and its replay rows [B][row_stride] (read instead of a gather)
  // k_actor_grad_r: B/16 extra workgroups run the NEXT critic step's
  // independent work (agent cpre_agent, indices cpre_idx) into cpre (null: none)
  float* cpre;
  float* cpre_rows;
  int cpre_agent;
  const int32_t* cpre_idx;
  const float* target;        // target nets (the critic_pre role's target actors / critic)
};
struct ActorArgs : ActorArgsHead {
  Topo topo;
};
struct ActorArgsSq : ActorArgs {};  // as CriticArgsSq
// agent's actor step with alpha != 0, as CriticArgsEnt: the loss gains alpha *
// mean_b(log pi(a_b | o_b)) of the fresh sample; alpha_b = alpha / B in float.  Slot
// 0 of the tile's record is the sum of q - alpha * log pi, slot 4 that of log pi
struct ActorArgsEnt : ActorArgs {
  float alpha, alpha_b;
};
struct ActorArgsMm : ActorArgs {  // M3DDPG, as CriticArgsMm
  float eps[MDP_MAX_AGENTS];
  float* adv_out;
};

// throughput mode on the general kernels: agent i's critic step and actor step
// (independent there: both read the round-start parameters) as ONE launch --
// workgroups [0, B/16) the critic step, [B/16, 2 B/16) the actor step
struct GradPairArgs {
  CriticArgs c;
  ActorArgsHead x;
};

struct ReduceArgs {
  const float* slab;
  int nwg, slab_stride;
  float* grad;
  int64_t off, size;
  float* beta;          // [4] of this optimizer: next powers (TF variables), this step's powers
  float b1, b2;
  Ctl* ctl;
  int bump_ctr;         // actor phase: advance the training-noise counter
};

#define MDP_APPLY_CHUNK 1024  // parameters per apply workgroup

struct ApplyArgs {
  int blk[7], oblk[7];  // prefix counts of chunk workgroups per tensor (net / other)
  float* theta;
  float* target;
  float* m;
  float* v;
  float* grad;
  const float* slab;    // null: read grad[] (already reduced / all-reduced)
  int slab_stride, nwg;
  float scale, clip, lr, b1, b2, eps;
  float* beta;          // [2] beta1^t, beta2^t of this optimizer
  int polyak;
  float pa, pb;         // fp32(1 - tau), fp32(1 - (1 - tau))
  // 0 none, 1 critic, 1 + A actor (A = the agent's action width, 6 for Discrete(5):
  // the p_reg stat is the mean of its B * A squared logits)
  int stats_mode;
  const double* slab_stat;
  const double* y;
  int B;
  float reg;
  double* stats_out;
  uint32_t* ticket;
  Ctl* ctl;
  int bump_ctr;         // the last workgroup advances Ctl::upd_ctr by this much
  NDesc net, other;
};

// k_reduce_apply (mdp_apply_fused.hip): batch reduction + optimizer step in one launch
#ifndef MDP_RA_NARROW
#define MDP_RA_NARROW 1   // (mdp_apply_fused.hip, mdp_ra_narrow; k_reduce follows the same rule)
#endif
#define MDP_RA_CHUNK 256   // parameters per workgroup
#define MDP_RA_MAXCH 256   // chunks per tensor the sync area holds
// Direct xGMI gradient exchange of the data-parallel step (phase 3 below):
// every rank owns one exchange buffer (uncached device memory, IPC-exported)
// of 64-bit words laid out as
//   [2 slots][world][PT + MDP_XCH_PROBE]   word = epoch << 32 | fp32 bits
// (slot = exchange epoch & 1; the last MDP_XCH_PROBE words of a row belong
// to the connection probe) and holds every peer's buffer mapped
// (hipIpcOpenMemHandle).  Rank r stores each value of its reduced chunk, tagged
// with the epoch, into row [slot][r] of every peer with ONE 64-bit
// system-scope store; the receiver polls each word of its peers' rows until
// the tag equals the epoch (data and flag arrive together: no fences, no
// separate flag round trip -- the LL protocol) and sums the world's values in
// rank order, so every rank computes the identical sum and replicas stay
// bit-equal.  Epoch 0 never occurs (the buffer starts zeroed).
#define MDP_XCH_MAXW 8
#define MDP_XCH_PROBE 2048   // probe words per row (8 chunks)
struct XchgDesc {
  int world, rank;
  int64_t pt;                        // words per row: param-space length + MDP_XCH_PROBE
  uint64_t* data[MDP_XCH_MAXW];      // rank q's exchange buffer in this process (data[rank] local)
};
inline int64_t mdp_xch_bytes(int world, int64_t param_floats) {
  return 8 * (2 * (int64_t)world * (param_floats + MDP_XCH_PROBE));
}

struct FusedApplyArgs {
  int pf_count;         // (below)
  int phase;            // 0 reduce + step; 1 reduce into grad[] only; 2 step from grad[] (all-reduced);
                        // 3 reduce, xGMI exchange with every rank (xd), step x ap.scale
  int rblk[7];          // prefix counts of MDP_RA_CHUNK workgroups per tensor of ap.net
  uint32_t* sync_ctr;   // 6 tensor counters of this (agent, net), 32 words apart
  uint64_t* sync_part;  // [6][MDP_RA_MAXCH][2] published sums of squares (epoch-tagged halves)
  uint32_t* done_ctr;   // workgroups finished (last one advances beta)
  const XchgDesc* xd;   // phase 3: device copy of the exchange descriptor
  int net_id;           // phase 3: 2 * agent + net (epoch counter)
  uint32_t* xstep;      // phase 3: Ctl::xstep[net_id], exchanges done for this net
  uint64_t* wstat;      // phase 3: Ctl::xw_ticks when the exchange waits are stamped, else null
  // pf_count > 0: one extra (last) workgroup draws pf_count indices of the NEXT
  // round into pf_out, continuing the MT19937 stream (a piece of the draw the
  // fast kernels make beside the critic step; general-kernel configurations)
  int32_t* pf_out;
  Ctl* pf_ctl;
  ApplyArgs ap;         // ap.slab / nwg / slab_stride: the partial gradients
};
// sync area: per (agent, net) 8 counters x 128 B (6 done, 7 norm epoch), then [6][MAXCH][2] tagged words
inline int64_t mdp_ra_sync_bytes() {
  return (int64_t)MDP_MAX_AGENTS * 2 * 8 * 128 + (int64_t)MDP_MAX_AGENTS * 2 * 6 * MDP_RA_MAXCH * 16;
}

// ---- prioritized replay (mdp_per.hip): one sum tree per agent in the caller's
// PER buffer.  A tree over P = 2^k >= capacity leaves is the heap array
// node[2 P] of {sum, min}: node 1 the root, node P + i the leaf of ring
// position i, node 0 unused; an unfilled leaf is {0, +inf}.
#define MDP_PER_STREAM 0x50000u   // Philox stream of the stratified draw: 0x50000 | agent
#define MDP_PER_TOP 2048          // nodes of the top levels k_per_sample keeps in LDS
struct PerNode {
  float sum, min;
};
struct PerHdr {                   // the sync's own cursor (device state: graphs stay argument-invariant)
  int64_t seen_steps;             // Ctl::env_steps at the last sync
  int64_t rows_synced;            // leaves reset by ring writes so far (mdp_per_info)
  uint32_t ticket;
  uint32_t pad[11];
};
struct PerState {                 // per agent
  float beta;
  uint32_t samples;               // sample calls so far: the draw's Philox counter
  uint32_t ticket;
  uint32_t pad[13];
};
struct PerSyncArgs {
  const Ctl* ctl;
  PerHdr* hdr;
  PerNode* trees;
  int64_t tree_stride;            // nodes per agent (2 P)
  int64_t P, cap;
  int E;                          // ring rows per env step
  int64_t host_rows;              // rows the host wrote since the last sync (eager calls only)
  int reset;                      // rebuild every leaf from the ring length
  // a new row's priority is powf(upper, alpha) formed on the device, the very
  // value k_per_update gives a row whose error reaches the clip
  float upper, alpha;
};
struct PerSampleArgs {
  const PerNode* trees;
  int64_t tree_stride, P, cap;
  PerState* st;                   // of the launch's first agent
  int agent0, count;
  const float* u;                 // [count] injected uniforms (one agent) or null: device Philox
  const int32_t* idx_in;          // [count] rows given by the caller (weights only) or null: stratified descent
  int32_t* idx_out;               // per agent `stride` apart
  float* w_out;
  int64_t stride;
  uint64_t seed;
  float beta_inc;
};
struct PerUpdateArgs {
  PerNode* trees;
  int64_t tree_stride, P, cap;
  int count;
  const Ctl* ctl;                 // positions at or beyond Ctl::len (unfilled) are ignored
  const int32_t* pos;             // per agent `stride` apart
  const float* val;               // priorities (from_err 0) or |TD errors| (from_err 1)
  int64_t stride;
  int from_err;
  float eps, upper, alpha;
};
hipError_t mdp_launch_per_sync(const PerSyncArgs& a, int agents, hipStream_t s);
hipError_t mdp_launch_per_sample(const PerSampleArgs& a, int agents, hipStream_t s);
hipError_t mdp_launch_per_update(const PerUpdateArgs& a, int agents, hipStream_t s);

struct RolloutArgs {
  Topo topo;
  EnvDesc env;
  const float* theta;
  float* replay;
  int64_t cap;
  float* pos;
  float* vel;
  int32_t* goal;
  int32_t* ep_step;
  float* ep_rew;
  float* eplog;
  int64_t eplog_cap;
  // env copies in lockstep (all terminate on the same step): episode e of a
  // step is logged at slot episodes + e -- env order, deterministic; otherwise
  // in arrival order
  int eplog_by_env;
  Ctl* ctl;
  uint64_t seed;
  int E, env_base;
  const float* act_in;
  const float* u_in;
  uint32_t* ticket;
  float* bench;  // benchmark_data records [E][n][MDP_BENCH_W] or null
  // > 0: one extra workgroup draws the step's first-round indices (pf_count
  // randint draws against the ring length after this step) beside the envs
  int pf_count;
  int32_t* pf_out;
  // consecutive env steps in this launch (1; > 1 only with one env workgroup,
  // no draw, no bench records and the policies' own actions)
  int nsteps;
  float* comm;  // [E][n][MDP_ACT_DIM] agents' state.c, or null (every agent silent: env_dim_c == 0)
};

struct EnvResetArgs {
  EnvDesc env;
  uint64_t seed;
  uint32_t ctr;
  int env_base, E;
  float* pos;
  float* vel;
  int32_t* goal;
  int32_t* ep_step;
  float* ep_rew;
  float* comm;  // as RolloutArgs::comm
};

struct EnvObsArgs {
  Topo topo;
  EnvDesc env;
  int E;
  const float* pos;
  const float* vel;
  const int32_t* goal;
  const float* comm;  // as RolloutArgs::comm
  float* obs;
};

// k_eval_episodes: episode ids [first, first + episodes), 16 per workgroup
struct EvalEpArgs {
  Topo topo;
  EnvDesc env;
  const float* theta;
  uint64_t seed;
  uint32_t first;
  int episodes;
  int mode;            // MDP_EVAL_SAMPLE / MDP_EVAL_MEAN
  const float* u_in;   // [episodes][max_ep_len][n][MDP_ACT_DIM] injected uniforms or null
  float* ret;          // [episodes][n]
  float* bench;        // [episodes][n][MDP_BENCH_W] record sums or null
};

// k_eval_episodes<H, EvalMuArgs>: EvalEpArgs' episodes for every row of a matchup
// table; theta is unused (agent j of matchup m plays bank + table[m][j] * set_stride)
struct EvalMuArgs : EvalEpArgs {
  const float* bank;     // [n_sets][set_stride], each set laid out as the theta region
  const int32_t* table;  // [matchups][n] set indices (device)
  int64_t set_stride;    // floats per set (mdp_actor_set_floats)
  int matchups;          // ret [matchups][episodes][n], bench [matchups][episodes][n][MDP_BENCH_W]
};

// k_eval_episodes<H, EvalQArgs> (mdp_evaluate_q): EvalEpArgs' episodes played
// `steps` steps without reset, every agent's live critic(s) scored on the row
// tile after the step's sample; ret / bench are unused (null)
struct EvalQArgs : EvalEpArgs {
  const float* theta2;  // the TD3 buffer's theta region (the twin critic), null when ncrit == 1
  int steps;            // steps per episode; u_in is [episodes][steps][n][MDP_ACT_DIM]
  int ncrit;            // C: 1, or 2 after mdp_td3_enable
  int qin;              // widest critic input of a local_q agent (0: none): the staging tile's width
  float* q;             // [episodes][steps][n][ncrit]
  float* rew;           // [episodes][steps][n]
};

// k_eval_returns: one thread per (episode, agent) over the traces k_eval_episodes<H, EvalQArgs> wrote
struct EvalRetArgs {
  int episodes, n, steps, scored, ncrit;
  float gamma;
  const float* q;    // [episodes][steps][n][ncrit]
  const float* rew;  // [episodes][steps][n]
  float* g;          // [episodes][steps][n]
  float* gap;        // [episodes][n][ncrit]
};

struct EvalArgs {
  const float* P;
  NDesc net;
  int in, rows;
  const float* x;
  float* out;
  int gumbel;
  const float* u;
  uint64_t seed;
  uint32_t stream, ctr;
  int act_w;  // gumbel: the agent's action space, kind bit | squash bit | action width (topo_act_space)
};

// kernel width that serves --num-units u: the gradient / rollout / eval kernels
// are instantiated for H = 64, 128, 256 (the fast register-resident ones for 64)
inline int mdp_device_units(int u) { return u <= 64 ? 64 : (u <= 128 ? 128 : 256); }

// ---- dynamic LDS sizes: each function sums the buffer list its kernel carves
// (mdp_carve.h), with the list's parameters computed from the Topo
// k_critic_grad / k_actor_grad (mdp_grads.hip)
inline int lds_critic_bytes(const Topo& t, int G) {
  int words = 0;
  MDP_CARVE_CRITIC(MDP_CARVE_WORDS, lds_ld(t.row_stride), lds_ld(t.cin_max), MDP_R * (t.H + 1), G)
  return 4 * words;
}
inline int lds_critic_twin_bytes(const Topo& t, int G) {
  int words = 0;
  MDP_CARVE_TWIN(MDP_CARVE_WORDS)
  return lds_critic_bytes(t, G) + 4 * words;
}
inline int lds_actor_bytes(const Topo& t) {
  int words = 0;
  MDP_CARVE_ACTOR(MDP_CARVE_WORDS, lds_ld(t.row_stride), lds_ld(t.cin_max), MDP_R * (t.H + 1), t.H)
  return 4 * words;
}
// the entropy instantiation's tail (CriticArgsEnt)
inline int lds_critic_ent_bytes(const Topo& t, int G) {
  int words = 0;
  MDP_CARVE_ENT(MDP_CARVE_WORDS)
  return lds_critic_bytes(t, G) + 4 * words;
}
// the minimax instantiations' tail, in words
inline int lds_mm_dxa(const Topo& t) {
  int words = 0;
  MDP_CARVE_MM(MDP_CARVE_WORDS, t.n)
  return words;
}
inline int lds_critic_mm_bytes(const Topo& t, int G) { return lds_critic_bytes(t, G) + 4 * lds_mm_dxa(t); }
inline int lds_actor_mm_bytes(const Topo& t) { return lds_actor_bytes(t) + 4 * lds_mm_dxa(t); }
// k_approx_grad, sized for the widest observation (a workgroup carves its own agent's)
inline int mdp_approx_threads(int H) { return 4 * H; }  // one forward tile per wave
inline int lds_approx_bytes(const Topo& t) {
  int omax = 1;
  for (int j = 0; j < t.n; ++j) omax = t.ag[j].obs_dim > omax ? t.ag[j].obs_dim : omax;
  int words = 0;
  MDP_CARVE_APPROX(MDP_CARVE_WORDS, lds_ld(omax), MDP_R * (t.H + 1))
  return 4 * words;
}
#define MDP_LDS_BUDGET (160 * 1024)
// fast (register-resident, H = 64) variants in mdp_grads_r.hip
// actor_pre role of k_critic_grad_r (actor_pre_tile)
inline int lds_actor_pre_bytes(const Topo& t) {
  int words = 0;
  MDP_CARVE_ACTOR_PRE(MDP_CARVE_WORDS, lds_ld(t.row_stride))
  return 4 * words;
}
// k_critic_grad_r, whose launch also holds the actor_pre workgroups (the smaller carve)
inline int lds_critic_r_bytes(const Topo& t, int agent) {
  const int na = t.ag[agent].local_q ? 1 : t.n;
  int words = 0;
  MDP_CARVE_CRITIC_R(MDP_CARVE_WORDS, lds_ld(t.row_stride), lds_ld(MDP_ACT_DIM * na))
  const int pre = lds_actor_pre_bytes(t);
  return 4 * words > pre ? 4 * words : pre;
}
inline int lds_actor_r_bytes(const Topo& t) {
  int words = 0;
  MDP_CARVE_ACTOR_R(MDP_CARVE_WORDS, lds_ld(t.row_stride))
  return 4 * words;
}
// critic_pre role of k_actor_grad_r (critic_pre_tile, always a MADDPG critic's).
// Exact: the hand-written formula this replaces counted 5632 bytes the tile
// never takes; the launch uses max(lds_actor_r_bytes, this), which the actor
// carve decides either way
inline int lds_critic_pre_bytes(const Topo& t) {
  int words = 0;
  MDP_CARVE_CRITIC_PRE(MDP_CARVE_WORDS, lds_ld(t.row_stride), lds_ld(MDP_ACT_DIM * t.n))
  return 4 * words;
}
// the fast kernels hold every weight of a wave in registers: H = 64, at most 3
// target actors, actor inputs <= 64, critic inputs <= 80, target-critic action part <= 20;
// their sampler is the Gumbel-softmax: no agent of the topology may have a Box space
inline bool grads_r_ok(const Topo& t, int agent) {
  if (t.H != 64 || topo_any_box(t)) return false;
  const ADesc& ag = t.ag[agent];
  const int na = ag.local_q ? 1 : t.n;
  if (na > 3) return false;
  for (int j = 0; j < t.n; ++j)
    if (t.ag[j].obs_dim > 64) return false;
  if (ag.cin > 80) return false;
  if ((ag.local_q ? ag.obs_dim : t.sum_obs) > 64) return false;
  return 5 * na <= 20;
}
// k_rollout, k_eval_episodes
inline int lds_rollout_bytes(const Topo& t) {
  int words = 0;
  MDP_CARVE_ROLLOUT(MDP_CARVE_WORDS, lds_ld(t.row_stride), t.H + 1, MDP_ROLLOUT_PAR_W(t.H))
  return 4 * words;
}
// k_eval_episodes<H, EvalMuArgs>
inline int lds_eval_matchups_bytes(const Topo& t) {
  int words = 0;
  MDP_CARVE_EVAL_MU(MDP_CARVE_WORDS)
  return lds_rollout_bytes(t) + 4 * words;
}
// k_eval_episodes<H, EvalQArgs>; qin: the widest critic input of a local_q agent, 0 when none
inline int lds_eval_q_in(const Topo& t) {
  int qin = 0;
  for (int j = 0; j < t.n; ++j)
    if (t.ag[j].local_q && t.ag[j].cin > qin) qin = t.ag[j].cin;
  return qin;
}
inline int lds_eval_q_bytes(const Topo& t) {
  const int qin = lds_eval_q_in(t);
  int words = 0;
  if (qin) { MDP_CARVE_EVAL_QV(MDP_CARVE_WORDS, lds_ld(qin)) }
  return lds_rollout_bytes(t) + 4 * words;
}
// k_mlp_eval
inline int lds_eval_bytes(int in, int H) {
  int words = 0;
  MDP_CARVE_MLP_EVAL(MDP_CARVE_WORDS, lds_ld(in), H + 1)
  return 4 * words;
}

// ---- per-launch timing (bench.py's kernel pass): when the host armed a
// start/stop event pair for the next launch, that launch carries them on its
// own dispatch packet (hipExtLaunchKernel), so their elapsed time is the
// packet's begin -> end -- the interval rocprofv3 --kernel-trace reports --
// with no marker packets of their own in between
struct MdpLaunchEv {
  hipEvent_t start = nullptr, stop = nullptr;
};
MdpLaunchEv& mdp_launch_ev();  // this host thread's armed pair (mdp_api.cpp)
template <typename F, typename... Args>
inline void mdp_launch(F kernel, const dim3& grid, const dim3& block, uint32_t lds, hipStream_t s, Args... args) {
  MdpLaunchEv& e = mdp_launch_ev();
  if (e.start) {
    const hipEvent_t a = e.start, z = e.stop;
    e.start = e.stop = nullptr;
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, a, z, 0u, args...);
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  }
}
// the kernels' hidden widths: f(std::integral_constant<int, H>) for the H given
template <typename F>
inline hipError_t mdp_for_width(int H, F&& f) {
  switch (H) {
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    case 256: return f(std::integral_constant<int, 256>{});
    default: return hipErrorInvalidValue;
  }
}
// before kernel instantiation K's first launch: let it take up to LIMIT bytes of
// dynamic LDS (an unsupported opt-in must not poison the next launch check)
template <auto K, int LIMIT>
inline void mdp_raise_lds_limit() {
  static bool done = false;
  if (!done) {
    (void)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, LIMIT);
    (void)hipGetLastError();
    done = true;
  }
}
// one launch of K with `lds` bytes of dynamic LDS, on the timed dispatch packet when one is armed
template <auto K, int LIMIT = MDP_LDS_BUDGET, typename A>
inline hipError_t mdp_launch_lds(const dim3& grid, const dim3& block, int lds, hipStream_t s, const A& a) {
  mdp_raise_lds_limit<K, LIMIT>();
  mdp_launch(K, grid, block, lds, s, a);
  return hipGetLastError();
}

hipError_t mdp_launch_critic_grad(const CriticArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_actor_grad(const ActorArgs& a, int H, int lds_bytes, hipStream_t s);
// an agent with an entropy coefficient (alpha != 0): its own instantiations
hipError_t mdp_launch_critic_grad_ent(const CriticArgsEnt& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_actor_grad_ent(const ActorArgsEnt& a, int H, int lds_bytes, hipStream_t s);
// out[0] = (sum over the nwg records of slot 4) / B: the mean log pi of the launch before it
hipError_t mdp_launch_entropy_fold(const double* slab_stat, int nwg, int B, double* out, hipStream_t s);
hipError_t mdp_launch_grad_pair(const GradPairArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_critic_grad_r(const CriticArgs& a, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_critic_grad_per(const CriticArgsPer& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_critic_grad_twin(const CriticArgsTwin& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_critic_grad_mm(const CriticArgsMm& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_actor_grad_mm(const ActorArgsMm& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_critic_grad_apx(const CriticArgsApx& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_approx_grad(const ApproxArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_critic_grad_r_per(const CriticArgsPer& a, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_actor_grad_r(const ActorArgs& a, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_rollout(const RolloutArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_eval(const EvalArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_eval_episodes(const EvalEpArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_eval_matchups(const EvalMuArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_eval_q(const EvalQArgs& a, int H, int lds_bytes, hipStream_t s);
hipError_t mdp_launch_eval_returns(const EvalRetArgs& a, hipStream_t s);
hipError_t mdp_launch_eval_reset(const EnvDesc& env, uint64_t seed, uint32_t first, int count, float* pos, float* vel,
                                 int32_t* goal, hipStream_t s);
hipError_t mdp_launch_apply(const ApplyArgs& a, hipStream_t s);
hipError_t mdp_launch_reduce(const ReduceArgs& a, hipStream_t s);
// lanes: the host allows the narrow launch's register body where mdp_ra_lanes(f) holds
hipError_t mdp_launch_reduce_apply(const FusedApplyArgs& f, hipStream_t s, bool lanes);
bool mdp_ra_lanes(const FusedApplyArgs& f);
// throughput mode: the optimizer steps of `count` nets in one launch; list[]
// lives in device memory (written once), wg_start[q] = first workgroup of net q
#define MDP_RA_BATCH_MAX (2 * MDP_MAX_AGENTS)
struct RaBatch {
  const FusedApplyArgs* list = nullptr;
  int count = 0;
  int narrow = 0;       // fan-in <= 64 partials: 256-thread workgroups (mdp_ra_narrow);
                        // 2: ... with the register body (mdp_ra_lanes holds for every net of list[])
  int wg_start[MDP_RA_BATCH_MAX + 1] = {};
  // pf_count > 0: one extra (last) workgroup draws pf_count indices of the next
  // round into pf_out, continuing the MT19937 stream in pf_ctl (as FusedApplyArgs)
  int pf_count = 0;
  int32_t* pf_out = nullptr;
  Ctl* pf_ctl = nullptr;
};
int mdp_ra_grid(const FusedApplyArgs& f);
hipError_t mdp_ra_occupancy(int* per_cu);   // co-resident k_reduce_apply workgroups per CU
hipError_t mdp_spin_kernels_scratch(int* bytes);  // largest scratch per lane of the spinning kernels
// grid of the fused optimizer launch of (agent, net): the 256-parameter chunks
// of the net, for the actor step the Polyak workgroups of the critic, one stats
// workgroup (mirrors fused_args_for / apply_args / mdp_ra_grid)
inline int mdp_ra_grid_of(const Topo& t, int agent, int net) {
  const NDesc& d = net ? t.ag[agent].critic : t.ag[agent].actor;
  const NDesc& o = net ? t.ag[agent].actor : t.ag[agent].critic;
  int g = 2;  // + the stats workgroup and a slot for an index-draw workgroup
  for (int k = 0; k < 6; ++k) {
    g += (d.t[k].rows * d.t[k].cols + MDP_RA_CHUNK - 1) / MDP_RA_CHUNK;
    if (!net) g += (o.t[k].rows * o.t[k].cols + MDP_APPLY_CHUNK - 1) / MDP_APPLY_CHUNK;
  }
  return g;
}
// the fused launch is safe: every tensor's chunks fit the sync area and the
// whole grid is co-resident on `capacity` workgroup slots
inline bool mdp_ra_fits(const Topo& t, int agent, int net, int capacity) {
  const NDesc& d = net ? t.ag[agent].critic : t.ag[agent].actor;
  for (int k = 0; k < 6; ++k)
    if ((d.t[k].rows * d.t[k].cols + MDP_RA_CHUNK - 1) / MDP_RA_CHUNK > MDP_RA_MAXCH) return false;
  return mdp_ra_grid_of(t, agent, net) <= capacity;
}
hipError_t mdp_launch_reduce_apply_batch(const RaBatch& b, hipStream_t s);
hipError_t mdp_ra_batch_occupancy(int* per_cu);
// connection probe of the xGMI exchange: nchunk chunks of a rank-tagged
// pattern through the same exchange code, *bad += mismatching parameters,
// *fault = 2 when a peer's flag did not arrive in time
hipError_t mdp_launch_xchg_probe(const XchgDesc* xd, uint32_t ep, int nchunk, uint32_t* bad, uint32_t* fault,
                                 hipStream_t s);
hipError_t mdp_launch_make_index(Ctl* ctl, int count, int32_t* out, hipStream_t s);
// target <- pa target + pb theta over n floats (make_update_exp, maddpg.py:20-26),
// skipped once Ctl::fault is set; n a multiple of 4
hipError_t mdp_launch_polyak(float* target, const float* theta, int64_t n, float pa, float pb, const Ctl* ctl,
                             hipStream_t s);
hipError_t mdp_launch_gather(const float* replay, int stride, const int32_t* idx, int count, float* out,
                             hipStream_t s);
hipError_t mdp_launch_count_nonfinite(const float* p, int64_t n, uint32_t* cnt, hipStream_t s);
hipError_t mdp_launch_put_rows(float* replay, int stride, int64_t cap, int64_t next, const float* src, int64_t rows,
                               hipStream_t s);
hipError_t mdp_launch_put_agent(float* replay, int stride, const ADesc& ag, const int64_t* pos, const float* cols,
                                int64_t rows, hipStream_t s);
hipError_t mdp_launch_env_reset(const EnvResetArgs& a, hipStream_t s);
hipError_t mdp_launch_env_obs(const EnvObsArgs& a, hipStream_t s);
hipError_t mdp_launch_set_ring(Ctl* ctl, int64_t len, int64_t next, hipStream_t s);
