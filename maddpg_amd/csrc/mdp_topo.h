// mdp_topo.h -- problem topology shared by host launch code and kernels.
//
// Param space (one region each for theta, target, Adam m, Adam v, grad):
//   [agent 0: actor | critic][agent 1: actor | critic] ...
// each net = W1[in][H] b1[H] W2[H][H] b2[H] W3[H][out] b3[out]
// (experiments/train.py:43-45, TF fully_connected stores W as [in, out]),
// every tensor padded to a multiple of 4 floats (16-B aligned).
//
// Joint replay row (one row per transition, shared by all agents, because the
// reference draws ONE index set and gathers it from every agent's buffer,
// maddpg.py:167-178):
//   [obs_0 .. obs_{N-1} | act_0 .. act_{N-1} | obs'_0 .. obs'_{N-1} | rew_0..rew_{N-1} | done_0..done_{N-1} | pad]
// so the MADDPG critic input concat(obs_n + act_n) (maddpg.py:85) is the row's
// contiguous prefix.
#pragma once
#include <stdint.h>

#include "../../include/maddpg_hip.h"

#define MDP_MAX_ENT 16

struct TDesc {
  int off, rows, cols;
};
struct NDesc {
  TDesc t[6];  // W1 b1 W2 b2 W3 b3
  int off, size, in, out;
};
struct ADesc {
  NDesc actor, critic;
  int obs_dim, obs_off, act_off, nobs_off, rew_off, done_off;
  int local_q, cin, a_in_off;  // critic input width; offset of a_i inside it
};
struct Topo {
  int n, H, row_stride, sum_obs, cin_max, obs_max;
  ADesc ag[MDP_MAX_AGENTS];
  // Per-agent action widths: agent j has a Discrete(A_j) space, A_j in
  // 1..MDP_ACT_DIM (mdp_set_act_dims), 4 bits each (topo_act_w).  Every layout
  // keeps the agent's slot MDP_ACT_DIM wide: the replay row, the critic input
  // columns, the actor's W3 / b3.  The agent uses the first A_j entries; the
  // pad entries are exactly zero everywhere.  (Behind the descriptors, in one
  // word: the argument blocks of the gradient kernels end with their Topo, so
  // every field the all-5 path reads stays where it was.)
  // Bit 3 of agent j's nibble is its action kind (mdp_set_act_spaces): 0
  // Discrete(A_j), the low bits A_j; 1 Box(d_j), the low bits d_j in {1, 2}.
  // A Box actor's head is [mean (d) | logstd (d)], 2 d <= MDP_ACT_DIM wide in
  // the same W3 / b3 block; its action fills the first d entries of the slot
  // (topo_act_w is the ACTION width of either kind, topo_head_w the head's).
  // A Box width needs two bits, so bit 2 of a Box agent's nibble is its squash
  // (mdp_set_act_squash): 0 none, 1 tanh -- the action is tanh of the sample.
  // The bit means nothing without the Box bit (a Discrete width may be 4 or 5),
  // and changes no width: topo_act_w masks a Box agent's nibble with 3.
  uint32_t act_w4;
  float reg_scale_w[MDP_ACT_DIM];  // actor regulariser 2 * actor_reg / (B * A) for A = 1..5 (A < 5: ActorArgs::reg_scale is A = 5's)
};
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int topo_act_w(const Topo& t, int j) {
  const uint32_t s = t.act_w4 >> (4 * j);
  return (int)(s & ((s & 8u) ? 3u : 7u));
}
// the same where no agent can be squashed (bit 2 is a width bit alone): the
// kernels of a handle without a squash, and of the variants that refuse Box,
// keep the mask they were compiled with before the squash existed
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int topo_act_w7(const Topo& t, int j) { return (int)((t.act_w4 >> (4 * j)) & 7u); }
// agent j's whole nibble: kind bit | squash bit | action width (the samplers' argument)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t topo_act_space(const Topo& t, int j) { return (t.act_w4 >> (4 * j)) & 15u; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool topo_act_box(const Topo& t, int j) { return ((t.act_w4 >> (4 * j)) & 8u) != 0u; }
// width of the actor's head: A_j logits, or mean | logstd of a Box(d_j)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int topo_head_w(const Topo& t, int j) { return topo_act_w(t, j) << (topo_act_box(t, j) ? 1 : 0); }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int topo_head_w7(const Topo& t, int j) { return topo_act_w7(t, j) << (topo_act_box(t, j) ? 1 : 0); }
// a Box agent whose action is tanh of its sample (MDP_SQUASH_TANH)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool topo_act_squash(const Topo& t, int j) { return ((t.act_w4 >> (4 * j)) & 12u) == 12u; }
inline void topo_set_act_squash(Topo& t, int j, bool on) {  // (a Box agent only)
  t.act_w4 = (t.act_w4 & ~(4u << (4 * j))) | ((on ? 4u : 0u) << (4 * j));
}
// some agent is squashed: the launchers then pick the kernels that know the squash
inline bool topo_any_squash(const Topo& t) {
  for (int j = 0; j < t.n; ++j)
    if (topo_act_squash(t, j)) return true;
  return false;
}
// (clears the squash: a Box width is at most 2)
inline void topo_set_act_space(Topo& t, int j, bool box, int w) {
  t.act_w4 = (t.act_w4 & ~(15u << (4 * j))) | (((uint32_t)w | (box ? 8u : 0u)) << (4 * j));
}
inline void topo_set_act_w(Topo& t, int j, int w) { topo_set_act_space(t, j, false, w); }
inline bool topo_any_box(const Topo& t) {
  for (int j = 0; j < t.n; ++j)
    if (topo_act_box(t, j)) return true;
  return false;
}

// MPE entity table for the device env (multiagent/core.py Entity/Agent fields)
struct EnvDesc {
  int scenario, n_agents, n_landmarks, n_adv, max_ep_len;
  float size[MDP_MAX_ENT];
  float accel[MDP_MAX_AGENTS];       // sensitivity (5.0 when agent.accel is None)
  float max_speed[MDP_MAX_ENT];      // <0: None
  int collide[MDP_MAX_ENT];
  int movable[MDP_MAX_ENT];
  int adversary[MDP_MAX_AGENTS];
};
// communication (core.py world.dim_c, agent.silent): 0 when every agent of the
// scenario is silent (no comm state in the arena); a speaking agent's state.c
// is its action vector of the step (environment._set_action, no c noise).
// Only simple_speaker_listener speaks: dim_c 3, agent 0 the speaker.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int env_dim_c(int scenario) { return scenario == MDP_SCN_SPEAKER_LISTENER ? 3 : 0; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool env_silent(int scenario, int agent) { return !(scenario == MDP_SCN_SPEAKER_LISTENER && agent == 0); }

// device control block (one per handle, in the arena)
struct Ctl {
  uint32_t mt[624];
  int32_t mt_pos;
  int32_t pad0;
  int64_t len;          // replay rows valid
  int64_t next;         // ring head
  int64_t env_steps;    // vector steps taken (RNG counter for rollouts)
  int64_t episodes;     // finished episodes logged
  uint32_t ticket[8];   // last-workgroup tickets
  uint32_t upd_ctr;     // RNG counter for training noise
  uint32_t fault;       // set by a bounded spin that timed out (1 norm handshake, 2 xGMI exchange)
  uint32_t xstep[16];   // xGMI exchanges completed per net (2 * agent + net): the epoch counter
  uint32_t ep_pending;  // episodes finished in the running rollout (the last workgroup folds it in)
  uint32_t pad1;
  // xGMI exchange diagnostics (mdp_dp_exchange_stats): per chunk workgroup,
  // the s_memrealtime ticks (100 MHz) from its own chunk's stores to the
  // arrival of every peer's chunk -- peer skew + fabric latency
  uint64_t xw_ticks;    // summed over chunk exchanges
  uint64_t xw_count;    // chunk exchanges counted
  uint64_t xw_max;      // the longest single wait
  uint32_t nonfinite;   // mdp_check_finite's count of non-finite parameters / Adam state
  uint32_t pad2;
};
