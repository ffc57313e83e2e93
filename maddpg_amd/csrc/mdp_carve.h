// mdp_carve.h -- the dynamic-LDS layout of every kernel, written once.
//
// A kernel lays its buffers out behind one another in the workgroup's dynamic
// LDS (LdsCarve, mdp_device.h); the host sizes the launch (lds_*_bytes,
// mdp_kernels.h).  Both expand the SAME list: one X(type, name, words) entry per
// buffer, in carve order.  The kernel supplies X = MDP_CARVE_DECL (the pointer
// declarations) or MDP_CARVE_SET (a tail behind an `if constexpr`, its pointers
// declared null before it); the host supplies X = MDP_CARVE_WORDS (a sum).
// Every buffer starts 16-B aligned: its word count is rounded up to 4 (mdp_r4).
// A count that depends on a kernel-local is a list parameter; the host passes
// the same quantity computed from the Topo.  DESIGN 23.
#pragma once
#include "mdp_topo.h"

#if defined(__HIPCC__)
#define MDP_HD __host__ __device__
#else
#define MDP_HD
#endif

#define MDP_NW 4     // waves per workgroup (rollout / eval kernels)
#define MDP_R 16     // batch rows per workgroup tile
#define MDP_RLH 68   // register-resident path: LDS row stride of forward activations (4r + kq: 64 distinct banks)
#define MDP_RLD 65   // ... of backward deltas (r + 16 kq + s: 64 distinct banks)

MDP_HD inline int mdp_r4(int n) { return (n + 3) & ~3; }
// odd leading dimension so the 16 row-reads of one fragment land on distinct banks
MDP_HD inline int lds_ld(int cols) { return (cols | 1); }

// ---- mdp_grads.hip (S = MDP_R * (H + 1): one activation slot)
// critic_body; G: target actors run concurrently per pass
#define MDP_CARVE_CRITIC(X, ldr, ldc, S, G)                                                        \
  X(float, rowbuf, MDP_R * (ldr))                                                                  \
  X(float, xt, MDP_R * (ldc))                                                                      \
  X(float, xl, MDP_R * (ldc))                                                                      \
  X(float, hA, ((G) + 1) * (S))                                                                    \
  X(float, hB, ((G) + 1) * (S))                                                                    \
  X(float, lg, ((G) + 1) * MDP_R * 8)                                                              \
  X(float, dq, MDP_R)                                                                              \
  X(int, cnt, MDP_MAX_AGENTS + 4) /* layer-1 units done per net, then the work-queue counter (fwd_phase_l12) */
// TWIN tail: the rows' fp32 TD target, kept for critic 2's loss seed
#define MDP_CARVE_TWIN(X) X(float, ys, MDP_R)
// ENT tail (critic_body, A = CriticArgsEnt): log pi of the agent's own target
// sample of the tile's rows, from the sampling lanes to wave 0's TD line
#define MDP_CARVE_ENT(X) X(float, lpt, MDP_R)
// MM tail (critic_body and actor_body): the rows' gradient to every action column
#define MDP_CARVE_MM(X, n_agents) X(float, dxa, MDP_R * MDP_ACT_DIM * (n_agents))
// actor_body
#define MDP_CARVE_ACTOR(X, ldr, ldc, S, H)                                                         \
  X(float, rowbuf, MDP_R * (ldr))                                                                  \
  X(float, x, MDP_R * (ldc))                                                                       \
  X(float, h1a, S)                                                                                 \
  X(float, h2a, S)                                                                                 \
  X(float, h1c, S)                                                                                 \
  X(float, h2c, S)                                                                                 \
  X(float, d2, S)                                                                                  \
  X(float, d1, S)                                                                                  \
  X(float, lg, MDP_R * 8)                                                                          \
  X(float, av, MDP_R * 8)                                                                          \
  X(float, da, MDP_R * 8)                                                                          \
  X(float, dl, MDP_R * 8)                                                                          \
  X(float, qv, MDP_R * 8)                                                                          \
  X(float, w1ai, MDP_ACT_DIM * (H)) /* the critic's layer-1 rows of the a_i input (for da) */
// k_approx_grad: the rows' obs_j, four activation slots, logits, act_j and the seed
#define MDP_CARVE_APPROX(X, ldo, S)                                                                \
  X(float, xo, MDP_R * (ldo))                                                                      \
  X(float, h1, S)                                                                                  \
  X(float, h2, S)                                                                                  \
  X(float, d2, S)                                                                                  \
  X(float, d1, S)                                                                                  \
  X(float, lg, MDP_R * 8)                                                                          \
  X(float, av, MDP_R * 8)                                                                          \
  X(float, dl, MDP_R * 8)

// ---- mdp_grads_r.hip (register-resident, H = 64); ldA = lds_ld(MDP_ACT_DIM * actions in the critic input)
// actor_pre_tile (extra workgroups of k_critic_grad_r)
#define MDP_CARVE_ACTOR_PRE(X, ldr)                                                                \
  X(float, rowbuf, MDP_R * (ldr))                                                                  \
  X(float, h1a, MDP_R * MDP_RLH)                                                                   \
  X(float, h2a, MDP_R * MDP_RLH)                                                                   \
  X(float, lg, MDP_R * 8)                                                                          \
  X(float, av, MDP_R * 8)
// critic_pre_tile (extra workgroups of k_actor_grad_r)
#define MDP_CARVE_CRITIC_PRE(X, ldr, ldA)                                                          \
  X(float, rowbuf, MDP_R * (ldr))                                                                  \
  X(float, xa, MDP_R * (ldA))                                                                      \
  X(float, lg, 3 * MDP_R * 8)                                                                      \
  X(float, h1a, 3 * MDP_R * MDP_RLH)                                                               \
  X(float, h2a, 3 * MDP_R * MDP_RLH)                                                               \
  X(float, h1c, MDP_R * MDP_RLH)                                                                   \
  X(float, h2c, MDP_R * MDP_RLH)
// k_critic_grad_r
#define MDP_CARVE_CRITIC_R(X, ldr, ldA)                                                            \
  X(float, rowbuf, MDP_R * (ldr))                                                                  \
  X(float, xa, MDP_R * (ldA))                                                                      \
  X(float, lg, 3 * MDP_R * 8)                                                                      \
  X(float, h1a, 3 * MDP_R * MDP_RLH)                                                               \
  X(float, h2a, 3 * MDP_R * MDP_RLH)                                                               \
  X(float, h1c, MDP_R * MDP_RLH)                                                                   \
  X(float, h2c, MDP_R * MDP_RLH)                                                                   \
  X(float, h1t, MDP_R * MDP_RLH)                                                                   \
  X(float, h2t, MDP_R * MDP_RLH)                                                                   \
  X(float, qv, MDP_R)                                                                              \
  X(float, qn, MDP_R)                                                                              \
  X(float, dq, MDP_R)                                                                              \
  X(float, d2, MDP_R * MDP_RLD)                                                                    \
  X(float, d1, MDP_R * MDP_RLD)
// k_actor_grad_r
#define MDP_CARVE_ACTOR_R(X, ldr)                                                                  \
  X(float, rowbuf, MDP_R * (ldr))                                                                  \
  X(float, av, MDP_R * 8)                                                                          \
  X(float, lg, MDP_R * 8)                                                                          \
  X(float, da, MDP_R * 8)                                                                          \
  X(float, dl, MDP_R * 8)                                                                          \
  X(float, qv, MDP_R)                                                                              \
  X(float, h1a, MDP_R * MDP_RLH)                                                                   \
  X(float, h2a, MDP_R * MDP_RLH)                                                                   \
  X(float, h1c, MDP_R * MDP_RLH)                                                                   \
  X(float, d2c, MDP_R * MDP_RLD)                                                                   \
  X(float, d1c, MDP_R * MDP_RLD)                                                                   \
  X(float, d2a, MDP_R * MDP_RLD)                                                                   \
  X(float, d1a, MDP_R * MDP_RLD)                                                                   \
  X(float, l1part, 2 * 64 * 16)             /* critic L1 partial accumulators of waves 2, 3 */      \
  X(float, gwpart, 4 * MDP_ACT_DIM * 64)    /* dW3a partials of the four row quarters */            \
  X(float, qpart, 4 * MDP_R)                /* critic head partials of the four L2 column tiles */

// ---- mdp_kernels.hip
// k_rollout's per-agent forward slots: at H = 64 every agent's policy forward
// runs on its own wave (rollout_par), h1 | h2 | logits per wave
#define MDP_ROLLOUT_PAR_W(H) ((H) == 64 ? MDP_NW * (2 * MDP_R * MDP_RLH + MDP_R * 8) : 0)
// k_rollout and k_eval_episodes
#define MDP_CARVE_ROLLOUT(X, ldr, ldh, par_w)                                                      \
  X(float, rowt, MDP_R * (ldr))                                                                    \
  X(float, h1, MDP_R * (ldh))                                                                      \
  X(float, h2, MDP_R * (ldh))                                                                      \
  X(float, lg, MDP_R * 8)                                                                          \
  X(float, hpar, par_w)                                                                            \
  X(float, sp, MDP_R * 2 * MDP_MAX_ENT)                                                            \
  X(float, sv, MDP_R * 2 * MDP_MAX_ENT)                                                            \
  X(float, sfo, MDP_R * 3 * MDP_MAX_ENT)    /* per-env force scratch of env_physics */              \
  X(float, epr, MDP_R * MDP_MAX_AGENTS)     /* the envs' running episode rewards / returns */       \
  X(int, sgoal, MDP_R)                      /* the envs' goal landmarks */
// k_eval_episodes<H, EvalMuArgs> tail: the matchup's table row
#define MDP_CARVE_EVAL_MU(X) X(int, stab, MDP_MAX_AGENTS)
// k_eval_episodes<H, EvalQArgs> tail, taken only when some agent is local_q: the
// [obs_j | act_j] staging tile of those agents' critics, ldq = lds_ld(widest such input)
#define MDP_CARVE_EVAL_QV(X, ldq) X(float, qx, MDP_R * (ldq))
// k_mlp_eval
#define MDP_CARVE_MLP_EVAL(X, ldx, ldh)                                                            \
  X(float, x, MDP_R * (ldx))                                                                       \
  X(float, h1, MDP_R * (ldh))                                                                      \
  X(float, h2, MDP_R * (ldh))                                                                      \
  X(float, lg, MDP_R * 8)

// host side: `words` += the list's size (every buffer is 4-byte words)
#define MDP_CARVE_WORDS(type, name, count)                    \
  static_assert(sizeof(type) == 4, "LDS buffers are words"); \
  words += mdp_r4(count);
