/*
 * maddpg_hip.h -- C ABI of libmaddpg_hip.so, the MI355X-native MADDPG hot path.
 *
 * The reference (adolfogonzalez3/maddpg) is pure Python over TensorFlow 1.x;
 * its "plugin" boundary for this path is the Python surface of
 *   maddpg/__init__.py:1-15               AgentTrainer
 *   maddpg/trainer/maddpg.py:112-196      MADDPGAgentTrainer(action/experience/preupdate/update)
 *   maddpg/trainer/replay_buffer.py:5-85  ReplayBuffer(add/make_index/sample_index/__len__)
 *   experiments/train.py:78-189           the training loop (env step + updates)
 * There is no reference FFI; the binding a maintainer adds is the ctypes stub
 * in maddpg_amd/_lib.py (shown in INTEGRATION.md).  Each entry point below
 * names the reference call it replaces.
 *
 * Conventions
 *  - All compute state lives in ONE device arena the caller allocates (a
 *    PyTorch uint8 CUDA tensor in practice) of mdp_arena_bytes() bytes.  The
 *    library's one device allocation of its own is the direct xGMI exchange
 *    buffer (mdp_dp_xgmi_open: hipExtMallocWithFlags, uncached, IPC-exported,
 *    [2 slots][world][params + probe] 64-bit words; freed by
 *    mdp_dp_xgmi_close / mdp_destroy); mdp_eval_initial_state stages its
 *    result, and mdp_evaluate_matchups its table, through a temporary device
 *    buffer that it frees before returning.
 *  - "_dev" pointers are device pointers on the handle's device; "_host"
 *    pointers are host memory.  Device-pointer calls are asynchronous on the
 *    handle's stream unless stated; host-pointer calls synchronise.  Every
 *    non-NULL "_dev" argument (and mdp_create's arena) is checked at entry
 *    with hipPointerGetAttributes / hipMemGetAddressRange: host memory
 *    (malloc, the stack, pinned hipHostMalloc), another device's memory or an
 *    allocation shorter than the call reads or writes returns < 0 with a
 *    message, before anything is launched.
 *  - Return 0 on success, 1 for "skipped" (update gates), <0 on error; the
 *    message is in mdp_last_error(h).  No C++ exception crosses the ABI.
 *  - One handle per GPU process; calls on one handle are not thread-safe.
 */
#ifndef MADDPG_HIP_H
#define MADDPG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDP_MAX_AGENTS 8
#define MDP_ACT_DIM 5          /* MPE Discrete(dim_p*2+1) action spaces; the widest (mdp_set_act_dims) */
#define MDP_MAX_UNITS 256      /* largest --num-units (train.py:24) */
/* Besides these bounds, a configuration must fit the kernels' LDS envelope (a
   16-row tile of every launch in a CU's 160 KB: the sum of obs dims up to
   ~530 / ~470 / ~270 at 64 / 128 / 256 units); mdp_arena_bytes returns -1 and
   mdp_create's handle carries the reason otherwise. */
#define MDP_ABI_VERSION 5

enum mdp_scenario {
    MDP_SCN_NONE = 0,          /* trainer only (no device env) */
    MDP_SCN_SIMPLE = 1,
    MDP_SCN_SPREAD = 2,
    MDP_SCN_ADVERSARY = 3,
    MDP_SCN_TAG = 4,
    MDP_SCN_SPEAKER_LISTENER = 5  /* simple_speaker_listener: Discrete(3) speaker, Discrete(5) listener */
};

/* which parameter set of one agent (mdp_set_params / mdp_get_params) */
enum mdp_which {
    MDP_ACTOR = 0, MDP_CRITIC = 1, MDP_TGT_ACTOR = 2, MDP_TGT_CRITIC = 3,
    MDP_M_ACTOR = 4, MDP_V_ACTOR = 5, MDP_M_CRITIC = 6, MDP_V_CRITIC = 7,
    MDP_G_ACTOR = 8, MDP_G_CRITIC = 9,
    /* MATD3 (mdp_td3_enable): the second critic's sets, in the TD3 buffer; shapes and pad rules are the critic's */
    MDP_CRITIC2 = 10, MDP_TGT_CRITIC2 = 11, MDP_M_CRITIC2 = 12, MDP_V_CRITIC2 = 13, MDP_G_CRITIC2 = 14
};

/* arena regions (mdp_region) */
enum mdp_region_id {
    MDP_R_THETA = 0, MDP_R_TARGET = 1, MDP_R_ADAM_M = 2, MDP_R_ADAM_V = 3,
    MDP_R_GRAD = 4, MDP_R_REPLAY = 5, MDP_R_INDEX = 6, MDP_R_STATS = 7,
    MDP_R_ENV = 8, MDP_R_EPLOG = 9, MDP_R_BETA = 10, MDP_R_SLAB = 11,
    MDP_R_CTL = 12, MDP_R_COUNT = 13
};

typedef struct mdp_config {
    int32_t n_agents;                 /* env.n (train.py:83) */
    int32_t obs_dim[MDP_MAX_AGENTS];  /* obs_shape_n (maddpg.py:113) */
    int32_t local_q[MDP_MAX_AGENTS];  /* local_q_func = ddpg (train.py:67-74) */
    int32_t act_dim;                  /* must be MDP_ACT_DIM */
    int32_t num_units;                /* --num-units, 1..MDP_MAX_UNITS (train.py:24) */
    int32_t batch_size;               /* --batch-size */
    int32_t max_episode_len;          /* --max-episode-len */
    int64_t capacity;                 /* ReplayBuffer(1e6) (maddpg.py:147) */
    int32_t num_envs;                 /* vector env copies on this rank (0: no env) */
    int32_t scenario;                 /* enum mdp_scenario */
    int32_t num_adversaries;          /* simple_tag / simple_adversary split */
    int32_t world_size, rank;         /* data-parallel group (grads scaled by 1/world) */
    float lr;                         /* --lr (Adam) */
    float tau;                        /* Polyak 1e-2 (maddpg.py:21) */
    float grad_clip;                  /* 0.5 (maddpg.py:130,142) */
    float actor_reg;                  /* 1e-3 (maddpg.py:56) */
    float adam_b1, adam_b2, adam_eps; /* TF1 AdamOptimizer defaults */
    double gamma;                     /* --gamma (TD target in fp64, maddpg.py:186) */
    uint64_t seed;                    /* device Philox key (Gumbel noise, env resets) */
    int32_t episode_log_rows;         /* finished-episode log ring (0: max(4096, 4 num_envs));
                                         otherwise >= 2 num_envs (mdp_create fails below);
                                         train.py sizes it save_rate + 2 num_envs */
    int32_t reserved;
} mdp_config;

typedef struct mdp_tensor_info {      /* one fully_connected{,_1,_2}/{weights,biases} */
    int64_t offset;                   /* floats from the start of a param-space region */
    int32_t rows, cols;               /* the TF variable's shape ([in, num_units] ...; mdp_set_act_dims) */
    int32_t dev_rows, dev_cols;       /* its block in the arena: num_units padded to the
                                         kernel width (64/128/256), extra entries zero */
} mdp_tensor_info;

typedef struct mdp_handle mdp_handle;

/* ---- lifecycle ------------------------------------------------------- */
int32_t mdp_abi_version(void);
/* arena size for cfg; fills *param_floats with the param-space length (may be NULL) */
int64_t mdp_arena_bytes(const mdp_config* cfg, int64_t* param_floats);
/* U.initialize() / MADDPGAgentTrainer.__init__ (maddpg.py:113-149): binds the
 * arena, zeroes it, sets Adam beta powers, seeds the index RNG with seed. */
int mdp_create(const mdp_config* cfg, void* arena_dev, int64_t arena_bytes,
               void* hip_stream, mdp_handle** out);
int mdp_destroy(mdp_handle* h);
const char* mdp_last_error(const mdp_handle* h);
void* mdp_stream(mdp_handle* h);
int mdp_synchronize(mdp_handle* h);
/* byte offset + size of a region inside the arena */
int mdp_region(const mdp_handle* h, int32_t region, int64_t* offset, int64_t* bytes);
/* layout of tensor t (0..5 = W1,b1,W2,b2,W3,b3) of agent's actor (net=0) or critic (net=1) */
int mdp_tensor(const mdp_handle* h, int32_t agent, int32_t net, int32_t t, mdp_tensor_info* out);
/* joint replay row layout: offsets (floats) of agent's obs/act/obs_next/rew/done, row stride */
int mdp_row_layout(const mdp_handle* h, int32_t agent, int32_t out6[6]);
/* Per-agent action widths: agent i has a Discrete(dims[i]) space, 1 <= dims[i] <=
 * MDP_ACT_DIM (make_pdtype(act_space) per agent, maddpg.py:31,39; distributions.py:
 * 413-415).  Default: MDP_ACT_DIM for every agent.  No device layout changes: the
 * replay row's action slot, the critic-input columns, the actor's W3 / b3 block and
 * every [.][MDP_ACT_DIM] action / noise array of this ABI stay MDP_ACT_DIM wide.
 * Agent i uses the first dims[i] entries of its slot; the Gumbel-softmax runs over
 * those only and writes exactly 0 to the pad entries, pad uniforms are never used,
 * and pad parameters, targets, Adam slots and gradients stay exactly 0.  The
 * logical shapes (mdp_tensor rows / cols, mdp_set_params / mdp_get_params) are the
 * reference's: actor W3 [num_units, A_i], b3 [A_i]; critic W1 [sum_obs + sum_j A_j,
 * num_units] (DDPG critic [obs_i + A_i, num_units]) -- the device block of that W1
 * has interior pad rows, which are written as zero and never returned.  Rows given
 * to mdp_buffer_add_rows / mdp_buffer_put_agent and actions given to mdp_env_step
 * must hold zeros in the pad entries.
 * Accepted only before the handle's first parameter write, act, update or env
 * call; on a handle with a device scenario the widths must equal the scenario's
 * own (such a handle needs no call).  < 0 with a message otherwise. */
int mdp_set_act_dims(mdp_handle* h, const int32_t dims[MDP_MAX_AGENTS]);
/* the widths in use (0 beyond n_agents) */
int mdp_get_act_dims(const mdp_handle* h, int32_t dims[MDP_MAX_AGENTS]);
/* Per-agent action spaces, kinds beside widths (make_pdtype, distributions.py:
 * 408-422): agent i is Discrete(dims[i]), 1 <= dims[i] <= MDP_ACT_DIM, or
 * Box(dims[i]), dims[i] in {1, 2}: a diagonal-Gaussian policy whose head is
 * flat = [mean (d) | logstd (d)] and whose sample is a = mean + exp(logstd) * eps
 * (distributions.py:343-371; no clamp on logstd).  eps is Box-Muller on the first
 * two uniforms of the agent's [5] noise slot: r = sqrt(-2 ln(1 - u0)), eps_0 =
 * r cos(2 pi u1), eps_1 = r sin(2 pi u1); u[2..4] are never read and every
 * [.][MDP_ACT_DIM] array of this ABI keeps its shape.  No device layout changes:
 * the head fills the first 2 d columns of the W3 / b3 block, the action the first d
 * entries of its slot, and everything beyond is exactly 0, as for a narrow Discrete
 * agent.  Logical shapes: actor W3 [num_units, 2 d], b3 [2 d]; a critic W1 counts d
 * rows for the agent's action.  mdp_actor_logits returns flat; MDP_EVAL_MEAN plays
 * the mean.  On a handle with a device scenario an agent keeps the scenario's own
 * Discrete space or, if it moves and does not speak, becomes Box(2), whose action is
 * the force (a[0], a[1]) * accel, unclipped; anything else is refused.
 * A handle with a Box agent trains in strict mode on one GPU, on the general
 * gradient kernels (mdp_grad_variant 0); prioritized replay, MATD3, M3DDPG,
 * inferred policies, throughput mode and data parallelism refuse it with a message.
 * Accepted when mdp_set_act_dims is (and before any of the enables above).  < 0
 * with a message for an unknown kind or a width outside the kind's range. */
#define MDP_ACT_DISCRETE 0
#define MDP_ACT_BOX 1
int mdp_set_act_spaces(mdp_handle* h, const int32_t kinds[MDP_MAX_AGENTS], const int32_t dims[MDP_MAX_AGENTS]);
/* the kinds and widths in use (0 beyond n_agents); either pointer may be NULL */
int mdp_get_act_spaces(const mdp_handle* h, int32_t kinds[MDP_MAX_AGENTS], int32_t dims[MDP_MAX_AGENTS]);
/* A Box agent's squash: MDP_SQUASH_NONE, the policy above, or MDP_SQUASH_TANH, a
 * bounded action.  The sample z = mean + exp(logstd) * eps is formed as above and the
 * action is a_k = tanhf(z_k), inside [-1, 1]: what the agent plays, what replay
 * stores and what the critics see.  The backward through the sample is dz_k =
 * da_k * (1 - a_k * a_k), dmean_k = dz_k, dlogstd_k = dz_k * std_k * eps_k; the head,
 * its width, the noise and the regulariser mean(square(flat)) are unchanged, and so
 * is every layout.  MDP_EVAL_MEAN plays tanh(mean).  The bounds are fixed at
 * [-1, 1]; a device scenario takes a * accel as the force, the magnitude a
 * Discrete(5) agent can reach.  No clamp on logstd.
 * squash[i] is one of the two values for each of the n_agents agents; a non-zero
 * entry for a Discrete agent, an unknown value and a null pointer are refused with
 * a message.  Accepted when mdp_set_act_spaces is, after it: mdp_set_act_spaces and
 * mdp_set_act_dims reset every squash to none.  A squashed handle is a Box handle in
 * everything else (mdp_get_act_spaces says MDP_ACT_BOX; the same refusals). */
#define MDP_SQUASH_NONE 0
#define MDP_SQUASH_TANH 1
int mdp_set_act_squash(mdp_handle* h, const int32_t squash[MDP_MAX_AGENTS]);
/* the squashes in use (0 beyond n_agents and for a Discrete agent) */
int mdp_get_act_squash(const mdp_handle* h, int32_t squash[MDP_MAX_AGENTS]);
/* A Box agent's entropy coefficient: soft MADDPG.  Agent i, Box(d), plain or
 * tanh-squashed, with alpha_i > 0 maximises its reward plus alpha_i times its own
 * policy's entropy.  Sampling does not change.  For a sample with noise eps,
 * pre-squash value z_k = mean_k + exp(logstd_k) * eps_k and action a_k (formed as
 * above), its log-probability, in float, every product and sum rounded on its own
 * (no fma), expf / log1pf libm's precise forms, in this order:
 *   g_k = ((-0.5f * (eps_k * eps_k)) - logstd_k) - 0.5 ln(2 pi)
 *   squashed:  w = |z_k|;  g_k = g_k - 2.0f * ((ln 2 - w) - log1pf(expf(-2.0f * w)))
 *   lp = g_0                 (d = 1)
 *   lp = g_0 + g_1           (d = 2)
 * The squash term is ln(1 - tanh^2 z_k), finite at every finite z (also where the
 * float action is exactly +-1).
 * Critic step of agent i (MADDPG or DDPG critic): lp' = the log-probability of
 * agent i's OWN target-actor sample at o'_i, the sample the step draws anyway;
 * qs = q' - alpha_i * lp' in float (product, then difference), and the TD line runs
 * with it: y = r + gamma (1 - done) (double)qs.  No other agent's entropy enters.
 * mdp_get_stats' mean target q is the mean of qs.
 * Actor step of agent i: the loss gains alpha_i * mean_b(lp_b) of the fresh own
 * sample, and the gradient goes through the reparameterised sample at fixed eps.
 * With ab = alpha_i / B (float division), per row and k < d, added (one rounded add)
 * to the backward's dmean_k / dlogstd_k after the regulariser:
 *   plain:     dlogstd_k += -ab                      (dmean_k gains nothing)
 *   squashed:  dmean_k += ab * (2.0f * a_k)
 *              dlogstd_k += ab * ((2.0f * a_k) * se_k - 1.0f),  se_k = std_k * eps_k
 * p_loss (mdp_get_stats [1]) includes alpha_i * mean_b(lp_b).  With alpha_i = 0 agent
 * i's update is what it is without the call, bit for bit; MDP_EVAL_MEAN, the
 * evaluation calls, mdp_act and replay do not change.  The next action comes from
 * the TARGET actor, the critic is single and alpha is fixed.
 * alpha[i] >= 0 and finite for each of the n_agents agents; a negative or
 * non-finite entry and a non-zero entry for a Discrete agent are refused with a
 * message that names the call and the agent, a null pointer with one that names
 * the call.  Accepted when mdp_set_act_squash is;
 * mdp_set_act_spaces and mdp_set_act_dims reset every coefficient to 0. */
int mdp_set_act_entropy(mdp_handle* h, const float* alpha /* [n_agents] */);
/* the coefficients in use, alpha[n_agents] */
int mdp_get_act_entropy(const mdp_handle* h, float* alpha);
/* out = {alpha, mean lp of the agent's last actor step, mean lp' of its last critic
 * step, 0} (0 before the first, and for an agent whose coefficient is 0); waits for
 * the stream.  Refused on a handle on which no agent has a coefficient. */
int mdp_entropy_info(mdp_handle* h, int32_t agent, double out[4]);

/* ---- parameters (golden injection, checkpoint; tf_util.py:259-273) --- */
int mdp_set_params(mdp_handle* h, int32_t agent, int32_t which, const float* src_host, int64_t n);
int mdp_get_params(mdp_handle* h, int32_t agent, int32_t which, float* dst_host, int64_t n);
/* beta1^t, beta2^t of agent's actor (net=0) / critic (net=1) Adam */
int mdp_get_beta_powers(mdp_handle* h, int32_t agent, int32_t net, float out2[2]);
int mdp_set_beta_powers(mdp_handle* h, int32_t agent, int32_t net, const float in2[2]);

/* ---- replay buffer (replay_buffer.py) -------------------------------- */
int64_t mdp_buffer_len(mdp_handle* h);                     /* __len__ :18-19 */
/* add `rows` whole joint rows [rows][row_stride] (device) at the ring head (:25-32) */
int mdp_buffer_add_rows(mdp_handle* h, const float* rows_dev, int64_t rows);
/* write agent's columns of arbitrary ring positions (per-agent add of the facade) */
int mdp_buffer_put_agent(mdp_handle* h, int32_t agent, const int64_t* pos_dev,
                         const float* cols_dev, int64_t rows);
/* host-tracked ring state after put_agent (len/next are per agent in the reference) */
int mdp_buffer_set_len(mdp_handle* h, int64_t len, int64_t next_idx);
/* the same with the count of rows the host ever added to the ring (monotone).
 * Prioritized replay resets the priorities of exactly the rows added since the
 * previous call, however often the ring wrapped meanwhile; mdp_buffer_set_len
 * can only infer them from the move of the head (fewer than `capacity` rows
 * between two calls).  Without prioritized replay it is mdp_buffer_set_len. */
int mdp_buffer_set_ring(mdp_handle* h, int64_t len, int64_t next_idx, int64_t rows_total);
/* random.seed(seed) on the device MT19937 (CPython init_by_array) */
int mdp_seed_py_random(mdp_handle* h, uint64_t seed);
/* random.setstate/getstate: 624 words + position (random.getstate()[1]) */
int mdp_set_rng_state(mdp_handle* h, const uint32_t* state625_host);
int mdp_get_rng_state(mdp_handle* h, uint32_t* state625_host);
/* make_index (:46-47): count x randint(0, len-1), bit-exact CPython stream */
int mdp_make_index(mdp_handle* h, int32_t count, int32_t* idx_dev);
/* sample_index (:55-56) fused gather: out[b] = joint row idx[b] */
int mdp_sample_rows(mdp_handle* h, const int32_t* idx_dev, int32_t count, float* out_dev);

/* ---- policies (maddpg.py:151-152, p_debug / q_debug) ------------------ */
/* act[rows][5] = gumbel_softmax(actor_or_target(obs)); u_dev: injected uniforms or NULL */
int mdp_act(mdp_handle* h, int32_t agent, int32_t target, const float* obs_dev,
            float* act_dev, int32_t rows, const float* u_dev);
/* logits[rows][5] = actor_or_target(obs) (p_debug['p_values'], maddpg.py:63) */
int mdp_actor_logits(mdp_handle* h, int32_t agent, int32_t target, const float* obs_dev,
                     float* logits_dev, int32_t rows);
/* q[rows] = critic_or_target(x[rows][cin]) with x already concatenated */
int mdp_q_values(mdp_handle* h, int32_t agent, int32_t target, const float* x_dev,
                 float* q_dev, int32_t rows);

/* ---- training (maddpg.py:161-196) ------------------------------------ */
/* One agent's update past the gates, strict reference order.
 * idx_dev: B indices or NULL (draw from the device MT stream);
 * u_tgt_dev: [n_agents][B][5] uniforms for the target actors or NULL;
 * u_act_dev: [B][5] uniforms for the actor-loss sample or NULL. */
int mdp_update(mdp_handle* h, int32_t agent, const int32_t* idx_dev,
               const float* u_tgt_dev, const float* u_act_dev);
/* gates of maddpg.py:162-165; returns 1 (skip) or 0 (train) */
int mdp_update_gate(mdp_handle* h, int64_t t);
/* MADDPGAgentTrainer.update(agents, t) as one call (maddpg.py:161-196), the
 * signature SURVEY.md 8b sketches: the gates at train step t (1 = skipped,
 * the reference's `return None`, nothing drawn), else the update on idx_dev
 * (B indices, or NULL: drawn from the device MT stream, replay_buffer.py:46-47)
 * with u_dev (NULL, or [n_agents][B][5] target-actor uniforms followed by
 * [B][5] actor-loss uniforms) and the 6 stats [q_loss, p_loss, mean y,
 * mean r, mean Q', std y] in stats_out (synchronous); 0 = trained, <0 error */
int mdp_agent_update(mdp_handle* h, int32_t agent, int64_t t, const int32_t* idx_dev, const float* u_dev,
                     double stats_out[6]);
/* update round: all agents in order (train.py:158-161), indices from the MT stream.
 * Replayed from a captured hipGraph after the first round (see mdp_set_graphs). */
int mdp_update_round(mdp_handle* h);
/* enable (default) / disable hipGraph replay of mdp_update_round / mdp_train_step */
int mdp_set_graphs(mdp_handle* h, int32_t on);
/* One vector step of the training loop (train.py:110-161 for num_envs env
 * copies): mdp_env_step with the policy's own actions, then `rounds` update
 * rounds (the rounds the update cadence makes due; 0..64).  Replayed as ONE
 * hipGraph per distinct `rounds` (per-round graph launches leave the GPU idle
 * between rounds).  Single-GPU path; data-parallel ranks use the phase entry
 * points below with an all-reduce between them. */
int mdp_train_step(mdp_handle* h, int32_t rounds);
/* n consecutive training steps (rounds[i] update rounds after step i's
 * rollout, exactly as n mdp_train_step calls) replayed as ONE graph, keyed
 * by the round counts: saves the graph-launch boundary between steps.  A step
 * with 0 rounds is its rollout launch alone inside the graph (a stretch of
 * them one k_rollout launch of that many steps when num_envs <= 16); before the first
 * (eager) training step, with profiling or eager collectives the steps run
 * one by one.  launch = 0:
 * only capture and instantiate the graph (nothing runs), so a timed region
 * replays graphs made ahead of it. */
int mdp_train_steps(mdp_handle* h, int32_t n, const int32_t* rounds, int32_t launch);

/* ---- native data parallelism (one process per GPU, RCCL over xGMI) ------
 * Replaces the reference's single-process update (maddpg.py:161-196) on G
 * ranks: each rank owns its env copies / replay shard / index stream; every
 * optimizer phase sums the reduced gradient with one ncclAllReduce on the
 * engine stream and applies it x 1/G (SURVEY §8e strict mode).  Rank 0 makes
 * the id, the caller broadcasts it (e.g. torch.distributed), every rank calls
 * mdp_dp_init; afterwards mdp_update / mdp_update_round / mdp_train_step run
 * the data-parallel update (collectives launched eagerly; MDP_DP_GRAPHS=1 in
 * the environment captures them in the step graph). RCCL is dlopen'ed. */
int mdp_dp_unique_id(uint8_t* out128);
int mdp_dp_init(mdp_handle* h, const uint8_t* id128, int32_t world, int32_t rank);

/* ---- direct xGMI gradient exchange (alternative to mdp_dp_init) ---------
 * Same semantics as the RCCL path (sum over ranks in rank order, x 1/G, every
 * replica bit-identical), but the exchange runs INSIDE the fused optimizer
 * kernel: each 256-parameter chunk workgroup stores its reduced chunk straight
 * into every peer's IPC-mapped buffer over xGMI, raises a per-chunk flag and
 * sums the world's chunks -- no collective launch, so a data-parallel update
 * has the single-GPU launch count (4 per agent strict, 3 per round
 * throughput).  Handshake (every rank, in order):
 *   open(world, rank) -> its 64-byte IPC handle; the caller all-gathers the
 *   handles; connect(handles[world][64]); probe() exchanges a known pattern
 *   (0 = every value arrived; fails after 30 s without a peer); the caller
 *   agrees on success across ranks, then enable() -- or close() everywhere and
 *   fall back to mdp_dp_init.  world 2..8. */
#define MDP_XGMI_HANDLE_BYTES 64
int mdp_dp_xgmi_open(mdp_handle* h, int32_t world, int32_t rank, uint8_t* handle_out);
int mdp_dp_xgmi_connect(mdp_handle* h, const uint8_t* handles);
int mdp_dp_xgmi_probe(mdp_handle* h, int32_t* mismatches);
int mdp_dp_xgmi_enable(mdp_handle* h);
int mdp_dp_xgmi_close(mdp_handle* h);
/* what this rank's data parallelism is wired to: out4 = {kind (0 none, 1 RCCL,
 * 2 direct xGMI), ranks in the communicator (ncclCommCount / exchange world),
 * this rank, peers reached (RCCL: ranks - 1; xGMI: peer buffers mapped)} */
int mdp_dp_info(mdp_handle* h, int32_t out4[4]);
/* what the direct xGMI exchange cost this rank (in-kernel s_memrealtime stamps
 * of k_reduce_apply's chunk workgroups: from a chunk's own stores to the
 * arrival of every peer's copy -- peer skew plus fabric latency): out4 =
 * {chunk exchanges counted, mean wait us, longest wait us, total wait us}
 * since the last reset; reset != 0 zeroes the counters.  The RCCL path's cost
 * is event-timed instead (mdp_prof_enable(MDP_K_ALLREDUCE)). */
int mdp_dp_exchange_stats(mdp_handle* h, double out4[4], int32_t reset);
/* collect those stamps (on != 0) in the optimizer launches issued from now on
 * while enabled -- eager launches and graphs captured meanwhile; graphs
 * captured with it off carry no stamping code path (default off: the three
 * counter atomics per chunk stay out of the exchange's critical path) */
int mdp_dp_exchange_stats_enable(mdp_handle* h, int32_t on);
/* Co-residency plan of the spin-waiting optimizer launch (k_reduce_apply: the
 * chunk workgroups of a tensor wait for each other's norm partials, the xGMI
 * exchange for the peers' chunks).  For cfg on a device with `cus` CUs that
 * hold `per_cu` of its 1024-thread workgroups each, out[2 agent + net] = the
 * launch's grid when the one-launch step is used (grid <= cus x per_cu), or
 * -grid when that net falls back to k_reduce + k_apply (no spin).  Returns the
 * number of nets that fall back, < 0 for an invalid cfg.  Needs no GPU. */
int mdp_ra_plan(const mdp_config* cfg, int32_t cus, int32_t per_cu, int32_t* out);
/* phase entry points for data parallelism (grad -> all-reduce -> apply) */
int mdp_critic_grad(mdp_handle* h, int32_t agent, const int32_t* idx_dev, const float* u_tgt_dev);
int mdp_actor_grad(mdp_handle* h, int32_t agent, const int32_t* idx_dev, const float* u_act_dev);
/* reduce the per-workgroup partials of net (0 actor, 1 critic) into MDP_R_GRAD */
int mdp_reduce_grad(mdp_handle* h, int32_t agent, int32_t net);
/* clip + Adam (+ Polyak of both nets when net==0) reading MDP_R_GRAD scaled by `scale` */
int mdp_apply_grad(mdp_handle* h, int32_t agent, int32_t net, float scale);
/* the 6 values update() returns (maddpg.py:196), fp64, synchronises */
int mdp_get_stats(mdp_handle* h, int32_t agent, double out6[6]);
/* debug check (the reference's _Function(check_nan), tf_util.py:322,366-368):
 * *nonfinite_out = the number of NaN / Inf values in every parameter set
 * (weights, targets, Adam m and v of every agent; the second critic's after
 * mdp_td3_enable, the approximators' after mdp_approx_enable) and in the agents'
 * update stats; counted on the device, synchronous (ABI 5) */
int mdp_check_finite(mdp_handle* h, int64_t* nonfinite_out);

/* ---- update mode of the round paths (mdp_update_round, mdp_train_step) ----
 * 0 strict (default): the reference's order -- agents in turn, each critic
 *   step before its actor step, later agents' TD targets see the earlier
 *   agents' Polyak-updated target actors (maddpg.py:180-194, train.py:160-161).
 * 1 throughput (opt-in, NOT the reference's semantics): every
 *   agent's critic and actor gradients from the round-start parameters, then
 *   every clip + Adam + Polyak -- 3 launches per round.  With data parallelism
 *   (mdp_dp_init BEFORE this call): gradients, a reduce pass, ONE all-reduce
 *   of the whole gradient region per round, the step pass (x 1/world).  Needs
 *   the fused optimizer step for every net (mdp_create's co-residency plan)
 *   and <= 8 agents; the fast H=64 kernels batch every agent's gradients in
 *   one launch, the general kernels (H=128/256, > 3 target actors) run one
 *   gradient launch per agent and step kind. */
int mdp_set_update_mode(mdp_handle* h, int32_t mode);
/* one throughput-mode round with injected randomness (the parity entry point,
 * like mdp_update): idx_dev [n][B] (NULL: drawn from the index stream),
 * u_tgt_dev [n][n][B][5] (agent, target actor j, row), u_act_dev [n][B][5]
 * (NULL: device Philox noise, counter upd_ctr + agent) */
int mdp_update_all(mdp_handle* h, const int32_t* idx_dev, const float* u_tgt_dev, const float* u_act_dev);

/* ---- device environments (MPE World.step, train.py:104-128) ---------- */
int mdp_env_reset(mdp_handle* h);
/* one vector step: actions from the actors (or act_in_dev [E][n][5]), physics,
 * replay append, episode bookkeeping and resets at max_episode_len.
 * u_dev: injected Gumbel uniforms [E][n][5] or NULL. */
int mdp_env_step(mdp_handle* h, const float* act_in_dev, const float* u_dev);
/* env state: pos/vel [E][n_entities][2] fp32, goal [E] int32, ep_step [E] int32 */
int mdp_env_get_state(mdp_handle* h, float* pos_host, float* vel_host, int32_t* goal_host, int32_t* ep_step_host);
int mdp_env_set_state(mdp_handle* h, const float* pos_host, const float* vel_host, const int32_t* goal_host, const int32_t* ep_step_host);
/* Communication state (core.py agent.state.c) of every agent, [num_envs][n_agents][MDP_ACT_DIM]
 * host floats; synchronises like mdp_env_get_state.  After a step a speaking agent's
 * state.c is its action vector of that step (environment._set_action, no noise), a
 * silent agent's is 0; everything is 0 after a reset.  Of the scenarios only
 * simple_speaker_listener has a speaker (agent 0, Discrete(3); the listener's last 3
 * observations are its state.c): on the others get returns zeros and set is refused.
 * simple_speaker_listener is restated from memory of the upstream MPE source, which
 * is neither vendored by the reference nor present here: its parity is UNPINNED. */
int mdp_env_get_comm(mdp_handle* h, float* comm_host);
int mdp_env_set_comm(mdp_handle* h, const float* comm_host);
int mdp_env_obs(mdp_handle* h, float* obs_dev);   /* current obs [E][sum obs] */
/* --benchmark mode (train.py:139-148): mdp_env_step that also writes every
 * agent's scenario benchmark_data() of the post-physics state (MPE
 * environment._get_info -> info_n['n']) to info_dev [E][n][MDP_BENCH_W] fp32,
 * before the episode reset.  Record per scenario (zero-padded):
 *   simple_spread    (rew_i, collisions_i, sum_l min_a dist, occupied landmarks)
 *   simple_adversary adversary: (|pos - goal|^2); good: (|pos - lm_l|^2 ..., |pos - goal|^2)
 *   simple_tag       adversary: (good agents in contact); good: (0)
 *   simple           has no benchmark_data (the reference's make_env raises): error */
#define MDP_BENCH_W 8
int mdp_env_step_bench(mdp_handle* h, float* info_dev);
/* the same with injected Gumbel uniforms u_dev [E][n][5] (NULL: mdp_env_step_bench) */
int mdp_env_step_bench_u(mdp_handle* h, float* info_dev, const float* u_dev);

/* ---- policy evaluation: whole episodes in one launch --------------------
 * Scores the handle's current actors on evaluation episodes without touching
 * anything training uses.  Episode id g (32 bits) is a pure function of the
 * actor parameters, cfg.seed, the scenario, g and the mode -- not of num_envs,
 * of how ids are split over calls, or of the training env state:
 *   reset     reset_world from Philox stream 0x60000, counter 0, env g (the
 *             slot order of mdp_env_reset); ep_step 0, every state.c 0
 *   step t    0 .. max_episode_len - 1, each mdp_env_step's step: observations
 *             (the speaker's message is its action of step t - 1), every actor's
 *             forward, the actions, World.step, the rewards, the records
 *   actions   MDP_EVAL_SAMPLE: the reference's act (Gumbel-softmax) on uniforms
 *             of stream 0x70000 | agent, counter t, row g, or injected ones;
 *             MDP_EVAL_MEAN: the softmax of the logits without noise (the same
 *             width-aware routine: pad entries exactly 0)
 *   ret       [i][j] agent j's return of id first_episode + i: the fp32 sum of its
 *             step rewards in step order (collaborative scenarios: the shared sum)
 *   bench     [i][j][MDP_BENCH_W] the fp32 sum in step order of the record
 *             mdp_env_step_bench writes; refused where that call is refused
 * It neither reads nor writes the training env state, the replay ring, the
 * episode log, the comm state, any control field (env step / episode counters,
 * tickets, the index RNG, the noise counter) or the prioritized-replay buffer.
 * One workgroup per 16 ids carries them through the whole episode.
 * ids [first_episode, first_episode + episodes): 1 <= episodes <= 2^20, the range inside uint32.
 * u_dev: NULL or [episodes][max_episode_len][n_agents][5] uniforms (SAMPLE only);
 * ret_dev [episodes][n_agents]; bench_dev NULL or [episodes][n_agents][MDP_BENCH_W].
 * Refused with a message before any launch: a bad mode, count or id range, u_dev
 * with MDP_EVAL_MEAN, a call while the handle's stream is capturing a graph. */
enum { MDP_EVAL_SAMPLE = 0, MDP_EVAL_MEAN = 1 };
int mdp_evaluate(mdp_handle* h, int64_t first_episode, int32_t episodes, int32_t mode,
                 const float* u_dev, float* ret_dev, float* bench_dev);
/* ---- critic evaluation: Q against the realised return, in the same launch --
 * Plays mdp_evaluate's episode ids and scores the handle's live (non-target)
 * critics on them: Q_j(o_t, a_t) beside the discounted return the policies then
 * collect -- the overestimation diagnostic (TD3's first figure).  The reference
 * never stores done = 1 for these scenarios (`terminal` only resets the env), so
 * a critic estimates the return of the CONTINUING world: the episode plays a
 * caller-chosen number of steps without reset, and only its leading part is scored.
 *   episode   id g is mdp_evaluate's id: reset stream 0x60000, noise stream
 *             0x70000 | agent with counter t and row g, the same modes, the same
 *             actor forward path.  It plays `steps` steps, 1 <= steps <= 4096,
 *             with no reset and without regard to max_episode_len: for
 *             t < max_episode_len the trajectory is mdp_evaluate's bit for bit,
 *             and a run with more steps reproduces a run with fewer on the
 *             common prefix
 *   C         critics per agent: 1, or 2 after mdp_td3_enable
 *   q         [i][t][j][C] Q_j (then Q2_j, of the TD3 buffer's MDP_CRITIC2) on the
 *             joint [obs_n | act_n] of step t ([obs_j | act_j] for a local_q
 *             agent), after every agent's action of step t and before World.step;
 *             the value mdp_q_values(j, 0, ...) gives on that row, bit for bit
 *   rew       [i][t][j] the step rewards, the values mdp_evaluate's ret sums
 *   g         [i][t][j] the return-to-go in fp64 from cfg.gamma (fp32): G_steps = 0,
 *             G_t = (double)r_t + (double)gamma * G_{t+1}, stored as (float)G_t
 *   gap       [i][j][C] (float)((1 / scored) * sum_{t < scored} ((double)q_t - G_t)),
 *             the sum in fp64 in step order, 1 <= scored <= steps
 * Truncation: G_t lacks the rewards from step `steps` on, i.e. gamma^(steps - t)
 * times a return-to-go; over the scored steps that is at most a factor
 * gamma^(steps - scored + 1) of the return's scale (0.0094 at gamma 0.95,
 * steps - scored = 90).  Nothing is bootstrapped from Q_steps.
 * u_dev: NULL or [episodes][steps][n_agents][5] uniforms (SAMPLE only).
 * Two launches on the handle's stream (the episodes, then one thread per
 * (episode, agent) for g and gap), both timed as MDP_K_EVAL; no synchronisation.
 * It neither reads nor writes the training env state, the replay ring, the
 * episode log, the comm state, any control field (env step / episode counters,
 * tickets, the index RNG, the noise counter), the prioritized-replay buffer or
 * the TD3 counters; of the parameters it reads the actors and the live critics.
 * Refused with a message that names the entry point and the argument, before any
 * launch: a handle without a device env, a bad mode, count, id range, steps or
 * scored, u_dev with MDP_EVAL_MEAN, a NULL q_dev / rew_dev / g_dev / gap_dev, any
 * of the five pointers that is not device memory of the full size, a stream
 * that is capturing a graph.  The handle trains and evaluates on after a refusal. */
int mdp_evaluate_q(mdp_handle* h, int64_t first_episode, int32_t episodes, int32_t mode,
                   int32_t steps, int32_t scored, const float* u_dev,
                   float* q_dev, float* rew_dev, float* g_dev, float* gap_dev);
/* the start states of those ids: pos/vel [episodes][n_entities][2], goal [episodes]
 * (host, synchronises; staged through a temporary device buffer freed before return) */
int mdp_eval_initial_state(mdp_handle* h, int64_t first_episode, int32_t episodes,
                           float* pos_host, float* vel_host, int32_t* goal_host);

/* ---- matchup evaluation: a bank of actor sets scored in one launch --------
 * mdp_evaluate's episodes with the actors taken from a caller-owned bank on
 * the device instead of the handle's parameters: the cross-play table of the
 * MADDPG paper (run A's adversaries against run B's good agents, every A and
 * B), every checkpoint of a run on the same start states, seeds against each
 * other.  The handle's own parameters are neither read nor written, so the
 * calls work in the middle of a training run.
 *   set       mdp_actor_set_floats() floats laid out as the theta region: agent
 *             j's actor tensor t at mdp_tensor(j, 0, t).offset.  Only the actor
 *             spans are ever read; what lies between them is never read.  The
 *             value (the set stride of a bank) is mdp_arena_bytes' param_floats
 *             rounded up to a multiple of 4; -1 on an unusable handle
 *   bank      [n_sets][mdp_actor_set_floats()] floats, 16-byte aligned
 *   table     [matchups][n_agents] int32 on the host: table[m][j] is the set that
 *             agent j's actor comes from in matchup m
 *   episode   id g as mdp_evaluate defines it: the same reset stream, noise
 *             stream, step, ret and bench definitions.  Neither the start state
 *             nor the noise depends on m, so two matchups on the same ids are a
 *             paired comparison on common random numbers
 *   ret       [m][i][j], bench [m][i][j][MDP_BENCH_W]
 *   u_dev     NULL or [episodes][max_episode_len][n_agents][5], shared by every matchup
 * mdp_actor_set_write takes the logical layout and the count of
 * mdp_set_params(agent, MDP_ACTOR, ...) and writes the agent's whole device
 * block (pad entries exact zeros) into set_dev; it touches neither the arena
 * nor the handle's state and synchronises.  mdp_actor_set_snapshot copies every
 * agent's actor span of the handle's current parameters into set_dev, device
 * to device on the handle's stream (refused while the stream captures).
 * mdp_evaluate_matchups checks the whole table on the host, stages it through
 * a temporary device buffer that is freed before return -- so the call
 * SYNCHRONISES the handle's stream, unlike mdp_evaluate -- and plays every
 * (matchup, id) in one launch (grid: 16-id tiles x matchups), timed as
 * MDP_K_EVAL.  Like mdp_evaluate it touches nothing training uses, and it never
 * writes the bank.
 * Bounds: 1 <= n_sets <= 4096, 1 <= matchups <= 4096, episodes and the id range
 * as mdp_evaluate, matchups * episodes <= 2^22.
 * Refused with a message that names the entry point and the argument, before
 * any launch: a handle without a device env, a bad mode, u_dev with
 * MDP_EVAL_MEAN, a NULL table_host / ret_dev / bank_dev, a table entry outside
 * [0, n_sets) (the message gives the matchup and the agent), a bound above, a
 * bank_dev that is not 16-byte aligned, bench_dev where mdp_evaluate refuses
 * it, a capturing stream, and every _dev pointer that is not device memory of
 * the full size (bank n_sets * stride, ret matchups * episodes * n_agents, ...). */
int64_t mdp_actor_set_floats(const mdp_handle* h);
int mdp_actor_set_write(mdp_handle* h, float* set_dev, int32_t agent, const float* src_host, int64_t n);
int mdp_actor_set_snapshot(mdp_handle* h, float* set_dev);
int mdp_evaluate_matchups(mdp_handle* h, const float* bank_dev, int32_t n_sets,
                          const int32_t* table_host, int32_t matchups,
                          int64_t first_episode, int32_t episodes, int32_t mode,
                          const float* u_dev, float* ret_dev, float* bench_dev);
/* finished-episode log, a ring of episode_log_rows entries [total | per agent]:
 * mdp_episode_count is the number of entries written so far (`count`);
 * mdp_episode_log copies entries [first, first + n) in the order they were
 * logged into out_host[n][1 + n_agents].  Only the last episode_log_rows
 * entries are live: the range must lie inside
 * [max(0, count - episode_log_rows), count), and 0 <= n <= episode_log_rows.
 * A range that reaches an overwritten or a not yet written entry is refused
 * (< 0, the message names mdp_episode_log and the live window); nothing is
 * copied then.  Both calls synchronise the handle's stream. */
int64_t mdp_episode_count(mdp_handle* h);
int mdp_episode_log(mdp_handle* h, int64_t first, int64_t n, float* out_host);

/* ---- prioritized replay (opt-in; the reference's unused second buffer,
 * maddpg/trainer/prioritized_replay_buffer.py, after Schaul et al. 2016) -----
 * Proportional prioritization on the device, one sum tree per agent driven by
 * that agent's own critic TD error (DESIGN.md "Prioritized replay" holds the
 * semantics and the departures from the reference module):
 *   priority of a trained row   min(|q - y| + eps, abs_err_upper) ** alpha (fp32)
 *   priority of a written row   abs_err_upper ** alpha (every ring write resets it)
 *   tree                        complete binary tree over P = 2^k >= capacity
 *                               leaves; node = {sum, min} fp32, parent.sum =
 *                               fl32(left.sum + right.sum), parent.min = min;
 *                               an unfilled leaf is {0, +inf}.  Ancestors are
 *                               recomputed from their children (no deltas, no
 *                               float atomics): the tree is a pure function of
 *                               its leaves, graph replay == eager
 *   sampling of B rows          seg = total / B, v_i = (i + u_i) * seg, descent:
 *                               right (v -= left.sum) iff v >= left.sum and
 *                               right.sum > 0.  u_i injected or Philox word 0 of
 *                               counter (i, samples drawn by this agent,
 *                               0x50000 | agent, 0), key = cfg.seed, through u01
 *   IS weight                   beta <- min(1, beta + beta_inc) first, then
 *                               w_i = (p_i / p_min) ** -beta, p_min = root.min
 *   critic step                 loss mean_b(w_b (q_b - y_b)^2); the actor step is
 *                               unweighted
 * State lives in a SECOND caller-allocated device buffer of mdp_per_bytes(cfg)
 * bytes (the arena and mdp_arena_bytes are unchanged): the ring-sync cursor,
 * per-agent beta and sample counter, per-agent index / weight / |TD error|
 * slots [n][B] and the trees.  It is not checkpointed (nor is the replay ring).
 * mdp_per_enable comes before the handle's first update / train call (captured
 * graphs never go stale); afterwards, with the defaults of the reference module
 * alpha 0.6, beta0 0.4, beta_inc 0.001, eps 0.01, abs_err_upper 1:
 *   mdp_update(idx_dev == NULL) draws the rows from that agent's tree; with
 *   idx_dev it takes those rows and their weights from the tree (beta advances
 *   the same way); the rows' priorities are written back after the critic step.
 *   mdp_update_round / mdp_train_step / mdp_train_steps do the same per round,
 *   eagerly and captured: ring sync, every agent's draw (one launch), the strict
 *   round, every agent's write-back (one launch).  No MT19937 index draw runs.
 * Refused with a message: throughput mode (either call order), any
 * data-parallel wiring (mdp_dp_init, mdp_dp_xgmi_*, world_size > 1), the phase
 * entry point mdp_critic_grad. */
int64_t mdp_per_bytes(const mdp_config* cfg);
int mdp_per_enable(mdp_handle* h, void* buf_dev, int64_t bytes, float alpha, float beta0, float beta_inc,
                   float eps, float abs_err_upper);
/* `count` rows of agent's tree (ring positions, not tree indices) and their IS
 * weights; u_dev: [count] injected uniforms in [0, 1) or NULL (device Philox).
 * Advances the agent's beta and sample counter on the device.  A row without a
 * priority -- an unfilled position among the rows given to mdp_update, or a
 * priority the caller set to 0 (such a leaf is {0, +inf} like an unfilled one:
 * never drawn, not part of p_min) -- gets weight 0 (it takes no part in the
 * critic loss) instead of inf / NaN; the draw itself needs total > 0, so keep
 * at least one priority positive. */
int mdp_per_sample(mdp_handle* h, int32_t agent, int32_t count, const float* u_dev, int32_t* idx_out_dev,
                   float* w_out_dev);
/* leaves of ring positions pos_dev [count] <- p_dev (raw priorities), or <-
 * min(abs_err + eps, abs_err_upper) ** alpha; ancestors repaired.  A position
 * repeated in one call gets the largest of its values (a row drawn twice has
 * its TD target sampled twice), whatever the order; priorities are >= 0;
 * positions outside the filled ring (< 0, >= the ring length) are ignored. */
int mdp_per_set_priorities(mdp_handle* h, int32_t agent, const int32_t* pos_dev, const float* p_dev, int32_t count);
int mdp_per_update_errors(mdp_handle* h, int32_t agent, const int32_t* pos_dev, const float* abs_err_dev,
                          int32_t count);
/* byte offsets inside the PER buffer of agent's slots of its last update:
 * out3 = {indices int32 [B], IS weights fp32 [B], |TD errors| fp32 [B]} */
int mdp_per_slots(mdp_handle* h, int32_t agent, int64_t out3[3]);
/* nodes of one tree (2 P; -1 without PER); mdp_per_get_tree copies agent's
 * [2 P][2] floats {sum, min} (node 0 unused and zero, node 1 the root, node
 * P + i ring position i) after bringing the tree up to date with the ring */
int64_t mdp_per_tree_nodes(const mdp_handle* h);
int mdp_per_get_tree(mdp_handle* h, int32_t agent, float* nodes_host);
/* out5 = {beta, total (root.sum), p_min (root.min), ring rows synced into the
 * trees so far, sample calls of this agent}; synchronises */
int mdp_per_info(mdp_handle* h, int32_t agent, double out5[5]);

/* ---- MATD3: twin critics, clipped double-Q target, delayed policy updates --
 * (DESIGN.md section 17).  Every agent gets a second critic Q2 with its own target,
 * Adam slots and beta powers in a SECOND caller-allocated device buffer of
 * mdp_td3_bytes(cfg) bytes, which must outlive the handle.  Agent i's k-th
 * update since enable (k = 1, 2, ...):
 *   y = r + gamma (1 - done) min(Q1_tgt(x'), Q2_tgt(x'))   (fp32 min, fp64 TD line)
 *   both critics step on mean (Q_c(x) - y)^2 with their own Adam;
 *   if k % policy_delay == 0: the actor step (on Q1 after its step), then
 *   Polyak of the target actor, target Q1 and target Q2; otherwise the actor,
 *   its Adam state and all three targets stay bit-unchanged.
 * The training-noise counter advances once per agent update either way.
 * mdp_get_stats: [0] critic 1's loss, [1] p_loss of the most recent actor step
 * (0 before the first), [4] the mean of min(q1', q2'), the rest as without TD3.
 * policy_delay in 1..8 (1: twin critics without delay).  Enable comes before
 * the handle's first update / train call.  MATD3 runs in strict mode on one
 * GPU on the general gradient kernels; refused: prioritized replay, throughput
 * mode, mdp_update_all, data parallelism, and the phase entry points
 * mdp_critic_grad / mdp_actor_grad / mdp_reduce_grad / mdp_apply_grad.
 * mdp_set_params / mdp_get_params take MDP_CRITIC2 .. MDP_G_CRITIC2 and
 * mdp_get_beta_powers / mdp_set_beta_powers net = 2 on a TD3 handle only.
 * The per-agent update counters live on the host and start at 0 at enable.
 * The buffer starts with the second critic's five param-space regions (theta,
 * target, Adam m, Adam v, reduced gradient: param_floats floats each, every
 * region rounded up to 256 bytes, tensors at the arena regions' offsets; the
 * actor spans stay zero); its partials, stats and sync area follow. */
int64_t mdp_td3_bytes(const mdp_config* cfg);
int mdp_td3_enable(mdp_handle* h, void* buf_dev, int64_t bytes, int32_t policy_delay);
/* out4 = {critic updates, actor updates, q_loss of critic 1, q_loss of critic 2}
 * of agent's last update; synchronises */
int mdp_td3_info(mdp_handle* h, int32_t agent, double out4[4]);

/* ---- M3DDPG: minimax critic targets and actor loss (Li et al., AAAI 2019; ----
 * DESIGN.md section 20).  eps_host [n_agents][n_agents], row-major, finite and
 * >= 0: eps[i][j] is agent i's perturbation rate for agent j's action (the
 * diagonal is ignored).  With g_j the gradient of agent i's (target) Q to
 * agent j's action of a batch row and ghat_j = g_j / sqrt(max(sum g_j^2,
 * 1e-12)) over agent j's logical action entries:
 *   critic step: q' = Q_tgt_i([o' | a~_i, (a~_j - eps[i][j] ghat_j)_{j != i}]), the
 *                gradient taken at the unperturbed target actions; the TD line
 *                and everything after it as without M3DDPG;
 *   actor step:  p_loss = -mean Q_i([o | a_i, (a_j - eps[i][j] ghat_j)_{j != i}])
 *                + the regulariser, the gradient taken at the replayed actions
 *                and the sample a_i; the perturbation is a constant of the
 *                backward.
 * One linearised worst-case step, neither clipped nor renormalised; pad entries
 * of a narrower agent's slot stay exact zeros.  An agent with a local (DDPG)
 * critic sees no other action: its update is the one without M3DDPG, bit for
 * bit; with every eps[i][*] = 0 agent i's update equals the MADDPG update of the
 * general gradient kernels bit for bit.  mdp_get_stats: [1] the perturbed
 * p_loss, [4] the mean of the perturbed q'.  Noise streams and counters are
 * MADDPG's.  Enable comes before the handle's first update / train call.
 * M3DDPG runs in strict mode on one GPU on the general gradient kernels;
 * refused: prioritized replay, MATD3, throughput mode, mdp_update_all, data
 * parallelism, and the phase entry points mdp_critic_grad / mdp_actor_grad /
 * mdp_reduce_grad / mdp_apply_grad.  No new parameters: checkpoints and the
 * evaluation entry points are unchanged. */
int mdp_minimax_enable(mdp_handle* h, const float* eps_host);
/* eps_out_host [n_agents][n_agents] as enabled (diagonal 0) */
int mdp_minimax_info(mdp_handle* h, float* eps_out_host);
/* debug: device buffers [batch_size][n_agents][MDP_ACT_DIM] (or NULL: none) that
 * receive every agent's action as the second forward of the next critic /
 * actor steps of a minimax agent reads it (the agent's own slot unperturbed) */
int mdp_minimax_debug_adv(mdp_handle* h, float* critic_adv_dev, float* actor_adv_dev);

/* ---- Inferred policies: approximators of the other agents, trained on the ----
 * device (Lowe et al. 2017, section 4.2).  Every agent i
 * with a MADDPG critic gets, for every other agent j, an approximator phi_i^j:
 * an MLP of agent j's actor shape (pad rules and action width A_j included)
 * with its own target network, Adam slots and beta powers, in a caller-
 * allocated device buffer of mdp_approx_bytes bytes that must outlive the
 * handle.  Agents with a local (DDPG) critic get none; their update is today's,
 * bit for bit.  Agent i's update on its minibatch then runs
 *   1. the critic step, with the target action of every j != i drawn from the
 *      target approximator of (i, j) on o'_j instead of target actor j -- same
 *      noise (u_tgt[j] or Philox stream (i << 8) | (j + 1)); agent i's own
 *      target action still comes from its target actor;
 *   2. the actor step and Polyak of actor and critic, unchanged;
 *   3. one gradient step of every phi_i^j on the same rows:
 *        loss = mean_b[ -sum_c a_c log p_c - lambda H(p) ],  p = softmax of the
 *        first A_j logits of phi_i^j(o_j), a = agent j's replayed action, log p
 *        the log-softmax; per-tensor clip and Adam with the handle's lr, betas,
 *        eps and clip on the pair's own slots; then target <- (1 - tau) target +
 *        tau phi with the optimizer kernels' constants.
 * With every target approximator holding the bits of the target actor it
 * stands for, agent i's first update equals the MADDPG update of the general
 * gradient kernels bit for bit.  The training-noise counter advances as without
 * the option.  lambda is finite and >= 0 (the paper: 1e-3).  Enable comes before
 * the handle's first update / train call and zeroes the buffer: write the
 * approximators afterwards.  Runs in strict mode on one GPU on the general
 * gradient kernels; refused: prioritized replay, MATD3, M3DDPG, throughput
 * mode, mdp_update_all, data parallelism and the phase entry points.
 * The buffer starts with, per observing agent, five param-space regions (net,
 * target, Adam m, Adam v, reduced gradient: param_floats floats each, rounded
 * up to 256 bytes): phi_i^j lies in agent j's actor span at the arena's
 * offsets, every other span stays zero; the partials, records, beta powers and
 * the optimizer launches' own sync area follow. */
enum mdp_approx_set { MDP_APX_NET = 0, MDP_APX_TARGET = 1, MDP_APX_M = 2, MDP_APX_V = 3, MDP_APX_GRAD = 4 };
int64_t mdp_approx_bytes(const mdp_config* cfg);
int mdp_approx_enable(mdp_handle* h, void* buf_dev, int64_t bytes, float lambda);
/* set `which` (mdp_approx_set) of phi_observer^agent in agent's actor layout, as
 * mdp_set_params / mdp_get_params take MDP_ACTOR.  MDP_APX_GRAD reads the raw
 * (unclipped) batch gradient of the pair's last gradient launch */
int mdp_approx_set_params(mdp_handle* h, int32_t observer, int32_t agent, int32_t which, const float* src, int64_t n);
int mdp_approx_get_params(mdp_handle* h, int32_t observer, int32_t agent, int32_t which, float* dst, int64_t n);
int mdp_approx_get_beta_powers(mdp_handle* h, int32_t observer, int32_t agent, float out2[2]);
int mdp_approx_set_beta_powers(mdp_handle* h, int32_t observer, int32_t agent, const float in2[2]);
/* out4 = {cross-entropy, entropy, loss = cross-entropy - lambda entropy (batch
 * means of the pair's last gradient launch), steps of the pair so far}; synchronises */
int mdp_approx_info(mdp_handle* h, int32_t observer, int32_t agent, double out4[4]);
/* mdp_actor_logits on phi_observer^agent (target != 0: its target network); the
 * trailing arguments keep mdp_actor_logits' order: obs_dev, logits_dev, rows */
int mdp_approx_logits(mdp_handle* h, int32_t observer, int32_t agent, int32_t target, const float* obs_dev,
                      float* logits_dev, int32_t rows);
/* step 3 alone on rows idx_dev [batch_size]: mdp_approx_grad launches only the
 * gradient kernel of every pair of `observer`; mdp_approx_step the whole step
 * (gradients, every pair's optimizer step, Polyak).  Neither touches a MADDPG
 * parameter set or the noise counter */
int mdp_approx_grad(mdp_handle* h, int32_t observer, const int32_t* idx_dev);
int mdp_approx_step(mdp_handle* h, int32_t observer, const int32_t* idx_dev);

/* ---- profiling: HIP events bracketing every launch of one kernel kind -- */
enum mdp_kernel_kind {
    MDP_K_INDEX = 0, MDP_K_GATHER = 1, MDP_K_CRITIC_GRAD = 2, MDP_K_ACTOR_GRAD = 3,
    MDP_K_APPLY = 4, MDP_K_ROLLOUT = 5, MDP_K_REDUCE = 6, MDP_K_REDUCE_APPLY = 7,
    MDP_K_ALLREDUCE = 8,   /* the RCCL data-parallel all-reduces (not a kernel of this library) */
    MDP_K_PER_SYNC = 9, MDP_K_PER_SAMPLE = 10, MDP_K_PER_UPDATE = 11,   /* prioritized replay (mdp_per.hip) */
    MDP_K_EVAL = 12,       /* k_eval_episodes (mdp_evaluate, mdp_evaluate_matchups, mdp_evaluate_q + its k_eval_returns) */
    MDP_K_COUNT = 13
};
/* Inferred policies add no kind: k_approx_grad is timed under MDP_K_ACTOR_GRAD,
 * the pairs' optimizer launches under MDP_K_REDUCE_APPLY (or MDP_K_REDUCE and
 * MDP_K_APPLY) and the approximators' k_polyak under MDP_K_APPLY.  With the
 * option on, those kinds therefore sum two different kernels each: time one of
 * them alone through mdp_approx_grad / mdp_approx_step or with device events. */
int mdp_prof_enable(mdp_handle* h, int32_t kind, int32_t on);
/* which grad kernels serve `agent`: 1 = register-resident k_*_grad_r (H = 64
 * envelope), 0 = general k_*_grad */
int mdp_grad_variant(mdp_handle* h, int32_t agent);
/* workgroups per 16-row tile of the strict-mode k_critic_grad_r launch, decided
 * at mdp_create: 2 (twins, each forming half of the tile's weight-gradient
 * tiles; same results bit for bit) while 3 x ceil(batch / 16) + 1 workgroups
 * find a compute unit each, else 1; MDP_GRAD_TWIN=0 in the environment at
 * create: always 1.  Throughput mode and the general kernels launch one. */
int mdp_grad_twin(mdp_handle* h);
/* sum of event-measured durations (ms) and launch count since enable; synchronises */
int mdp_prof_read(mdp_handle* h, int32_t kind, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* MADDPG_HIP_H */
