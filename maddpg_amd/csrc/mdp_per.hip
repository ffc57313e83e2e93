// mdp_per.hip -- device-side prioritized experience replay (Schaul et al. 2016,
// proportional variant; the reference's maddpg/trainer/prioritized_replay_buffer.py
// restated per DESIGN.md "Prioritized replay").
//
// One sum tree per agent (mdp_kernels.h: PerNode heap array over P = 2^k leaves,
// every node {sum, min}).  The tree is a PURE FUNCTION of its leaves: a kernel
// that changes leaves recomputes their ancestors from the children, level by
// level with a workgroup barrier between levels -- no deltas, no float atomics
// -- so any update order gives the same bits and a graph replay equals the eager
// run.  One workgroup serves one agent's tree in the writing kernels, which
// makes the barrier a __syncthreads() (its workgroup-scope release / acquire
// orders the global stores of a level before the loads of the next).
//
//   k_per_sync    ring -> trees: positions written since the last sync get the
//                 new-row priority (the ring head and env step counter are read
//                 from the device Ctl, the cursor from PerHdr)
//   k_per_sample  stratified descent (or given rows) -> indices + IS weights;
//                 advances beta and the sample counter on the device
//   k_per_update  leaf writes from priorities or |TD errors|, then the ancestors
#include <hip/hip_runtime.h>

#include "mdp_device.h"
#include "mdp_kernels.h"

namespace {

#define MDP_PER_NT 1024   // threads of the tree-writing workgroups
#define MDP_PER_ST 256    // threads of a sampling workgroup

__device__ __forceinline__ PerNode per_join(const PerNode* T, int64_t node) {
  // both children in one 16-byte load (2 node is even: 16-byte aligned)
  const float4 c = *reinterpret_cast<const float4*>(T + 2 * node);
  PerNode r;
  r.sum = c.x + c.z;
  r.min = fminf(c.y, c.w);
  return r;
}

// recompute the ancestors of the leaves [lo, lo + cnt) (ring positions), level
// by level up to the root; every thread of the workgroup calls it
__device__ __forceinline__ void per_repair_level(PerNode* T, int64_t P, int64_t lo, int64_t cnt, int l, int tid, int nt) {
  if (cnt <= 0) return;
  const int64_t a = (P + lo) >> l, b = (P + lo + cnt - 1) >> l;
  for (int64_t j = a + tid; j <= b; j += nt) T[j] = per_join(T, j);
}

__global__ __launch_bounds__(MDP_PER_NT) void k_per_sync(PerSyncArgs a) {
  PerNode* T = a.trees + (int64_t)blockIdx.x * a.tree_stride;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t steps = a.ctl->env_steps, next = a.ctl->next, len = a.ctl->len;
  const int64_t seen = a.hdr->seen_steps;
  const int64_t arrived = (steps - seen) * (int64_t)a.E + a.host_rows;
  const int64_t P = a.P;
  PerNode fresh, empty;
  fresh.sum = fresh.min = powf(a.upper, a.alpha);
  empty.sum = 0.f;
  empty.min = INFINITY;
  int64_t moved = 0;
  if (a.reset || arrived >= a.cap) {  // every filled leaf is new
    for (int64_t i = tid; i < P; i += nt) T[P + i] = i < len ? fresh : empty;
    for (int64_t w = P >> 1; w >= 1; w >>= 1) {
      __syncthreads();
      for (int64_t j = tid; j < w; j += nt) T[w + j] = per_join(T, w + j);
    }
    moved = len;
  } else if (arrived > 0) {  // the `arrived` positions behind the ring head, in up to two runs
    int64_t start = (next - arrived) % a.cap;
    if (start < 0) start += a.cap;
    const int64_t n0 = arrived < a.cap - start ? arrived : a.cap - start, n1 = arrived - n0;
    for (int64_t i = tid; i < n0; i += nt) T[P + start + i] = fresh;
    for (int64_t i = tid; i < n1; i += nt) T[P + i] = fresh;
    for (int l = 1; (P >> l) >= 1; ++l) {
      __syncthreads();
      per_repair_level(T, P, start, n0, l, tid, nt);
      per_repair_level(T, P, 0, n1, l, tid, nt);
    }
    moved = arrived;
  }
  // the last workgroup (every one has read the cursor by then) advances it
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    const uint32_t old = atomicAdd(&a.hdr->ticket, 1u);
    if (old == gridDim.x - 1) {
      a.hdr->seen_steps = steps;
      a.hdr->rows_synced += moved;
      a.hdr->ticket = 0u;
    }
  }
}

__global__ __launch_bounds__(MDP_PER_ST) void k_per_sample(PerSampleArgs a) {
  // the top levels of the tree (one round trip for all of them): the descent's
  // chain of dependent loads then starts below them
  __shared__ __attribute__((aligned(16))) PerNode top[MDP_PER_TOP];
  const int ag = blockIdx.y;
  const PerNode* T = a.trees + (int64_t)ag * a.tree_stride;
  PerState* st = a.st + ag;
  const int tid = threadIdx.x;
  const int64_t P = a.P;
  const int ntop = 2 * P < MDP_PER_TOP ? (int)(2 * P) : MDP_PER_TOP;
  const float beta0 = st->beta;
  const uint32_t samples = st->samples;
  for (int j = tid; j < ntop; j += MDP_PER_ST) top[j] = T[j];
  const int i = blockIdx.x * MDP_PER_ST + tid;
  float u = 0.f;
  if (i < a.count && !a.idx_in) {
    if (a.u) {
      u = a.u[i];
    } else {
      const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
      u = u01(Philox::gen(make_uint4((uint32_t)i, samples, MDP_PER_STREAM | (uint32_t)(a.agent0 + ag), 0u), key).x);
    }
  }
  __syncthreads();
  const float beta = fminf(1.0f, beta0 + a.beta_inc);
  if (i < a.count) {
    int64_t node;
    if (a.idx_in) {
      int64_t r = a.idx_in[i];
      r = r < 0 ? 0 : (r >= a.cap ? a.cap - 1 : r);
      node = P + r;
    } else {
      const float total = top[1].sum;
      const float seg = total / (float)a.count;
      float v = ((float)i + u) * seg;
      node = 1;
      while (node < P) {
        const int64_t left = 2 * node;
        float ls, rs;
        if (left < ntop) {
          ls = top[left].sum;
          rs = top[left + 1].sum;
        } else {
          const float4 c = *reinterpret_cast<const float4*>(T + left);
          ls = c.x;
          rs = c.z;
        }
        if (v >= ls && rs > 0.f) {
          v -= ls;
          node = left + 1;
        } else {
          node = left;
        }
      }
    }
    const float p = node < ntop ? top[node].sum : T[node].sum;
    const float p_min = top[1].min;
    a.idx_out[(int64_t)ag * a.stride + i] = (int32_t)(node - P);
    // a row without a priority (an unfilled position among given rows, a zero
    // priority set by the caller) takes no part in the loss: weight 0, not inf / NaN
    a.w_out[(int64_t)ag * a.stride + i] = (p > 0.f && p_min < INFINITY) ? powf(p / p_min, -beta) : 0.f;
  }
  // the agent's last workgroup (every one has read beta and the counter) advances them
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    const uint32_t old = atomicAdd(&st->ticket, 1u);
    if (old == gridDim.x - 1) {
      st->beta = beta;
      st->samples = samples + 1u;
      st->ticket = 0u;
    }
  }
}

__global__ __launch_bounds__(MDP_PER_NT) void k_per_update(PerUpdateArgs a) {
  const int ag = blockIdx.x;
  PerNode* T = a.trees + (int64_t)ag * a.tree_stride;
  const int32_t* pos = a.pos + (int64_t)ag * a.stride;
  const float* val = a.val + (int64_t)ag * a.stride;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t P = a.P;
  const int64_t len = a.ctl->len < a.cap ? a.ctl->len : a.cap;
  // A row drawn more than once in the batch can carry different values (its TD
  // target is sampled per batch position): the largest one becomes its
  // priority, whatever the order -- an integer max on the bits of the
  // non-negative floats, so no float atomic and the same bits every time.
  for (int i = tid; i < a.count; i += nt) {
    const int64_t r = pos[i];
    if (r < 0 || r >= len) continue;
    T[P + r].sum = 0.f;
  }
  __syncthreads();
  for (int i = tid; i < a.count; i += nt) {
    const int64_t r = pos[i];
    if (r < 0 || r >= len) continue;
    float p = val[i];
    if (a.from_err) p = powf(fminf(p + a.eps, a.upper), a.alpha);
    atomicMax(reinterpret_cast<unsigned int*>(&T[P + r].sum), __float_as_uint(fmaxf(p, 0.f)));
  }
  __syncthreads();
  for (int i = tid; i < a.count; i += nt) {
    const int64_t r = pos[i];
    if (r < 0 || r >= len) continue;
    // (the max was formed in L2: read it there, then write the whole leaf the ordinary way)
    PerNode leaf;
    leaf.sum = __uint_as_float(__hip_atomic_load(reinterpret_cast<unsigned int*>(&T[P + r].sum), __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT));
    leaf.min = leaf.sum > 0.f ? leaf.sum : INFINITY;  // a zero priority is never drawn: not part of p_min either
    T[P + r] = leaf;
  }
  for (int l = 1; (P >> l) >= 1; ++l) {
    __syncthreads();
    for (int i = tid; i < a.count; i += nt) {
      const int64_t r = pos[i];
      if (r < 0 || r >= len) continue;
      const int64_t j = (P + r) >> l;
      T[j] = per_join(T, j);
    }
  }
}

}  // namespace

#define MDP_PER_CHECK_LAUNCH()           \
  do {                                   \
    hipError_t e_ = hipGetLastError();   \
    if (e_ != hipSuccess) return e_;     \
  } while (0)

hipError_t mdp_launch_per_sync(const PerSyncArgs& a, int agents, hipStream_t s) {
  mdp_launch(k_per_sync, dim3(agents), dim3(MDP_PER_NT), 0, s, a);
  MDP_PER_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t mdp_launch_per_sample(const PerSampleArgs& a, int agents, hipStream_t s) {
  mdp_launch(k_per_sample, dim3((a.count + MDP_PER_ST - 1) / MDP_PER_ST, agents), dim3(MDP_PER_ST), 0, s, a);
  MDP_PER_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t mdp_launch_per_update(const PerUpdateArgs& a, int agents, hipStream_t s) {
  mdp_launch(k_per_update, dim3(agents), dim3(MDP_PER_NT), 0, s, a);
  MDP_PER_CHECK_LAUNCH();
  return hipSuccess;
}
