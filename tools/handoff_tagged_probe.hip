// handoff_tagged_probe.hip -- the in-launch hand-off of the actor-step
// optimizer's target actor to the next critic step, with the protocol the fused
// optimizer ships today (one tagged word per chunk, no counter, few pollers)
// instead of the one tools/handoff_probe.hip measured in round 3 (a counter
// every producer adds to, every consumer polling it, the block read in a loop).
// (measurement tool, not part of the library)
//
// One launch at the S2 shape: PT producer workgroups first (PA of them active:
// the 26 chunk workgroups of the actor net, then Polyak / stats stand-ins; the
// rest exit at once -- the pad to a multiple of 8), then C consumer workgroups,
// all of 512 threads and one per CU (a dynamic LDS request keeps a second
// workgroup off the CU, as the critic kernel's registers do).
//   producer: waves 4..7 exit; waves 0..3 spin `work` us (the optimizer's body up
//     to Adam), store their slice of the block -- chunk c of tensor t of the
//     actor net, tensor-relative as mdp_apply_fused.hip cuts it, so chunk edges
//     fall inside 128-B lines -- with agent-scope 4-byte stores (write-through),
//     drain them (s_waitcnt vmcnt(0)), meet at one barrier, and one lane stores
//     the epoch to the workgroup's own word.
//   consumer: every thread issues its share of a `pre`-KiB prologue (40 KiB the
//     workgroups share -- weights -- and 8 KiB of their own -- rows, the cpre
//     block); then waves 0..3 only: lane c polls word c (bounded spin that sets
//     the fault word) and, once every word carries the epoch, the wave loads its
//     column tile of the block with agent-scope 4-byte loads in the pattern of
//     the critic_post path (rt_load_k<16> of W1 with K = 18, rt_load<16> of W2,
//     b1, b2; wave 0 also the head's 16 + 1) and checks every value.
// Printed (us from the launch's first workgroup start; median over reps of the
// per-launch figure): the last chunk producer's spin end, stores drained and
// word stored; the consumers' first / last start; over the consumers' polling
// waves, every word seen (median / max) and the block in registers (median /
// max); stale values and the fault word.  `words` = 26 polls the chunk
// workgroups only, 41 every active producer; `stride` is the distance between
// two workgroups' words in 4-byte units (1: one line holds them all; 16: 64 B).
//   hipcc -O3 --offload-arch=gfx950 tools/handoff_tagged_probe.hip -o tools/handoff_tagged_probe_bin
//   tools/handoff_tagged_probe_bin [work_us=3.7] [words=26] [stride=1] [PT=48] [PA=41] [C=193] [pre_kib=48] [reps=200]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHK(x)                                                                   \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));  \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

// the S2 actor net (obs 18, H = 64, 5 actions), tensors back to back
constexpr int kNT = 6;
__device__ constexpr int kTN[kNT] = {18 * 64, 64, 64 * 64, 64, 64 * 5, 5};
__device__ constexpr int kTOff[kNT + 1] = {0, 1152, 1216, 5312, 5376, 5696, 5701};
constexpr int kChunk = 256;
constexpr int kNCh = 5 + 1 + 16 + 1 + 2 + 1;  // 26 chunk workgroups
constexpr int kBlock = 5701;
constexpr int kOther = 64 * kChunk;           // the Polyak / stats stand-ins' slices
constexpr int kMaxWords = 64;
constexpr uint32_t kSpinLimit = 1u << 22;
constexpr int kStamps = 16;                   // per workgroup: start, then per role (below)

struct Args {
  float* block;                 // [kBlock] the handed-over net
  float* other;                 // [kOther] what the other active producers write
  const float* pre;             // consumers' prologue data: 40 KiB shared + 8 KiB per workgroup
  uint32_t* words;              // [kMaxWords * stride] one epoch word per producer
  uint32_t* bad;                // [2] stale values, keep-alive
  uint32_t* fault;
  unsigned long long* t;        // [grid][kStamps]
  int PT, PA, C, nwords, stride, pre_shared4, pre_own4;
  uint32_t epoch;
  unsigned long long work_ticks;
};

__device__ __forceinline__ float want_at(uint32_t epoch, int i) { return (float)(epoch * 1000u + (uint32_t)i % 1000u); }
__device__ __forceinline__ float ld_agent(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(512) void k_handoff_tagged(Args a) {
  extern __shared__ float lds_hold[];
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  const int b = blockIdx.x, tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  unsigned long long* ts = a.t + (size_t)b * kStamps;
  if (b < a.PT) {
    if (b >= a.PA || wave >= 4) return;  // the pad, and the waves the optimizer's body does not use
    // producer: the optimizer's body up to Adam, then this workgroup's slice
    while (__builtin_amdgcn_s_memrealtime() - t0 < a.work_ticks) __builtin_amdgcn_s_sleep(1);
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    float* dst = nullptr;
    float v = 0.f;
    if (b < kNCh) {
      int t = 0, c = b;
      while (c >= (kTN[t] + kChunk - 1) / kChunk) c -= (kTN[t++] + kChunk - 1) / kChunk;
      const int q = c * kChunk + tid;
      if (q < kTN[t]) {
        dst = a.block + kTOff[t] + q;
        v = want_at(a.epoch, kTOff[t] + q);
      }
    } else {
      dst = a.other + (b - kNCh) * kChunk + tid;
      v = (float)a.epoch;
    }
    if (dst) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t2 = __builtin_amdgcn_s_memrealtime();
    __syncthreads();  // (the four waves that got here)
    if (tid == 0) {
      __hip_atomic_store(a.words + b * a.stride, a.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long t3 = __builtin_amdgcn_s_memrealtime();
      ts[0] = t0;
      ts[1] = t1;
      ts[2] = t2;
      ts[3] = t3;
    }
    return;
  }
  // consumer: its own prologue (nothing of it waited for), then waves 0..3 poll and load
  const float4* pre4 = reinterpret_cast<const float4*>(a.pre);
  const float4* own4 = pre4 + a.pre_shared4 + (size_t)(b - a.PT) * a.pre_own4;
  float4 pv[6];
#pragma unroll
  for (int k = 0; k < 5; ++k) pv[k] = pre4[min(tid + 512 * k, a.pre_shared4 - 1)];
  pv[5] = own4[min(tid, a.pre_own4 - 1)];
  if (tid == 0) ts[0] = t0;
  if (wave >= 4) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc += pv[k].x + pv[k].y + pv[k].z + pv[k].w;
    if (acc == 12345.f) a.bad[1] = 1;  // keep the prologue loads
    return;
  }
  // lane c polls producer c's word (one load per lane and poll)
  const bool polls = lane < a.nwords;
  const uint32_t* w = a.words + (polls ? lane : 0) * a.stride;
  uint32_t it = 0;
  bool ok = !polls || __hip_atomic_load(const_cast<uint32_t*>(w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.epoch;
  while (__ballot(!ok) != 0ull) {
    __builtin_amdgcn_s_sleep(1);
    if (++it > kSpinLimit) {
      if (lane == 0) __hip_atomic_store(a.fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    if (!ok) ok = __hip_atomic_load(const_cast<uint32_t*>(w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.epoch;
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
  // the wave's column tile: col = 16 wave + r, k = 4 s + kq
  const int r = lane & 15, kq = lane >> 4, col = 16 * wave + r;
  const float* P = a.block;
  float w1t[5], w2t[16], w3[16];
  int i1[5], i2[16], i3[16];
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    i1[s] = kTOff[0] + min(4 * s + kq, 17) * 64 + col;
    w1t[s] = ld_agent(P + i1[s]);
  }
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    i2[s] = kTOff[2] + (4 * s + kq) * 64 + col;
    w2t[s] = ld_agent(P + i2[s]);
  }
  const float b1 = ld_agent(P + kTOff[1] + col), b2 = ld_agent(P + kTOff[3] + col);
  float b3 = 0.f;
  if (wave == 0) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      i3[s] = kTOff[4] + (4 * s + kq) * 5 + min(r, 4);
      w3[s] = ld_agent(P + i3[s]);
    }
    b3 = ld_agent(P + kTOff[5] + min(r, 4));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long t2 = __builtin_amdgcn_s_memrealtime();
  uint32_t nbad = 0;
#pragma unroll
  for (int s = 0; s < 5; ++s) nbad += w1t[s] != want_at(a.epoch, i1[s]);
#pragma unroll
  for (int s = 0; s < 16; ++s) nbad += w2t[s] != want_at(a.epoch, i2[s]);
  nbad += b1 != want_at(a.epoch, kTOff[1] + col);
  nbad += b2 != want_at(a.epoch, kTOff[3] + col);
  if (wave == 0) {
#pragma unroll
    for (int s = 0; s < 16; ++s) nbad += w3[s] != want_at(a.epoch, i3[s]);
    nbad += b3 != want_at(a.epoch, kTOff[5] + min(r, 4));
  }
  if (nbad) atomicAdd(a.bad, nbad);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) acc += pv[k].x + pv[k].y + pv[k].z + pv[k].w;
  if (acc == 12345.f) a.bad[1] = 1;
  if (lane == 0) {
    ts[1 + 2 * wave] = t1;
    ts[2 + 2 * wave] = t2;
  }
}

static double med(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}
static double mx(const std::vector<double>& v) { return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()); }

int main(int argc, char** argv) {
  const double work_us = argc > 1 ? atof(argv[1]) : 3.7;
  const int nwords = argc > 2 ? atoi(argv[2]) : kNCh;
  const int stride = argc > 3 ? atoi(argv[3]) : 1;
  const int PT = argc > 4 ? atoi(argv[4]) : 48;
  const int PA = argc > 5 ? atoi(argv[5]) : 41;
  const int C = argc > 6 ? atoi(argv[6]) : 193;
  const int pre_kib = argc > 7 ? atoi(argv[7]) : 48;
  const int reps = argc > 8 ? atoi(argv[8]) : 200;
  if (PA < kNCh || PA > PT || PT > kMaxWords || nwords < 1 || nwords > PA || stride < 1 || stride > 32 || C < 1 ||
      C > 1024 || pre_kib < 16 || PA - kNCh > kOther / kChunk) {
    fprintf(stderr, "arguments out of range\n");
    return 2;
  }
  int dev = 0, cus = 0;
  CHK(hipGetDevice(&dev));
  CHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int grid = PT + C;
  // every consumer has to find a CU beside the active producers, or it would wait for nothing:
  // the producers never wait, so this is about the measurement, not about termination
  if (PA + C > cus) fprintf(stderr, "note: %d active workgroups on %d CUs: consumers will queue\n", PA + C, cus);
  Args a{};
  a.pre_shared4 = (pre_kib - 8) * 64;  // float4s
  a.pre_own4 = 8 * 64;
  const size_t pre_f4 = (size_t)a.pre_shared4 + (size_t)C * a.pre_own4;
  float* pre;
  CHK(hipMalloc(&a.block, sizeof(float) * kBlock));
  CHK(hipMalloc(&a.other, sizeof(float) * kOther));
  CHK(hipMalloc(&pre, 16 * pre_f4));
  CHK(hipMemset(pre, 0, 16 * pre_f4));
  a.pre = pre;
  CHK(hipMalloc(&a.words, 4 * kMaxWords * 32));
  CHK(hipMalloc(&a.bad, 8));
  CHK(hipMalloc(&a.fault, 4));
  CHK(hipMalloc(&a.t, sizeof(unsigned long long) * grid * kStamps));
  CHK(hipMemset(a.block, 0, sizeof(float) * kBlock));
  CHK(hipMemset(a.words, 0, 4 * kMaxWords * 32));
  CHK(hipMemset(a.bad, 0, 8));
  CHK(hipMemset(a.fault, 0, 4));
  a.PT = PT;
  a.PA = PA;
  a.C = C;
  a.nwords = nwords;
  a.stride = stride;
  a.work_ticks = (unsigned long long)(work_us * 100.0);
  const size_t lds = 96 * 1024;  // more than half a CU's LDS: one workgroup per CU
  CHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_handoff_tagged), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds));
  std::vector<double> p_spin, p_drain, p_pub, c_first, c_last, seen_med, seen_max, load_med, load_max;
  std::vector<unsigned long long> h((size_t)grid * kStamps);
  for (int rep = 0; rep < reps; ++rep) {
    a.epoch = (uint32_t)(rep + 1);
    CHK(hipMemsetAsync(a.t, 0, sizeof(unsigned long long) * grid * kStamps, 0));
    hipLaunchKernelGGL(k_handoff_tagged, dim3(grid), dim3(512), lds, 0, a);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(h.data(), a.t, sizeof(unsigned long long) * grid * kStamps, hipMemcpyDeviceToHost));
    unsigned long long s0 = ~0ull;
    for (int b = 0; b < grid; ++b)
      if (h[(size_t)b * kStamps]) s0 = std::min(s0, h[(size_t)b * kStamps]);
    auto us = [&](unsigned long long v) { return (double)(v - s0) / 100.0; };
    std::vector<double> sp, dr, pb, cs, sn, ld;
    for (int b = 0; b < nwords; ++b) {  // the producers the consumers wait for
      sp.push_back(us(h[(size_t)b * kStamps + 1]));
      dr.push_back(us(h[(size_t)b * kStamps + 2]));
      pb.push_back(us(h[(size_t)b * kStamps + 3]));
    }
    for (int b = PT; b < grid; ++b) {
      cs.push_back(us(h[(size_t)b * kStamps]));
      for (int wv = 0; wv < 4; ++wv) {
        sn.push_back(us(h[(size_t)b * kStamps + 1 + 2 * wv]));
        ld.push_back(us(h[(size_t)b * kStamps + 2 + 2 * wv]));
      }
    }
    if (rep < 5) continue;  // warm-up launches
    p_spin.push_back(mx(sp));
    p_drain.push_back(mx(dr));
    p_pub.push_back(mx(pb));
    c_first.push_back(*std::min_element(cs.begin(), cs.end()));
    c_last.push_back(mx(cs));
    seen_med.push_back(med(sn));
    seen_max.push_back(mx(sn));
    load_med.push_back(med(ld));
    load_max.push_back(mx(ld));
  }
  uint32_t bad[2], fault;
  CHK(hipMemcpy(bad, a.bad, 8, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(&fault, a.fault, 4, hipMemcpyDeviceToHost));
  printf("{\"work_us\": %.2f, \"words\": %d, \"stride\": %d, \"PT\": %d, \"PA\": %d, \"C\": %d, \"pre_kib\": %d, "
         "\"launches\": %zu, \"cus\": %d, "
         "\"producer_last_spin_end\": %.2f, \"producer_last_stores_drained\": %.2f, \"producer_last_word_stored\": %.2f, "
         "\"consumer_first_start\": %.2f, \"consumer_last_start\": %.2f, "
         "\"words_seen_med\": %.2f, \"words_seen_max\": %.2f, \"words_seen_max_worst\": %.2f, "
         "\"block_in_regs_med\": %.2f, \"block_in_regs_max\": %.2f, \"block_in_regs_max_worst\": %.2f, "
         "\"stale\": %u, \"fault\": %u}\n",
         work_us, nwords, stride, PT, PA, C, pre_kib, p_spin.size(), cus, med(p_spin), med(p_drain), med(p_pub),
         med(c_first), med(c_last), med(seen_med), med(seen_max), mx(seen_max), med(load_med), med(load_max),
         mx(load_max), bad[0], fault);
  return fault || bad[0] ? 1 : 0;
}
