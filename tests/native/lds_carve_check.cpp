// lds_carve_check -- every lds_*_bytes value of mdp_kernels.h over a fixed grid of
// topologies, as one JSON list (host only: no device is touched).
//
// tests/test_lds_carve.py compares the output with tests/golden/lds_sizes.json,
// which holds the answers of the hand-written formulas the buffer lists of
// mdp_carve.h replaced.  Only the fields the size functions read are filled in:
// n, H, row_stride, sum_obs, cin_max, obs_max and per agent obs_dim, local_q, cin
// (the replay-row layout at the top of mdp_topo.h).
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "mdp_kernels.h"

static Topo make_topo(const std::vector<int>& obs, int H, int lq_mode) {
  Topo t = {};
  const int n = (int)obs.size();
  t.n = n;
  t.H = H;
  for (int d : obs) {
    t.sum_obs += d;
    t.obs_max = std::max(t.obs_max, d);
  }
  t.row_stride = (2 * t.sum_obs + (MDP_ACT_DIM + 2) * n + 3) & ~3;
  for (int i = 0; i < n; ++i) {
    ADesc& a = t.ag[i];
    a.obs_dim = obs[i];
    a.local_q = lq_mode == 1 || (lq_mode == 2 && i == 0);  // 0: all off, 1: all on, 2: agent 0 only
    a.cin = a.local_q ? a.obs_dim + MDP_ACT_DIM : t.sum_obs + MDP_ACT_DIM * n;
    t.cin_max = std::max(t.cin_max, a.cin);
  }
  return t;
}

template <typename F>
static void per_group(const char* name, const Topo& t, F f) {
  printf(", \"%s\": [", name);
  for (int G = 1; G <= t.n; ++G) printf("%s%d", G > 1 ? ", " : "", f(t, G));
  printf("]");
}

int main() {
  std::vector<std::vector<int>> sets;
  for (int n : {1, 2, 3, 4, 6, 8}) {
    for (int d : {1, 4, 18, 33, 64, 66, 95}) sets.push_back(std::vector<int>(n, d));
    if (n == 1) sets.push_back({256});
  }
  sets.push_back({3, 11});
  sets.push_back({16, 16, 16, 14});
  // one past the widest accepted observation of (8 agents, 64 units), (3, 256), (8, 256), (1, 256)
  sets.push_back(std::vector<int>(8, 67));
  sets.push_back(std::vector<int>(3, 96));
  sets.push_back(std::vector<int>(8, 34));
  sets.push_back({257});
  printf("[");
  bool first = true;
  for (const auto& obs : sets)
    for (int H : {64, 128, 256})
      for (int lq = 0; lq < 3; ++lq) {
        const Topo t = make_topo(obs, H, lq);
        printf("%s\n{\"obs\": [", first ? "" : ",");
        first = false;
        for (size_t i = 0; i < obs.size(); ++i) printf("%s%d", i ? ", " : "", obs[i]);
        printf("], \"H\": %d, \"local_q\": %d", H, lq);
        per_group("critic", t, lds_critic_bytes);
        per_group("critic_twin", t, lds_critic_twin_bytes);
        per_group("critic_mm", t, lds_critic_mm_bytes);
        printf(", \"actor\": %d, \"actor_mm\": %d, \"approx\": %d", lds_actor_bytes(t), lds_actor_mm_bytes(t),
               lds_approx_bytes(t));
        printf(", \"critic_r\": [%d, %d], \"actor_r\": %d, \"critic_pre\": %d", lds_critic_r_bytes(t, 0),
               lds_critic_r_bytes(t, t.n - 1), lds_actor_r_bytes(t), lds_critic_pre_bytes(t));
        printf(", \"rollout\": %d, \"eval_matchups\": %d, \"eval_q\": %d", lds_rollout_bytes(t),
               lds_eval_matchups_bytes(t), lds_eval_q_bytes(t));
        printf(", \"eval\": [%d, %d]}", lds_eval_bytes(t.obs_max, H), lds_eval_bytes(t.cin_max, H));
      }
  printf("\n]\n");
  return 0;
}
