// The training variants and where a handle's state refuses a call.
//
// Four opt-in variants -- prioritized replay, MATD3, M3DDPG, inferred policies
// -- and one property of the topology, a Box action space.  No two variants
// share a handle; none runs in throughput mode, data parallel or through the
// phase entry points; a Box handle takes no variant, no throughput mode and no
// data parallelism.  That rule is the two tables below and refusal(); the shim
// (mdp_api.cpp: gate) asks it at every seam, and tests/native/variant_gate_check
// prints it cell by cell.  Host only: no HIP header, plain C++17.
//
// A new variant is one row of kVariants (and one of maddpg_amd/variants.py).
#pragma once
#include <string>

enum class Variant { None, Per, Td3, Minimax, Approx };
constexpr int kVariantCount = 5;

struct VariantInfo {
  const char* name;      // as messages and documents call it
  const char* enable;    // its enable entry point
  bool plural;           // the name takes a plural verb
  bool general_kernels;  // runs on the general gradient kernels: no actor_pre / critic_pre, no index prefetch
};
constexpr VariantInfo kVariants[kVariantCount] = {
    {"plain MADDPG", "", false, false},
    {"prioritized replay", "mdp_per_enable", false, false},
    {"MATD3", "mdp_td3_enable", false, true},
    {"M3DDPG", "mdp_minimax_enable", false, true},
    {"inferred policies", "mdp_approx_enable", true, true},
};
constexpr const VariantInfo& variant_info(Variant v) { return kVariants[(int)v]; }

// the seams: every entry point at which the handle's state can refuse the call
enum class Seam {
  Enable,         // mdp_{per,td3,minimax,approx}_enable: the variant being enabled rides along
  BoxSpace,       // mdp_set_act_spaces with a Box agent
  SetThroughput,  // mdp_set_update_mode(1)
  UpdateAll,
  DpInit, XgmiOpen, XgmiConnect, XgmiProbe, XgmiEnable,
  CriticGrad, ActorGrad, ReduceGrad, ApplyGrad,
};
constexpr int kSeamCount = 13;
enum class SeamKind { Enable, BoxSpace, Throughput, DataParallel, Phase };

constexpr unsigned vbit(Variant v) { return 1u << (int)v; }
constexpr unsigned kEveryVariant = vbit(Variant::Per) | vbit(Variant::Td3) | vbit(Variant::Minimax) | vbit(Variant::Approx);

struct SeamInfo {
  const char* fn;     // the entry point ("" for Enable: the variant's own)
  SeamKind kind;
  unsigned variants;  // handles with one of these variants are refused here
  bool box;           // a Box handle is refused here
  bool joins;         // the call joins data parallelism: refused once throughput mode is chosen
};
// The masks below that are narrower than their neighbours' are what the shim
// did, case by case, before this table existed.  They are kept, not endorsed:
//  - mdp_dp_xgmi_connect / _probe, the steps between open and enable, refuse a
//    Box handle only (a variant's handle never gets past mdp_dp_xgmi_open, so
//    they answer "open first" instead) and do not look at the update mode;
//  - mdp_actor_grad / mdp_reduce_grad / mdp_apply_grad let a prioritized handle
//    through where mdp_critic_grad refuses it;
//  - no phase entry point refuses a Box handle;
//  - mdp_set_act_spaces refuses a handle that joined data parallelism but not one
//    merely created with world_size > 1 (GateState::dp_joined / dp_world).
constexpr SeamInfo kSeams[kSeamCount] = {
    {"", SeamKind::Enable, kEveryVariant, true, false},
    {"mdp_set_act_spaces", SeamKind::BoxSpace, kEveryVariant, false, false},
    {"mdp_set_update_mode", SeamKind::Throughput, kEveryVariant, true, false},
    {"mdp_update_all", SeamKind::Throughput, kEveryVariant, true, false},
    {"mdp_dp_init", SeamKind::DataParallel, kEveryVariant, true, true},
    {"mdp_dp_xgmi_open", SeamKind::DataParallel, kEveryVariant, true, true},
    {"mdp_dp_xgmi_connect", SeamKind::DataParallel, 0, true, false},
    {"mdp_dp_xgmi_probe", SeamKind::DataParallel, 0, true, false},
    {"mdp_dp_xgmi_enable", SeamKind::DataParallel, kEveryVariant, true, true},
    {"mdp_critic_grad", SeamKind::Phase, kEveryVariant, false, false},
    {"mdp_actor_grad", SeamKind::Phase, kEveryVariant & ~vbit(Variant::Per), false, false},
    {"mdp_reduce_grad", SeamKind::Phase, kEveryVariant & ~vbit(Variant::Per), false, false},
    {"mdp_apply_grad", SeamKind::Phase, kEveryVariant & ~vbit(Variant::Per), false, false},
};
constexpr const SeamInfo& seam_info(Seam s) { return kSeams[(int)s]; }

// what of a handle the decision reads
struct GateState {
  Variant variant = Variant::None;
  bool box = false;      // some agent has a Box space
  bool trained = false;  // an update, round or train call was made
  int update_mode = 0;   // 0 strict, 1 throughput
  bool dp_joined = false;  // an RCCL communicator or the xGMI exchange is set up or being set up
  bool dp_world = false;   // created with world_size > 1
};

// "<name> (<enable>)"
inline std::string variant_ref(Variant v) {
  return std::string(variant_info(v).name) + " (" + variant_info(v).enable + ")";
}
inline const char* verb(Variant v, const char* singular, const char* plural) {
  return variant_info(v).plural ? plural : singular;
}

// why a Box handle stays out of everything else
inline std::string box_reason() {
  std::string s = "a handle with a Box action space (mdp_set_act_spaces) trains in strict mode on one GPU: no ";
  for (int v = 1; v < kVariantCount; ++v) s += std::string(kVariants[v].name) + ", ";
  return s + "throughput mode or data-parallel exchange";
}

// The refusal of `at` on a handle in state `s` ("<entry point>: <reason>"), or
// the empty string when the call may go on.  `enabling`: the variant of Seam::Enable.
inline std::string refusal(const GateState& s, Seam at, Variant enabling = Variant::None) {
  const SeamInfo& seam = seam_info(at);
  const std::string fn = seam.kind == SeamKind::Enable ? variant_info(enabling).enable : seam.fn;
  const auto no = [&](const std::string& why) { return fn + ": " + why; };
  if (s.box && seam.box) return no(box_reason());
  const bool held = s.variant != Variant::None && (seam.variants & vbit(s.variant));
  const Variant v = seam.kind == SeamKind::Enable ? enabling : s.variant;
  const std::string one_gpu = variant_ref(v) + verb(v, " runs", " run") + " on one GPU in strict mode: no data-parallel exchange";
  const std::string strict = variant_ref(v) + verb(v, " needs", " need") + " the strict update mode (throughput mode is not supported)";
  switch (seam.kind) {
    case SeamKind::Enable:
      if (s.variant == enabling) return no("already enabled");
      if (held) return no(std::string(variant_info(enabling).name) + " and " + variant_ref(s.variant) + " do not combine");
      if (s.trained) return no("call it before the handle's first update, round or train call");
      if (s.update_mode != 0) return no(strict);
      if (s.dp_joined || s.dp_world) return no(one_gpu);
      break;
    case SeamKind::BoxSpace:
      if (held || s.update_mode != 0 || s.dp_joined) return no(box_reason());
      break;
    case SeamKind::Throughput:
      if (held) return no(strict);
      break;
    case SeamKind::DataParallel:
      if (held) return no(one_gpu);
      if (s.update_mode != 0 && seam.joins) return no("join data parallelism before choosing the throughput mode");
      break;
    case SeamKind::Phase:
      if (held)
        return no("the phase entry points serve data parallelism; " + variant_ref(v) + verb(v, " uses", " use") + " mdp_update");
      break;
  }
  return std::string();
}
