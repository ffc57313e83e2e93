// Host-only table of mdp_variants.h's refusal() over the variants x seams matrix
// (make -C maddpg_amd/csrc variant-check).  One JSON object: "<state> | <entry
// point>" -> the refusal text, or null where the gate lets the call go on.  The
// states and their names are those of tools/variant_matrix.py, which recorded
// tests/golden/variant_matrix.json from the library; tests/test_variant_gate.py
// compares the two.
#include <cstdio>
#include <string>

#include "mdp_variants.h"

namespace {

struct Row {
  const char* name;
  GateState s;
};

GateState state(Variant v, bool box = false, bool trained = false, int mode = 0, bool world = false) {
  GateState s;
  s.variant = v;
  s.box = box;
  s.trained = trained;
  s.update_mode = mode;
  s.dp_world = world;
  return s;
}

std::string quoted(const std::string& s) {
  std::string q = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') q += '\\';
    q += c;
  }
  return q + "\"";
}

}  // namespace

int main() {
  const Row rows[] = {
      {"plain", state(Variant::None)},
      {"prioritized", state(Variant::Per)},
      {"MATD3", state(Variant::Td3)},
      {"M3DDPG", state(Variant::Minimax)},
      {"inferred policies", state(Variant::Approx)},
      {"Box agent", state(Variant::None, true)},
      {"throughput mode", state(Variant::None, false, false, 1)},
      {"plain after one update", state(Variant::None, false, true)},
      {"plain, world_size 2", state(Variant::None, false, false, 0, true)},
  };
  bool first = true;
  const auto cell = [&](const Row& r, const char* fn, const std::string& why) {
    std::printf("%s\n %s: %s", first ? "{" : ",", quoted(std::string(r.name) + " | " + fn).c_str(),
                why.empty() ? "null" : quoted(why).c_str());
    first = false;
  };
  for (const Row& r : rows) {
    for (int v = 1; v < kVariantCount; ++v) cell(r, kVariants[v].enable, refusal(r.s, Seam::Enable, (Variant)v));
    for (int k = 1; k < kSeamCount; ++k) cell(r, kSeams[k].fn, refusal(r.s, (Seam)k));
  }
  std::printf("\n}\n");
  return 0;
}
