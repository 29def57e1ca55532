// cycle_select_probe.hip - the host side of csrc/shc_cycle_select.hpp behind a C ABI, for tests/test_cycle_select.py: the feature word
// select_features() picks for every configuration of a morphology, and the feature words its KernelTable lists.  No kernel, no HIP call.
#include "../syropod_highlevel_controller_amd/csrc/shc_cycle_launch.hpp"
#include "../syropod_highlevel_controller_amd/csrc/shc_cycle_select.hpp"

using namespace shc;

// configuration i of the enumeration: bits 0 - 6 the feature switches in the order of their F_* bits, 7 rough_terrain, 8 tip_align,
// 9 gravity_aligned, 10 joint_control == 2, 11 RT_MANUAL_LEGS, 12 the generic flag
constexpr unsigned kConfigurations = 1u << 13;
static unsigned select_configuration(int L, int NJ, unsigned i) {
  CycleParams c{};
  c.manual_posing = i >> 0 & 1, c.auto_posing = i >> 1 & 1, c.inclination_posing = i >> 2 & 1, c.imu_posing = i >> 3 & 1;
  c.admittance_control = i >> 4 & 1, c.tip_force = i >> 5 & 1, c.odometry = i >> 6 & 1;
  c.rough_terrain = i >> 7 & 1, c.tip_align = i >> 8 & 1, c.gravity_aligned = i >> 9 & 1, c.joint_control = (i >> 10 & 1) ? 2 : 0;
  return select_features(L, NJ, c, (i >> 11 & 1) ? RT_MANUAL_LEGS : 0, (i >> 12 & 1) != 0);
}

template <unsigned... Fs>
static int copy_table(uint32_t *out, int capacity, FeatureList<Fs...>) {
  const uint32_t words[] = {Fs...};
  const int n = int(sizeof...(Fs));
  for (int k = 0; k < n && k < capacity; ++k) out[k] = words[k];
  return n;
}

extern "C" int shc_select_probe_configurations() { return int(kConfigurations); }

// out[i] = the feature word of configuration i; -1: the library has no such morphology
extern "C" int shc_select_probe_enumerate(int L, int NJ, uint32_t *out) {
#define X(L_, NJ_) if (L == L_ && NJ == NJ_) { for (unsigned i = 0; i < kConfigurations; ++i) out[i] = select_configuration(L_, NJ_, i); return 0; }
  SHC_FOR_EACH_MORPHOLOGY(X)
#undef X
  return -1;
}

// the feature words of KernelTable<L, NJ> -> how many there are (the first `capacity` of them in out); -1: no such morphology
extern "C" int shc_select_probe_table(int L, int NJ, uint32_t *out, int capacity) {
#define X(L_, NJ_) if (L == L_ && NJ == NJ_) return copy_table(out, capacity, KernelTable<L_, NJ_>{});
  SHC_FOR_EACH_MORPHOLOGY(X)
#undef X
  return -1;
}

// which forms a feature word has in a default build: bit 0 resident, 1 batch, 2 two-wavefront resident, 3 half kernels
extern "C" unsigned shc_select_probe_forms(unsigned F) {
  return (has_resident(F) ? 1u : 0u) | (has_batch(F) ? 2u : 0u) | (has_two_wave(F) ? 4u : 0u) | (has_half_kernels(F) ? 8u : 0u);
}
