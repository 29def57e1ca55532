// shc_cycle_select.hpp - which fused cycle kernel a configuration runs on, and which kernels the library has:
//   select_features(): configuration -> feature word F of the kernel specialisation (the one selection rule);
//   KernelTable<L, NJ>: the feature words a morphology has kernels for (the one instantiation list: shc_cycle_inst.hip builds exactly these);
//   has_*(): which forms (resident, batch, two-wavefront, half kernels) a feature word has.
// Host arithmetic on plain data, no HIP runtime call: tests/test_cycle_select.py enumerates it on a machine without a GPU.
#pragma once

#include "shc_cycle.hpp"

#include <utility>

#ifndef SHC_GENERIC_LOOP_FORMS
#define SHC_GENERIC_LOOP_FORMS 0
#endif

namespace shc {

// the posing sets with feature-exact kernels (dead features cost neither registers nor HBM traffic)
constexpr unsigned F_C2 = F_MANUAL | F_ODOM;                // default.yaml's posing set: BASELINE.json configs 2 / 4
constexpr unsigned F_C3 = F_MANUAL | F_IMU | F_ADM | F_ODOM; // the north-star set (admittance + IMU posing): BASELINE.json config 3
// the BASELINE.json morphologies: default.yaml hexapods (6 x 3) and the synthetic octopods (8 x 5)
constexpr bool is_baseline_morphology(int L, int NJ) { return (L == 6 && NJ == 3) || (L == 8 && NJ == 5); }

// Pick the kernel specialisation: the BASELINE.json configurations get feature-exact kernels; every other flag combination runs a
// runtime-flag kernel (F_DYN).  generic (SHC_FEAT_GENERIC_KERNEL): always a runtime-flag kernel.
static inline unsigned select_features(int L, int NJ, const CycleParams &c, unsigned rt_flags, bool generic) {
  const bool baseline = is_baseline_morphology(L, NJ), exact = !generic;
  const unsigned f = (c.manual_posing ? F_MANUAL : 0) | (c.auto_posing ? F_AUTO : 0) | (c.inclination_posing ? F_INCL : 0) |
                     (c.imu_posing ? F_IMU : 0) | (c.admittance_control ? F_ADM : 0) | (c.tip_force ? F_TIPF : 0) | (c.odometry ? F_ODOM : 0);
  // rough terrain mode / the tip-align pose / manual legs: generic kernels with that logic compiled in - one path each where a
  // configuration needs just one (the usual case), all of them otherwise
  const bool rough = c.rough_terrain != 0, talign = c.tip_align != 0, mlegs = (rt_flags & RT_MANUAL_LEGS) != 0;
  const bool terrain = rough || talign || mlegs;
  // gravity-aligned tips: kernels with the tip-rotation logic compiled in; also a robot with 3-joint legs next to longer ones under
  // joint_control leg manipulation (a MANUAL 3-joint leg holds its FK tip rotation), once a leg has been toggled
  if (NJ > 3 && (c.gravity_aligned || (mlegs && c.joint_control == 2))) {
    if (exact && !terrain) {
      // default.yaml's posing set: feature-exact for every morphology (with the tip-force estimate: the BASELINE morphology only), and with that
      // the two-launch form of the cycle for large launches (has_half_kernels)
      if (f == F_C2) return F_C2 | F_ROT;
      // ... and the north-star feature set together with the tip rotations on the BASELINE octopods: feature-exact, and with that the
      // two-launch form (the runtime-flag kernel below needs one wavefront per SIMD + 122 - 141 AGPRs)
      if (baseline && (f == (F_C2 | F_TIPF) || f == F_C3)) return f | F_ROT;
    }
    return terrain ? F_DYN | F_ROT | F_TERRAIN : F_DYN | F_ROT;
  }
  // joint_control leg manipulation (3-joint legs): a MANUAL leg's tip pose carries its FK rotation, the rotation-constrained IK runs on
  // it (walk_controller.cpp:677-690); only once a leg has been toggled
  if (NJ == 3 && mlegs && c.joint_control == 2) return rough || talign ? F_DYN | F_ROT | F_TERRAIN : F_DYN | F_ROT | F_MLEGS;
  if (terrain) {
    const bool only_rough = rough && !talign && !mlegs, only_mlegs = mlegs && !rough && !talign;
    const bool only_talign = NJ <= 3 && talign && !rough && !mlegs; // (longer legs: tip rotations instead of the tip-align pose)
    // default.yaml's posing set (manual posing + odometry, with / without the tip-force estimate) on the BASELINE morphologies: feature-exact kernels
    if (baseline && exact && (f & ~F_TIPF) == F_C2) {
      if (only_rough) return f | F_ROUGH;
      if (only_talign) return f | F_TALIGN;
    }
    return only_rough ? F_DYN | F_ROUGH : only_mlegs ? F_DYN | F_MLEGS : only_talign ? F_DYN | F_TALIGN : F_DYN | F_TERRAIN;
  }
  if (exact) {
    // every morphology: default.yaml's posing set without the tip-force estimate (what the bins of BASELINE.json configs[4] run on) is
    // feature-exact - the runtime-flag kernels of 8 x 3, 6 x 5 and 8 x 5 carry 12 - 36 B of scratch per lane, these carry none
    if (f == F_C2) return F_C2;
    if (baseline && (f == (F_C2 | F_TIPF) || f == F_C3 || f == (F_C3 | F_TIPF))) return f; // BASELINE.json configs 2 / 4 and 3
  }
  return F_DYN;
}

// ---- the kernels the library has: one list of feature words per morphology class.  shc_cycle_inst.hip instantiates launch_cycle<L, NJ, F> for
//      exactly these and dispatches select_features()'s word over them; a word that is not listed has no kernel.
template <unsigned... Fs>
using FeatureList = std::integer_sequence<unsigned, Fs...>;
template <int L, int NJ>
constexpr auto kernel_table() {
  if constexpr (L == 6 && NJ == 3) // BASELINE hexapods: the 3-joint list + the feature-exact families of configs 2 / 4 and 3
    return FeatureList<F_DYN, F_C3, F_C3 | F_TIPF, F_C2, F_C2 | F_TIPF, F_DYN | F_TERRAIN, F_DYN | F_TALIGN, F_DYN | F_MLEGS, F_DYN | F_ROUGH,
                       F_C2 | F_TALIGN, F_C2 | F_TIPF | F_TALIGN, F_C2 | F_ROUGH, F_C2 | F_TIPF | F_ROUGH, F_DYN | F_ROT | F_MLEGS,
                       F_DYN | F_ROT | F_TERRAIN>{};
  else if constexpr (L == 8 && NJ == 5) // BASELINE octopods: the list of longer legs + the feature-exact families
    return FeatureList<F_DYN, F_C3, F_C3 | F_TIPF, F_C2, F_C2 | F_TIPF, F_DYN | F_TERRAIN, F_DYN | F_MLEGS, F_DYN | F_ROUGH, F_C2 | F_ROUGH,
                       F_C2 | F_TIPF | F_ROUGH, F_DYN | F_ROT, F_DYN | F_ROT | F_TERRAIN, F_C3 | F_ROT, F_C2 | F_TIPF | F_ROT, F_C2 | F_ROT>{};
  else if constexpr (NJ == 3) // 3-joint legs: the tip-align pose; tip rotations only under joint_control leg manipulation
    return FeatureList<F_DYN, F_C2, F_DYN | F_TERRAIN, F_DYN | F_TALIGN, F_DYN | F_MLEGS, F_DYN | F_ROUGH, F_DYN | F_ROT | F_MLEGS,
                       F_DYN | F_ROT | F_TERRAIN>{};
  else // longer legs: tip rotations (gravity-aligned tips), no tip-align pose
    return FeatureList<F_DYN, F_C2, F_DYN | F_TERRAIN, F_DYN | F_MLEGS, F_DYN | F_ROUGH, F_DYN | F_ROT, F_DYN | F_ROT | F_TERRAIN, F_C2 | F_ROT>{};
}
template <int L, int NJ>
using KernelTable = decltype(kernel_table<L, NJ>());

// ---- which forms a specialisation has in this build
// Loop forms.  Manual legs: none (the ManualRobot records change under loop-level calls).  Runtime-flag families: the plain one keeps its
// resident kernels; everything else of F_DYN is opt-in (SHC_GENERIC_LOOP_FORMS) - no test, bench line or fleet bin selects them
// (SHC_KERNEL_LOG over the GPU suite), they are a quarter of the library's kernels and all of them carry scratch.
constexpr bool has_resident(unsigned F) { return (F & F_MLEGS) == 0 && (SHC_GENERIC_LOOP_FORMS || (F & F_DYN) == 0 || (F & (F_TERRAIN | F_ROT)) == 0); }
constexpr bool has_batch(unsigned F) { return (F & F_MLEGS) == 0 && (SHC_GENERIC_LOOP_FORMS || (F & F_DYN) == 0); }
// Rough terrain and tip rotations run as ONE wavefront per robot group (Leg::applyIK feeds back into the stepper there - touchdown detection,
// the FK tip rotation - so the walker / model halves cannot be pipelined); every other resident kernel also has the two-wavefront form.
constexpr bool has_two_wave(unsigned F) { return has_resident(F) && (F & (F_TERRAIN | F_ROT)) == 0; }
// ... and default.yaml's posing set on the BASELINE hexapods also the helper forms of it (helper wavefronts take the velocity front off the walker and the pose,
// the odometry and the leader's duty off the model wavefront: four roles in 512-thread workgroups, three in 384-thread ones, shc_cycle_kernel.hpp)
constexpr bool has_helper_wave(int L, int NJ, unsigned F) { return L == 6 && NJ == 3 && (F == F_C2 || F == (F_C2 | F_TIPF)); }
// Rotation-constrained cycles of the feature-exact kernels: a cycle can run as the walker / poser launch + the model launch
constexpr bool has_half_kernels(unsigned F) { return (F & F_ROT) != 0 && (F & (F_DYN | F_TERRAIN | F_MLEGS | F_AUTO)) == 0; }

} // namespace shc
