// shc_cycle_inst.hip - the fused cycle kernels of ONE morphology (compile with -DSHC_INST_L=<legs> -DSHC_INST_NJ=<joints> -DSHC_INST_PART=<0|1>):
// libshc_batch.so links two objects of this file per supported (legs, joints), built in parallel (engine.py build_library) -
//   part 0: the launch forms (shc_cycle_kernel, the half kernels of rotation-constrained cycles) and the morphology's entry point shc_launch_cycle_L_NJ;
//   part 1: the loop forms (shc_resident_kernel, shc_resident2_kernel, shc_batch_kernel) behind shc_launch_loop_L_NJ, which part 0 hands loop launches to.
// Both parts run the same selection (shc_cycle_select.hpp: select_features, configuration -> feature word) over the same list (KernelTable: the
// feature words this morphology has kernels for); each instantiates only its own forms of them.
// -DSHC_GENERIC_LOOP_FORMS=1 (engine.py: SHC_GENERIC_LOOP_FORMS=1 in the environment of the build) adds the loop forms of the runtime-flag (F_DYN) families
// that the default build leaves out: their batch kernels (shc_engine_step_k then runs such a configuration as K single launches - same results, see
// shc_resident.hpp) and the resident kernels of F_DYN with rough terrain / tip-align / tip rotations (resident_begin reports SHC_ERR_UNSUPPORTED).
#include "shc_cycle_kernel.hpp"
#include "shc_cycle_select.hpp"

#if !defined(SHC_INST_L) || !defined(SHC_INST_NJ) || !defined(SHC_INST_PART)
#error "compile with -DSHC_INST_L=<legs> -DSHC_INST_NJ=<joints> -DSHC_INST_PART=<0|1>"
#endif

#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <tuple>

namespace shc {

// Development aid: SHC_KERNEL_LOG=<file> appends one line per kernel specialisation this process launches ("form legs joints features"), the
// first time it is launched - which of the library's instantiations a test suite / a bench run actually exercises (scripts/kernels_used.py).
static void note_kernel(const char *form, int legs, int joints, unsigned features) {
  static const char *path = std::getenv("SHC_KERNEL_LOG");
  if (!path) return;
  static std::mutex mu;
  static std::set<std::tuple<const char *, unsigned>> seen;
  std::lock_guard<std::mutex> lock(mu);
  if (!seen.insert({form, features}).second) return;
  if (FILE *f = std::fopen(path, "a")) {
    std::fprintf(f, "%s %d %d %u\n", form, legs, joints, features);
    std::fclose(f);
  }
}

template <int L, int NJ, unsigned F>
static void launch_cycle(const CycleLaunch &a) {
  constexpr int RPW = 64 / L;
  constexpr size_t wave_bytes = size_t(RobotFields::COUNT * RPW + PK_COUNT * 64 + (RobotFields::I_COUNT * RPW + 1) / 2) * 8;
#if SHC_INST_PART == 1
  // Resident kernels: every specialisation but manual legs (the tip-align pose of gravity_aligned_tips on <= 3-joint legs is per-robot state of the
  // tile like any other and has had a loop form since round 5); which of them also has the two-wavefront form: has_two_wave.
  if (a.fit) {
    a.fit->supported = has_resident(F) ? 1 : 0;
    a.fit->batch = has_batch(F) ? 1 : 0;
    a.fit->two_wave = has_two_wave(F) ? 1 : 0;
    a.fit->helper_wave = has_helper_wave(L, NJ, F) ? 1 : 0;
    a.fit->blocks_per_cu = 0;
    if constexpr (has_resident(F)) {
      int blocks = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, shc_resident_kernel<L, NJ, F>, 64, wave_bytes) != hipSuccess) blocks = 0;
      a.fit->blocks_per_cu = blocks;
    }
  } else if (a.resident->batch_cycles != 0) { // shc_engine_step_k: the batch form, a kernel of its own
    if constexpr (has_batch(F)) {
      note_kernel("batch", L, NJ, F);
      shc_batch_kernel<L, NJ, F><<<dim3(a.grid), dim3(a.block), wave_bytes * (a.block / 64), a.stream>>>(a.st, (const SharedConsts<L, NJ> *)a.consts, *a.resident, a.rt_flags);
    }
  } else if (a.block == 512) { // the helper form: four roles (logged as "resident3", the name the helper form has had since it had one helper)
    if constexpr (has_helper_wave(L, NJ, F)) {
      static_assert(has_two_wave(F), "the helper forms are forms of the two-wavefront pipeline");
      note_kernel("resident3", L, NJ, F);
      shc_resident2_kernel<L, NJ, F, 2><<<dim3(a.grid), dim3(512), 2 * wave_bytes + sizeof(Resident3Lds<L, NJ>), a.stream>>>(
          a.st, (const SharedConsts<L, NJ> *)a.consts, *a.resident, a.rt_flags);
    }
  } else if (a.block == 384) { // its three-role predecessor, one helper wavefront per robot group: grids that leave the four-role form no room, and SHC_RESIDENT_THREE_ROLE=1
    if constexpr (has_helper_wave(L, NJ, F)) {
      note_kernel("resident3_one_helper", L, NJ, F);
      shc_resident2_kernel<L, NJ, F, 1><<<dim3(a.grid), dim3(384), 2 * wave_bytes + sizeof(Resident3Lds<L, NJ>), a.stream>>>(
          a.st, (const SharedConsts<L, NJ> *)a.consts, *a.resident, a.rt_flags);
    }
  } else if (a.block == 256) {
    if constexpr (has_two_wave(F)) {
      note_kernel("resident2", L, NJ, F);
      shc_resident2_kernel<L, NJ, F><<<dim3(a.grid), dim3(256), 2 * wave_bytes + sizeof(Resident2Lds<L, NJ>), a.stream>>>(
          a.st, (const SharedConsts<L, NJ> *)a.consts, *a.resident, a.rt_flags);
    }
  } else {
    if constexpr (has_resident(F)) {
      note_kernel("resident", L, NJ, F);
      shc_resident_kernel<L, NJ, F><<<dim3(a.grid), dim3(64), wave_bytes, a.stream>>>(a.st, (const SharedConsts<L, NJ> *)a.consts, *a.resident, a.rt_flags);
    }
  }
#else
  // Rotation-constrained cycles of the feature-exact kernels: one cycle = the walker / poser launch + the model launch (two wavefronts per SIMD
  // each instead of one) once the launch holds at least two wavefronts for every SIMD of the chip; smaller launches stay one kernel.
  if constexpr (has_half_kernels(F)) {
    const int64_t waves = int64_t(a.grid) * (a.block / 64);
    if (a.half_steps >= 0 && (a.half_steps > 0 || waves >= 2048)) {
      note_kernel("half", L, NJ, F);
      for (int c = 0; c < a.n_cycles; ++c) {
        shc_cycle_half_kernel<L, NJ, F, ROLE_FRONT><<<dim3(a.grid), dim3(a.block), wave_bytes * (a.block / 64), a.stream>>>(
            a.st, (const SharedConsts<L, NJ> *)a.consts, a.rt_flags, a.wave0);
        shc_cycle_half_kernel<L, NJ, F, ROLE_BACK><<<dim3(a.grid), dim3(a.block), wave_bytes * (a.block / 64), a.stream>>>(
            a.st, (const SharedConsts<L, NJ> *)a.consts, a.rt_flags, a.wave0);
      }
      return;
    }
  }
  note_kernel("cycle", L, NJ, F);
  shc_cycle_kernel<L, NJ, F><<<dim3(a.grid), dim3(a.block), wave_bytes * (a.block / 64), a.stream>>>(a.st, (const SharedConsts<L, NJ> *)a.consts, a.n_cycles,
                                                                                              a.rt_flags, a.wave0);
#endif
}

// The kernel select_features() names, out of this morphology's list.  false: the selection named a feature word the list lacks (the two
// are pinned to each other by tests/test_cycle_select.py) - nothing was launched, the caller reports it.
template <int L, int NJ, unsigned... Fs>
static bool launch_selected(const CycleLaunch &a, FeatureList<Fs...>) {
  const unsigned f = select_features(L, NJ, *a.cp, a.rt_flags, a.generic);
  return ((f == Fs && (launch_cycle<L, NJ, Fs>(a), true)) || ...);
}

#define SHC_CAT3(a, b, c) a##b##_##c
#define SHC_LAUNCHER_NAME(L_, NJ_) SHC_CAT3(shc_launch_cycle_, L_, NJ_)
#define SHC_LOOP_LAUNCHER_NAME(L_, NJ_) SHC_CAT3(shc_launch_loop_, L_, NJ_)
#if SHC_INST_PART == 1
bool SHC_LOOP_LAUNCHER_NAME(SHC_INST_L, SHC_INST_NJ)(const CycleLaunch &a) { return launch_selected<SHC_INST_L, SHC_INST_NJ>(a, KernelTable<SHC_INST_L, SHC_INST_NJ>{}); }
#else
bool SHC_LOOP_LAUNCHER_NAME(SHC_INST_L, SHC_INST_NJ)(const CycleLaunch &a);
bool SHC_LAUNCHER_NAME(SHC_INST_L, SHC_INST_NJ)(const CycleLaunch &a) {
  if (a.fit || a.resident) return SHC_LOOP_LAUNCHER_NAME(SHC_INST_L, SHC_INST_NJ)(a); // a loop form (or the question whether there is one): the other object of this morphology
  return launch_selected<SHC_INST_L, SHC_INST_NJ>(a, KernelTable<SHC_INST_L, SHC_INST_NJ>{});
}
#endif

} // namespace shc
