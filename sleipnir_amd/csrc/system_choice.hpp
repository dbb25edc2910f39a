// Which plan a system gets and which kernels serve it, decided in one place: pure host code — no device, no look at
// the environment (switches.hpp has been read by then) — so that the CPU tier checks every decision
// (tests/test_system_choice_cpu.py).  NewtonSystem's constructors choose options and plan here; DeviceNlp measures what
// fits on its device and has the stages below turn that into its LaunchModes, which nothing else writes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ldlt_symbolic.hpp"
#include "switches.hpp"

namespace slpx {

// ---- the plan ----

// Lane-per-problem (ldlt_il_kernels.h) pays from one 64-problem chunk per task on (r02: from ~200 problems — the
// backward solve was one wave per task and chunk, a chain of columns; with the columns of a level dealt to four
// waves, 64 x N=500: 251 k steps/s against 224-238 k for the per-task kernels, profiles/r03_b64_probe.txt;
// 512 x N=1000: 508 k vs 171 k).  SLPX_LDLT_IL=0 turns it off, SLPX_IL_MIN_BATCH moves the threshold.
bool interleaved_for(int batch, const Switches& sw);

// The options of the symbolic factorization of `batch` systems of order `dim`, from the caller's.  compiled_model =
// false (the linear-solver seam): the three batch rules only.
LdltOptions choose_ldlt_options(const LdltOptions& base, int batch, int dim, bool compiled_model, const Switches& sw);
// ... and those of the pair-list kernels for a system whose fronts were asked for (`chosen`) and not built
LdltOptions pair_list_options(const LdltOptions& base, const LdltOptions& chosen);

constexpr int kDenseMaxOrder = 8192;            // 512 MB of factors per problem, two columns in LDS
constexpr int kReferenceDenseMaxOrder = 2048;   // the reference's density rule is followed up to here
// the whole batch's dense factors, batch x dim x dim doubles, within reach of one device (64 GB): throws beyond
void require_dense_factors_fit(int batch, int dim);

// The plan.  In this order: the reference's density rule (`reference_takes_dense`: KktPlan::reference_takes_dense; no
// caller's permutation, SLPX_DENSE not 0, order <= 2048) -> dense with diagonal pivoting (SLPX_DENSE=1: without);
// SLPX_DENSE=1 -> dense; the sparse build with `options`; where a column of L does not fit the LDS of a task (and
// SLPX_DENSE is not 0) -> dense; where `pair_retry` is given, fronts were asked for and not built -> the build again
// with those options.  Every dense route passes require_dense_factors_fit.  dense_because (optional): what the sparse
// build said where the plan is dense for it.
LdltPlan choose_ldlt_plan(const CscPattern& lhs, int n_dec, bool reference_takes_dense, const std::vector<int32_t>* user_perm,
                          const std::vector<uint8_t>* diag_has_source, int batch, const LdltOptions& options,
                          const LdltOptions* pair_retry, const Switches& sw, std::string* dense_because = nullptr);

// ---- the launch modes ----

// What the choice reads of a plan (DeviceNlp fills it from its LdltPlan)
struct PlanFacts {
  bool dense = false, dense_pivoted = false;
  size_t tasks = 0;
  uint32_t factor_lds_bytes = 0;
  bool mf = false;             // the fronts were built
  uint32_t mf_n_mfma = 0;      // ... of them on the matrix cores
  bool update_slots_have_one_reader = false;  // device_images.hpp
};

struct LaunchModes {
  bool dense = false, dense_pivoted = false;  // the dense branch (ldlt_dense_kernels.h), with diagonal pivoting
  bool il = false;                // batch-interleaved LDLT (ldlt_il_kernels.h)
  // all rounds of a factorization / backward solve in one launch (device-side round counters, double-buffered like
  // the inertia counters); SLPX_SINGLE_LAUNCH=0 disables
  bool single_launch = true;
  bool fuse_launches = false;     // KKT assembly inside the factorization launch, back-substitution inside the solve's
  bool fuse_kkt = false, fuse_backsub = false;  // the two halves of it (SLPX_FUSE_KKT, SLPX_FUSE_BACKSUB)
  bool fuse_kkt_store = false;
  bool fuse_solve = false;        // factorization and solve of a step in one launch (ldlt_mf_step_kernel)
  bool slot_handoff = false;      // factorization rounds hand over through the update block slots
  bool xg_by_data = false;        // backward solve: x of finished columns handed to the descendants through the values
  // multifrontal step (ldlt_mf_kernels.h: ldlt_mf_step_kernel; SLPX_LDLT_MF=0: the pair lists)
  bool mf = false;
  bool mf_solve = false;          // a new right-hand side goes through the fronts too (ldlt_mf_solve_kernel; SLPX_MF_SOLVE=0: the pair lists)
  bool mf_mfma = false;           // the plan has fronts on the matrix cores: the kernel variant with that path
  int mf_threads = 1024;          // 512 where the 1024-thread workgroups of every task are not resident at once
  int twin_threads = 1024;        // ... of a launch of two attempts
  int chain_mode = 0;             // TapeJitOptions::chain_mode the full tape's kernel is generated with
  bool chain_on = false;          // chained steps (DeviceNlp::sweep_full_for_step)
  int twin = 0;                   // 0: not looked at yet, 1: available, -1: not (not resident at once, SLPX_TWIN=0, ...)
  int ride = -1;                  // the riding error launch fits beside both attempts' tasks (-1: not asked yet)
};

// Workgroups of a kernel the device holds at once, by workgroup size (0: not asked, or none)
struct Residency {
  size_t at_1024 = 0, at_512 = 0;
};

// From the plan's shape and the batch, and the switches that overrule it.  n_sums: the tape's separable sums (their
// workgroups ride in the step kernel's launch); cus: compute units of the device.
LaunchModes initial_launch_modes(int batch, const PlanFacts& plan, size_t n_sums, int cus, const Switches& sw);
// After the inline images: a pack that failed sends its half to the stand-alone kernels
void note_inline_images(LaunchModes& m, bool kkt_ok, bool backsub_ok);
// Whether the task images of the multifrontal step are to be made at all
bool wants_multifrontal(const LaunchModes& m, const PlanFacts& plan, const Switches& sw);
// The multifrontal step: every task's workgroup (and the sums') resident at once — `step`, the smaller of the step
// kernel's variants; `solve`: ldlt_mf_solve_kernel — with no static LDS in front of the dynamic block (the tables hold
// LDS byte addresses from 0).  Sets mf, mf_mfma, mf_threads, mf_solve, fuse_solve, chain_on.
struct MfFit {
  bool declined = true;      // the images were not made (wants_multifrontal said no, or the packer declined)
  uint32_t lds_bytes = 0;    // of a task image
  size_t static_lds_bytes = 0;
  Residency step, solve;
};
void choose_multifrontal(LaunchModes& m, const PlanFacts& plan, size_t n_sums, const MfFit& fit, const Switches& sw);
// A launch of two attempts (ldlt_mf_twin_kernel): decided on first use, where its buffers are made.  Sets twin and
// twin_threads.  (twin_worth_measuring: what choose_twin asks before it looks at `twin` — false spares the queries.)
bool twin_worth_measuring(const LaunchModes& m, int batch, const Switches& sw);
void choose_twin(LaunchModes& m, int batch, const PlanFacts& plan, size_t n_sums, const Residency& twin, const Switches& sw);
// ... and the deciding error launch riding in it: both attempts' tasks, the sums and its 64 workgroups at once
// (`riding`: ldlt_mf_twin_kernel<twin_threads, true> at the larger of the two LDS sizes).  Sets ride.
size_t riding_workgroups(const PlanFacts& plan, size_t n_sums);
void choose_ride(LaunchModes& m, const PlanFacts& plan, size_t n_sums, size_t riding, const Switches& sw);
// the device showed that kernels of two streams do not run at once, or a chained step lost its hand-over
inline void unchain(LaunchModes& m) { m.chain_on = false; }

}  // namespace slpx
