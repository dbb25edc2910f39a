// The behavioural environment variables of DESIGN.md §8, read once: NewtonSystem's constructors call
// Switches::from_environment(), keep the result (NewtonSystem::switches()) and hand it to DeviceNlp; nothing after that
// looks at the environment for any of these names.  A switch is `env[0] != '0'`, a number is atoi — nothing stricter.
// Not here, and read where they are used: the tape compiler's and the tape JIT's own switches (SLPX_TAPE_*,
// SLPX_HESSIAN_FAMILIES), the cache directories, SLPX_SETUP_THREADS and every diagnostic (*_VERBOSE, *_TIMING, *_DEBUG*,
// *_DUMP*).
#pragma once

#include <cstdint>
#include <optional>

namespace slpx {

struct Switches {
  // paths (default on; "0..." selects the other one — the table of DESIGN.md §8)
  bool fuse_launches = true;  // SLPX_FUSE_LAUNCHES
  bool fuse_kkt = true;       // SLPX_FUSE_KKT
  bool fuse_backsub = true;   // SLPX_FUSE_BACKSUB
  bool ldlt_mf = true;        // SLPX_LDLT_MF
  bool ldlt_il = true;        // SLPX_LDLT_IL
  bool chain_tape = true;     // SLPX_CHAIN_TAPE
  bool ipm_resident = true;   // SLPX_IPM_RESIDENT
  bool ipm_lookahead = true;  // SLPX_IPM_LOOKAHEAD
  bool ipm_pipeline = true;   // SLPX_IPM_PIPELINE
  bool twin = true;           // SLPX_TWIN
  bool ipm_ride = true;       // SLPX_IPM_RIDE
  bool mf_solve = true;       // SLPX_MF_SOLVE
  bool fuse_kkt_store = false;  // SLPX_FUSE_KKT_STORE (default off)
  int il_min_batch = 64;        // SLPX_IL_MIN_BATCH
  // unset is a third state
  std::optional<bool> dense;  // SLPX_DENSE: "0..." always sparse, "1..." dense without pivoting, anything else as unset (the reference's 25 % rule)
  std::optional<uint32_t> task_entries;  // SLPX_TASK_ENTRIES (unset: the computed size, and single_problem_task_rules)
  std::optional<bool> single_launch;     // SLPX_SINGLE_LAUNCH: overrules the computed choice in both directions
  std::optional<int> mf_threads;         // SLPX_MF_THREADS: anything but 1024 keeps the step kernel off 1024-thread workgroups
  std::optional<int> relax_zeros;        // SLPX_RELAX_ZEROS
  std::optional<int> sn_min_width;       // SLPX_SN_MIN_WIDTH
  std::optional<uint32_t> mfma_min_entries;  // SLPX_MFMA_MIN_ENTRIES

  static Switches from_environment();
};

}  // namespace slpx
