// TEST INFRASTRUCTURE ONLY: the stages of csrc/system_choice.hpp in the order DeviceNlp runs them, on numbers handed
// in — what the device would have measured among them.  Shared by the ctypes library (choicecheck.cpp) and the
// stand-alone program (choicecheck_main.cpp).  The names of both rows are in choicecheck.py (MODES_IN, MODES_OUT).
#pragma once

#include <cstdint>

#include "../../sleipnir_amd/csrc/system_choice.hpp"

namespace choicecheck {

constexpr int kModesIn = 24, kModesOut = 20;

inline void run_modes(const int64_t* in, int64_t* out) {
  using namespace slpx;
  const Switches sw = Switches::from_environment();
  const int batch = static_cast<int>(in[0]);
  PlanFacts plan;
  plan.dense = in[1] != 0;
  plan.dense_pivoted = in[2] != 0;
  plan.tasks = static_cast<size_t>(in[3]);
  plan.factor_lds_bytes = static_cast<uint32_t>(in[4]);
  plan.mf = in[5] != 0;
  plan.mf_n_mfma = static_cast<uint32_t>(in[6]);
  plan.update_slots_have_one_reader = in[7] != 0;
  const size_t n_sums = static_cast<size_t>(in[8]);
  LaunchModes m = initial_launch_modes(batch, plan, n_sums, static_cast<int>(in[9]), sw);
  note_inline_images(m, in[10] != 0, in[11] != 0);
  MfFit fit;
  fit.declined = in[12] != 0 || !wants_multifrontal(m, plan, sw);
  fit.lds_bytes = static_cast<uint32_t>(in[13]);
  fit.static_lds_bytes = static_cast<size_t>(in[14]);
  fit.step = Residency{static_cast<size_t>(in[15]), static_cast<size_t>(in[16])};
  fit.solve = Residency{static_cast<size_t>(in[17]), static_cast<size_t>(in[18])};
  choose_multifrontal(m, plan, n_sums, fit, sw);
  if (in[19] != 0) choose_twin(m, batch, plan, n_sums, Residency{static_cast<size_t>(in[20]), static_cast<size_t>(in[21])}, sw);
  if (in[22] != 0 && m.twin > 0) choose_ride(m, plan, n_sums, static_cast<size_t>(in[23]), sw);
  const int64_t o[kModesOut] = {m.dense, m.dense_pivoted, m.il, m.single_launch, m.fuse_launches, m.fuse_kkt, m.fuse_backsub,
                                m.fuse_kkt_store, m.fuse_solve, m.slot_handoff, m.xg_by_data, m.mf, m.mf_solve, m.mf_mfma,
                                m.mf_threads, m.twin_threads, m.chain_mode, m.chain_on, m.twin, m.ride};
  for (int i = 0; i < kModesOut; ++i) out[i] = o[i];
}

}  // namespace choicecheck
