// The device side of the batched interior-point driver (batch_lockstep.hpp: the loop and the state every batched
// driver shares).
#pragma once

#include "batch_lockstep.hpp"

namespace slpx {

// What the interior-point iteration adds to BatchDevice (ipm_batch_launch.hip, kernels: ipm_batch_kernels.h): s and z
// of the iterate, the trial point and the correction, the Newton direction, the second-order correction's
// accumulators, and the barrier's per-instance parameters.
struct BatchIpmDevice : BatchDevice {
  explicit BatchIpmDevice(NewtonSystem& sys);
  std::vector<double> mu, tau, alpha_z;
  std::vector<uint8_t> s_from_ci;
  void upload();  // these four, then BatchDevice's (one synchronization)

  void newton_direction(std::vector<double>& dir);     // after compute(): keep p, p_s, p_z; dir [B][3]
  // trial point along the Newton (mode 0) or correction (mode 1) direction, value sweep, metrics -> met [B][4]
  void trial_values(std::vector<double>& met);
  // second-order correction: rhs, solve on the instance's factor, direction -> sd [B][2] (alpha_soc, alpha_z_soc)
  void soc_step(std::vector<double>& sd);
  // KKT-error fallback: errors at the current point, then full sweep at the full step and its errors
  void kkt_fallback(std::vector<double>& err_cur, std::vector<double>& err_trial);
  void commit();

 private:
  friend struct BatchIpmProbe;  // (the test-only probe, tests/support/batchcheck.cpp, reads the buffers)
  DevBuf<uint8_t> m_s_from_ci;
  DevBuf<double> m_mu, m_tau, m_alpha_z;
  DevBuf<double> m_s, m_z, m_ts, m_tz, m_ss, m_sz;  // iterate, trial, correction
  DevBuf<double> m_p, m_ps, m_pz, m_tci, m_scims, m_t;
  void launch_trial(int with_duals);
};

}  // namespace slpx
