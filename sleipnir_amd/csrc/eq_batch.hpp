// Batched whole solves of models without inequality constraints: B instances of one compiled model in lockstep, as
// interior_point_batch (ipm_batch.hpp) runs the others.  An unconstrained model follows the Newton iteration
// (newton.hpp:51-292), an equality-constrained one the SQP iteration (sqp.hpp:98-604), each instance as Problem::solve()
// would from its start: its own problem scaling, filter, full-step-rejection counter, δ/γ memory, iteration count and
// exit, its decisions taken by the shared host code (ipm_line_search.hpp, ipm_decide.h) from a few scalars.  The
// iterate (x, y), the trial point, the directions and the correction's accumulator stay on the device (BatchEqDevice);
// every piece of device work is one masked launch for the instances that want it at that point.
//
// Feasibility restoration (SQP only) runs on the problem's batch-1 system, one instance at a time, as in the
// interior-point batch.
#pragma once

#include <cstdint>
#include <vector>

#include "ipm_batch.hpp"

namespace slpx {

// The device side (launch wrappers beside those of BatchIpmDevice in ipm_batch_launch.hip; kernels: eq_batch_kernels.h,
// and batch_errors_kernel / batch_scale_V_kernel / batch_load_state_kernel of ipm_batch_kernels.h, which compute exactly
// what is needed here when m_i = 0).  Buffers are batch-major; launches take effect for the instances flagged in
// `active` only.
struct BatchEqDevice {
  explicit BatchEqDevice(NewtonSystem& sys);
  NewtonSystem& sys;
  int B, n, m_e, dim, ns, nV;
  // per-instance parameters, host side; upload() sends them with `active` (one synchronization)
  std::vector<double> alpha, alpha_soc;
  std::vector<int32_t> mode;            // trial direction: 0 Newton, 1 second-order correction
  std::vector<uint8_t> first, active;   // first: the correction's accumulator starts from c_e
  void upload();
  void set_scales(const std::vector<double>& scales);                                // [B][1 + m_e]
  void set_iterate(const std::vector<double>& x, const std::vector<double>& y);      // all instances
  void get_iterate(std::vector<double>& x, std::vector<double>& y);
  // one instance (feasibility restoration hand-off): its iterate, and its current V
  void get_instance(int b, std::vector<double>& x, std::vector<double>& y, std::vector<double>& V);
  void put_instance(int b, const std::vector<double>& x, const std::vector<double>& y);

  // the full tape at the iterate, scaled; the system's y, V are then the iterate's (what the Newton step reads), a
  // copy of V is kept as the current point's, and the errors are reduced -> err [B][kBatchErrN]
  void refresh(std::vector<double>& err);
  void direction(std::vector<double>& dphi);  // after compute(): keep p_x, p_y = -p[n..]; dphi [B] = g . p_x
  // trial point (x, y) + alpha d, d = Newton's (mode 0) or the correction's (mode 1), value sweep -> met [B][3]
  // (f, ||c_e||_1, count of non-finite f, c_e)
  void trial_values(std::vector<double>& met);
  void soc_step();  // second-order correction: rhs, solve on the instance's factor, its direction
  // KKT-error fallback: errors at the current point, then a full sweep at (x, y) + alpha p and its errors
  void kkt_fallback(std::vector<double>& err_cur, std::vector<double>& err_trial);
  void commit();

 private:
  friend struct BatchEqProbe;  // (the test-only probe, tests/support/eqbatchcheck.cpp, reads the buffers below)
  DevBuf<int32_t> m_scale_idx, m_mode;
  DevBuf<uint8_t> m_is_static, m_active, m_first;
  DevBuf<double> m_static_raw, m_scales, m_alpha, m_alpha_soc, m_zero, m_none, m_out;
  DevBuf<double> m_x, m_y, m_tx, m_ty, m_px, m_py, m_sx, m_sy;  // iterate, trial, Newton direction, correction's
  DevBuf<double> m_Vcur, m_tce, m_sce;
  void scale_V(int count);
  void errors(const double* V, bool trial, std::vector<double>& err);
  void launch_trial(int with_duals);
  void download_out(size_t per_instance, std::vector<double>& out);
};

// Arguments as interior_point_batch: x0 = [B][n]; scales = [B][1 + m_e]; run[b] = 0: instance b is not solved here.
// `sys` is the batch system (tape at unit scales), `single` the batch-1 system of the same model (restoration).
// sqp_batch: m_i == 0 and m_e > 0.  newton_batch: m_e == m_i == 0.
void sqp_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
               const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out);
void newton_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
                  const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out);

}  // namespace slpx
