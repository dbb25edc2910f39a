// Batched whole solves: B instances of one compiled model, each from its own initial guess, with the
// options and the compiled structure shared.  Every instance follows the interior-point iteration
// (interior_point.hpp:129-878) as Problem::solve() would from its start, its decisions taken by the code the
// single-problem drivers share (ipm_line_search.hpp, ipm_decide.h) — its own
// problem scaling, barrier parameter, filter, δ/γ memory, full-step-rejection counter, iteration count and
// exit — while the device work of all instances still iterating runs as ONE batched launch per phase:
// the AD sweeps, the KKT build, the regularized factorization (NewtonSystem::compute with an instance
// mask), the solves, and every O(n) piece around them (ipm_batch_kernels.h).
//
// The loop runs in lockstep: one Newton step for every running instance, then the line search in rounds —
// each round one masked launch of value sweeps (and of second-order-correction solves, and of the full
// sweeps of the KKT-error fallback) for the instances still searching.  The vectors stay on the device;
// the host reads a few scalars per instance and decides.  An instance that has finished is frozen: the
// new kernels skip it by its active flag.
//
// Feasibility restoration runs on the problem's own batch-1 system (`single`), one instance at a time,
// with that instance's scaling, iterate, barrier parameter, δ/γ memory and filter; the result is written
// back into the batch state.
#pragma once

#include <cstdint>
#include <vector>

#include "ipm.hpp"

namespace slpx {

// the per-instance scalars of batch_errors_kernel (out[b * kBatchErrN + k]); see ipm_batch.cpp for their use
enum BatchErr {
  BE_F = 0,
  BE_DUAL_INF, BE_DUAL_1, BE_Y1, BE_Z1, BE_SZ_MAX, BE_SZ_MIN, BE_COMP_1, BE_CE_INF, BE_CE_1, BE_CIS_INF, BE_CIS_1,
  BE_DUALU_INF, BE_YU1, BE_ZU1, BE_COMPU_INF, BE_CEU_INF, BE_CISU_INF,
  BE_LOGSUM, BE_V_BAD, BE_CI_NONPOS, BE_AETCE2, BE_CE2, BE_AITCM2, BE_CM2, BE_X_INF, BE_X_BAD, BE_S_INF, BE_S_BAD,
  kBatchErrN
};
constexpr int kBatchErrReduced = kBatchErrN - 1;  // all but BE_F

// the reductions of batch_errors_kernel (one instance's BatchErr) as the fields the shared decisions read
inline IpmErrOut err_of(const double* e) {
  IpmErrOut o{};
  o.dual_inf_u = e[BE_DUALU_INF], o.sz_max_u = e[BE_COMPU_INF], o.ce_inf_u = e[BE_CEU_INF], o.cis_inf_u = e[BE_CISU_INF];
  o.y1_u = e[BE_YU1], o.z1_u = e[BE_ZU1];
  o.dual_inf = e[BE_DUAL_INF], o.sz_min = e[BE_SZ_MIN], o.sz_max = e[BE_SZ_MAX], o.ce_inf = e[BE_CE_INF], o.cis_inf = e[BE_CIS_INF];
  o.y1 = e[BE_Y1], o.z1 = e[BE_Z1];
  o.f = e[BE_F], o.viol = e[BE_CE_1] + e[BE_CIS_1], o.logsum = e[BE_LOGSUM];
  o.aetce_sq = e[BE_AETCE2], o.ce_sq = e[BE_CE2], o.aitcp_sq = e[BE_AITCM2], o.cp_sq = e[BE_CM2];
  o.x_inf = e[BE_X_INF], o.s_inf = e[BE_S_INF];
  o.finite = e[BE_X_BAD] == 0.0 && e[BE_S_BAD] == 0.0 ? 1.0 : 0.0;
  o.ci_all_pos = e[BE_CI_NONPOS] == 0.0 ? 1.0 : 0.0;
  return o;
}
inline double error_one_norm(const double* e) { return e[BE_DUAL_1] + e[BE_COMP_1] + e[BE_CE_1] + e[BE_CIS_1]; }

// The device side of the batched driver (ipm_batch_launch.hip, kernels: ipm_batch_kernels.h): the iterate, the
// trial point, the directions and the second-order correction's accumulators of every instance, batch-major, and the
// per-instance parameters of a launch.  Launches take effect for the instances flagged in `active` only.
struct BatchIpmDevice {
  explicit BatchIpmDevice(NewtonSystem& sys);
  NewtonSystem& sys;
  int B, n, m_e, m_i, dim, ns, nV;
  // per-instance parameters, host side; upload() sends them with `active` (one synchronization)
  std::vector<double> mu, tau, alpha, alpha_z, alpha_soc;
  std::vector<int32_t> mode;                   // trial direction: 0 Newton, 1 second-order correction
  std::vector<uint8_t> s_from_ci, first, active;
  void upload();
  void set_scales(const std::vector<double>& scales);  // [B][1 + m_e + m_i]
  void set_iterate(const std::vector<double>& x, const std::vector<double>& s, const std::vector<double>& y,
                   const std::vector<double>& z);      // all instances
  void get_iterate(std::vector<double>& x, std::vector<double>& s, std::vector<double>& y, std::vector<double>& z);
  // one instance (feasibility restoration hand-off): its iterate, and its current V
  void get_instance(int b, std::vector<double>& x, std::vector<double>& s, std::vector<double>& y,
                    std::vector<double>& z, std::vector<double>& V);
  void put_instance(int b, const std::vector<double>& x, const std::vector<double>& s, const std::vector<double>& y,
                    const std::vector<double>& z);

  // the full tape at the iterate, scaled; the system's s, y, z, V are then the iterate's (what the Newton step reads),
  // a copy of V is kept as the current point's, and the errors are reduced -> err [B][kBatchErrN]
  void refresh(std::vector<double>& err);
  void newton_direction(std::vector<double>& dir);     // after compute(): keep p, p_s, p_z; dir [B][3]
  // trial point along the Newton (mode 0) or correction (mode 1) direction, value sweep, metrics -> met [B][4]
  void trial_values(std::vector<double>& met);
  // second-order correction: rhs, solve on the instance's factor, direction -> sd [B][2] (alpha_soc, alpha_z_soc)
  void soc_step(std::vector<double>& sd);
  // KKT-error fallback: errors at the current point, then full sweep at the full step and its errors
  void kkt_fallback(std::vector<double>& err_cur, std::vector<double>& err_trial);
  void commit();

 private:
  friend struct BatchIpmProbe;  // (the test-only probe, tests/support/batchcheck.cpp, reads the buffers below)
  DevBuf<int32_t> m_scale_idx, m_mode;
  DevBuf<uint8_t> m_is_static, m_active, m_s_from_ci, m_first;
  DevBuf<double> m_static_raw, m_scales, m_mu, m_tau, m_alpha, m_alpha_z, m_alpha_soc, m_out;
  DevBuf<double> m_x, m_s, m_y, m_z, m_tx, m_ts, m_ty, m_tz, m_sx, m_ss, m_sy, m_sz;  // iterate, trial, correction
  DevBuf<double> m_p, m_ps, m_pz, m_Vcur, m_tce, m_tci, m_sce, m_scims, m_t;
  void scale_V(int count);
  void errors(const double* V, bool trial, std::vector<double>& err);
  void download_out(size_t per_instance, std::vector<double>& out);
};

struct BatchSolveResult {
  std::vector<ExitStatus> status;                     // [B]
  std::vector<double> x, s, y, z;                     // [B][n], [B][m_i], [B][m_e], [B][m_i]
  std::vector<double> cost;                           // [B] unscaled f at the last iterate
  std::vector<int> iterations, restorations;          // [B]
  SolveReport report;                                 // batch totals; wall-clock phases of the batch
  // how the batch ran: lockstep rounds (batched Newton-step computations of the outer loop), instances handed to the
  // batch-1 system for restoration, and the driver: 0 none needed, 1 interior point, 2 SQP, 3 Newton
  int64_t rounds = 0, handoffs = 0;
  int driver = 0;
};

// x0 = [B][n]; scales = [B][1 + m_e + m_i] (compute_problem_scaling at each instance's x0); `run[b]` = 0:
// instance b is not solved here (its status in `out` is left as the caller set it).  `sys` is the batch
// system (batch() == B, tape at unit scales), `single` the batch-1 system of the same model (restoration).
// Problems with inequality constraints only (the others: sqp_batch / newton_batch, eq_batch.hpp).
void interior_point_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales,
                          const Options& options, const std::vector<double>& x0, const std::vector<uint8_t>& run,
                          BatchSolveResult& out);

}  // namespace slpx
