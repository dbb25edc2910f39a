// Batched whole solves: B instances of one compiled model, each from its own initial guess, with the options and the
// compiled structure shared.  Every instance follows the iteration Problem::solve() would run from its start —
// interior point (interior_point.hpp:129-878), SQP (sqp.hpp:98-604) or Newton (newton.hpp:51-292) — with its own
// problem scaling, filter, δ/γ memory, full-step-rejection counter, iteration count and exit, its decisions taken by
// the code the single-problem drivers share (ipm_line_search.hpp, ipm_decide.h) from a few scalars, while the device
// work of all instances still iterating runs as ONE batched launch per phase: the AD sweeps, the KKT build, the
// regularized factorization (NewtonSystem::compute with an instance mask), the solves, and every O(n) piece around
// them.
//
// ONE loop runs every driver in lockstep (batch_lockstep.cpp): one Newton step for every running instance, then the
// line search in rounds — each round one masked launch of second-order-correction solves, of value sweeps and of the
// full sweeps of the KKT-error fallback for the instances that wait for that work — then commit, refresh, exits.  An
// instance that has finished is frozen: the kernels skip it by its active flag.  Feasibility restoration runs on the
// problem's own batch-1 system (`single`), one instance at a time, with that instance's scaling, iterate, barrier
// parameter, δ/γ memory and filter; the result is written back into the batch state.  (restoration_mode 1: the
// instances that ask in one round run one restoration phase together on the batch system instead — fr_batch.hpp.)
//
// This header holds what every driver shares on the device: the reductions of batch_errors_kernel and BatchDevice,
// the state under BatchIpmDevice (ipm_batch.hpp) and BatchEqDevice (eq_batch.hpp).
#pragma once

#include <cstdint>
#include <vector>

#include "ipm.hpp"

namespace slpx {

// the per-instance scalars of batch_errors_kernel (out[b * kBatchErrN + k]); see batch_lockstep.cpp for their use
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

// pointers of one batch's iterate-shaped buffers
struct BatchIter {
  double *x, *s, *y, *z;
};

// A warm start of a batch (warm_start.h: units and safeguard): the iterate every instance begins at, in the USER'S
// units, host arrays [B][m_i], [B][m_e], [B][m_i] and the barrier parameter [B] (<= 0: choose); a null block is
// absent.  Passing one, even with every block null, also asks for the end iterate in the user's units
// (BatchSolveResult::s_u, y_u, z_u, mu_u) and the repair counts.
struct BatchWarmStart {
  const double *s = nullptr, *y = nullptr, *z = nullptr, *mu = nullptr;
};

// The device state every batched driver has (methods: ipm_batch_launch.hip): the iterate's x and y, the trial
// point's, the correction's, the current point's V of every instance, batch-major, and the per-instance parameters
// of a launch.  Launches take effect for the instances flagged in `active` only.  A derived device adds the buffers
// and launches of its iteration and says, once, where the errors and the refresh find the rest of an iterate
// (m_cur, m_trial) and the barrier parameter (m_mu_of_errors).
struct BatchDevice {
  NewtonSystem& sys;
  int B, n, m_e, m_i, dim, ns, nV;
  // per-instance parameters, host side; upload() sends them with `active` (one synchronization)
  std::vector<double> alpha, alpha_soc;
  std::vector<int32_t> mode;           // trial direction: 0 Newton, 1 second-order correction
  std::vector<uint8_t> first, active;  // first: the correction's accumulators start from the constraints' values
  void upload();
  void set_scales(const std::vector<double>& scales);  // [B][1 + m_e + m_i]
  // all instances; s and z are empty where m_i = 0
  void set_iterate(const std::vector<double>& x, const std::vector<double>& s, const std::vector<double>& y,
                   const std::vector<double>& z);
  void get_iterate(std::vector<double>& x, std::vector<double>& s, std::vector<double>& y, std::vector<double>& z);
  // one instance (feasibility restoration hand-off): its iterate, and its current V
  void get_instance(int b, std::vector<double>& x, std::vector<double>& s, std::vector<double>& y, std::vector<double>& z,
                    std::vector<double>& V);
  void put_instance(int b, const std::vector<double>& x, const std::vector<double>& s, const std::vector<double>& y,
                    const std::vector<double>& z);
  // the full tape at the iterate, scaled; the system's s, y, z, V are then the iterate's (what the Newton step reads),
  // a copy of V is kept as the current point's, and the errors are reduced -> err [B][kBatchErrN]
  void refresh(std::vector<double>& err);
  // The first iterate from a warm start (batch_warm_start_kernel): s, y, z of every instance with run[b] != 0 and a
  // finite input are written into the iterate — x must be there (set_iterate) and the system's V must be the sweep at
  // x with unit scales, as the caller's scaling sweep leaves it.  mu_min [B]; out [B][3]: the first barrier parameter
  // (scaled), the entries repaired, 1 for a non-finite input (then nothing of the instance was written).
  void warm_start(const BatchWarmStart& ws, const std::vector<uint8_t>& run, const std::vector<double>& mu_min,
                  std::vector<double>& out);
  // s, y, z of the iterate in the user's units (batch_unscale_iterate_kernel); instances with run[b] == 0 read 0
  void unscaled_iterate(const std::vector<uint8_t>& run, std::vector<double>& s_u, std::vector<double>& y_u,
                        std::vector<double>& z_u);

 protected:
  explicit BatchDevice(NewtonSystem& sys);
  DevBuf<int32_t> m_scale_idx, m_mode;
  DevBuf<uint8_t> m_is_static, m_active, m_first;
  DevBuf<double> m_static_raw, m_scales, m_alpha, m_alpha_soc, m_out, m_Vcur;
  DevBuf<uint8_t> m_ws_run;                                 // warm start: made at its first use
  DevBuf<double> m_ws_s, m_ws_y, m_ws_z, m_ws_mu, m_ws_out;
  DevBuf<double> m_x, m_y, m_tx, m_ty, m_sx, m_sy, m_tce, m_sce;  // iterate, trial, correction; trial c_e, its accumulator
  BatchIter m_cur{}, m_trial{};            // the iterate and the trial point, with the derived device's s and z
  const double* m_mu_of_errors = nullptr;  // [B] the barrier parameter batch_errors_kernel reads
  template <class Buf, class Vec>
  void put_async(Buf& buf, const Vec& v) {
    SLPX_HIP_CHECK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, sys.device().stream()));
  }
  void scale_V(int count);
  // the tape's inputs from m_cur (duals times the instance's d_c; with_state: s, y, z into the system's buffers too), the
  // full tape at unit scales, the instance's scaling of what it wrote: the system's V is the iterate's
  void sweep_iterate(bool with_state);
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
  // restoration in lockstep (restoration_mode 1; fr_batch.hpp): instances restored, phases, lockstep rounds of the
  // restoration loop, instances that used the batch-1 system for the KKT-error fallback — all 0 in hand-off mode
  int64_t restoration_lockstep[4] = {0, 0, 0, 0};
  // with a BatchWarmStart only: the end iterate in the user's units (warm_start.h), and how many entries of the given
  // iterate the safeguard replaced or clamped, [B]
  std::vector<double> s_u, y_u, z_u, mu_u;
  std::vector<int> repaired;
};

// x0 = [B][n]; scales = [B][1 + m_e + m_i] (compute_problem_scaling at each instance's x0); `run[b]` = 0: instance b
// is not solved here (its status in `out` is left as the caller set it).  `sys` is the batch system (batch() == B,
// tape at unit scales), `single` the batch-1 system of the same model (restoration).  A model takes the driver
// Problem::solve() gives it: interior_point_batch m_i > 0, sqp_batch m_i == 0 and m_e > 0, newton_batch m_e == m_i == 0.
// restoration_mode 0: an instance that asks for feasibility restoration is handed to `single`, one after the other
// (the default); 1: all instances that ask in one round enter one restoration phase on the batch system, in lockstep
// (fr_batch.hpp: restoration_phase).
// instance_params (null: every instance is the model as compiled): [B][n_p] parameter rows (NlpStructure::
// parameter_nodes order) that the caller has INSTALLED per instance on `sys` (DeviceNlp::set_parameters); wherever
// `single` works for an instance — the restoration hand-off, the KKT-error fallback and the multiplier estimate of a
// lockstep phase — that instance's row is installed there first, as its scaling is.  The caller puts `single`'s own
// values back afterwards, as it does the scaling.
// warm (null: the cold start, the bits of every release before it): see BatchWarmStart; the system's V must then be the
// sweep at x0 with unit scales (what the scaling was computed from).  Newton reads x0 only.
void interior_point_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales,
                          const Options& options, const std::vector<double>& x0, const std::vector<uint8_t>& run,
                          BatchSolveResult& out, int restoration_mode = 0,
                          const std::vector<double>* instance_params = nullptr, const BatchWarmStart* warm = nullptr);
void sqp_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
               const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out, int restoration_mode = 0,
               const std::vector<double>* instance_params = nullptr, const BatchWarmStart* warm = nullptr);
void newton_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
                  const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out,
                  const std::vector<double>* instance_params = nullptr, const BatchWarmStart* warm = nullptr);

}  // namespace slpx
