// The device side of feasibility restoration for a batch (restoration.hpp: the same reduction, per instance): the
// batched counterpart of FrDevice, layered like BatchIpmDevice over BatchDevice.  Kernels: fr_batch_kernels.h, launch
// wrappers: fr_batch_launch.hip.
//
// An instance in restoration has its WHOLE restoration iterate here — its own x, s_0, y, z_0 (BatchDevice's iterate
// buffers of THIS object), p / n with their slacks and duals, x_R, zeta D_R and the outer problem's quantities at the
// point of entry — so the outer iterate in the driver's BatchIpmDevice / BatchEqDevice is not touched until the
// instance leaves restoration.  The batch system's shared buffers (tape input, V, lhs, rhs, solution) are scratch, as
// for every batched driver: a sweep or a solve overwrites the slices of all instances.
//
// Determinism contract: an instance's outputs are a function of ITS inputs alone.  The reduced system is built row by
// row ((chunks, B) grid, no reduction); everything that reduces is one 256-thread workgroup per instance, strided
// per-thread partials and block_reduce (ipm_reduce.h) in an order fixed by the model's sizes — never by B, by the slot
// or by which other instances are active.  No floating-point atomics, and no kernel waits for another workgroup.  An
// instance whose active flag is 0 is skipped by whole workgroups: nothing of its slices is read or written.
// The row arithmetic is fr_rows.h's and ipm_formulas.h's, the bodies the single-problem kernels run.
#pragma once

#include "batch_lockstep.hpp"
#include "restoration.hpp"

namespace slpx {

// out[b * kFrBatchErrN + k] of BatchFrDevice::errors: FrErrOut (restoration.hpp) as doubles, field by field
constexpr int kFrBatchErrN = 29;
static_assert(sizeof(FrErrOut) == kFrBatchErrN * sizeof(double), "FrErrOut is 24 + 5 doubles");

struct FrBatchArgs;  // the kernels' view (fr_batch_kernels.h)

struct BatchFrDevice : BatchDevice {
  explicit BatchFrDevice(NewtonSystem& sys);
  int M = 0, nnz = 0;  // 2 m_e + 2 m_i; entries of an instance's lhs
  // per-instance parameters of the next launches, host side, beside BatchDevice's alpha (the step size of a trial
  // point, a correction or a commit), first and active; upload() sends them all (one synchronization)
  std::vector<double> delta, mu, tau, alpha_z, mu_outer;
  std::vector<uint8_t> soc, rhs_only;
  void upload();

  // Start of a restoration phase for instance b (host vectors, FrDevice::begin's): the restoration iterate (x, s_0,
  // y, z_0; [p_e | n_e | p_i | n_i] with slacks and duals), x_R and zeta D_R, the outer problem's dense gradient and
  // slacks at the point of entry.  mu_outer[b] and the scales (set_scales: [d_f | d_ce | d_ci], which also un-scale
  // the error measure) are set by the caller.  Synchronizes.
  void begin(int b, const double* x, const double* s0, const double* y, const double* z0, const double* x_r, const double* w,
             const double* g_outer, const double* s_outer, const double* pn, const double* sx, const double* zx);
  // the whole restoration iterate of instance b -> host (x n, s_0 m_i, y m_e, z_0 m_i, pn / sx / zx M each)
  void download_instance(int b, double* x, double* s0, double* y, double* z0, double* pn, double* sx, double* zx);

  // ... its direction (p dim, p_s0 / p_z0 m_i, dpn / psx / pzx M each) and its current V (nV) -> host
  void download_direction(int b, double* p, double* ps0, double* pz0, double* dpn, double* psx, double* pzx);
  void download_V(int b, double* V);

  // the full tape at the active instances' (x, y, z_0), scaled: their current V (kept here)
  void sweep();
  // the reduced system of every active instance for delta[b], mu[b] (soc[b], rhs_only[b]) into the batch system's
  // batch-major lhs / rhs, which then ARE the current system (DeviceNlp::system_written_by_caller)
  void build();
  // the batch system's solution p = (dx, w) of every active instance -> the whole direction, kept here; dir [B][4]:
  // alpha_max, alpha_z, D_phi, the smallest eliminated pivot; the first trial x is in the tape's input
  void expand(std::vector<double>& dir);
  // trial x = x + alpha[b] dx into the tape's input, a value sweep, the filter entry of X + alpha dX -> met [B][4]:
  // f, violation, sum ln s, finite.  after_expand: the trial x is already in place (alpha[b] is the step it was made with)
  void trial_values(std::vector<double>& met, bool after_expand = false);
  // second-order correction (interior_point.hpp:590-640): accumulate (first[b]) from the trial values in the system's V,
  // the corrected right-hand side (rhs only), a solve on the instance's factors, expand -> dir [B][4]
  void soc_accumulate();
  void save_direction();
  void restore_direction();
  void commit();  // X += alpha[b] dX, y, z += alpha_z[b] .., z reset with mu[b] (interior_point.hpp:775-801)
  // after sweep(): err [B][kFrBatchErrN], FrErrOut of every active instance; check_all_V as FrDevice::errors
  void errors(bool check_all_V, std::vector<double>& err);

 private:
  friend struct BatchFrProbe;  // (the test-only probe, tests/support/frbatchcheck.cpp, reads the buffers)
  DevBuf<int32_t> m_diag_of;
  DevBuf<double> m_delta, m_mu, m_tau, m_alpha_z, m_mu_outer;
  DevBuf<uint8_t> m_soc, m_rhs_only;
  DevBuf<double> m_s0, m_z0;                                 // with BatchDevice's m_x, m_y: the restoration iterate
  DevBuf<double> m_xr, m_w, m_g_outer, m_s_outer;            // fixed for the phase
  DevBuf<double> m_pn, m_sxx, m_zx;                          // [p_e | n_e | p_i | n_i], their slacks and duals
  DevBuf<double> m_p, m_ps0, m_pz0, m_dpn, m_psx, m_pzx;     // the direction
  DevBuf<double> m_soc_ce, m_soc_c0, m_soc_x;
  DevBuf<double> m_keep_p, m_keep_ps0, m_keep_pz0, m_keep_dpn, m_keep_psx, m_keep_pzx;
  DevBuf<double> m_vt;  // f, c_e, c_i of an instance's last trial point
  DevBuf<double> m_fr_out;
  void fill(FrBatchArgs& G);
  void copy_direction(bool restore);
  void download_fr_out(size_t per_instance, std::vector<double>& out);
};

// ---- the restoration phase of the lockstep loop (fr_batch_lockstep.cpp) ----
// One instance's part in a phase: feasibility_restoration() (ipm_restoration.cpp) as interior_point() / sqp() enter it — the outer
// iterate (x, s, y, z; in / out), its barrier parameter, c_e, c_i and the dense gradient at x, its constraint violation and
// `outer_accepts(entry, D_phi)`, the outer filter's verdict on a restoration iterate — and what comes back: the status
// feasibility_restoration() returns (SUCCESS: accepted, multipliers estimated).
struct BatchRestorationRequest {
  int b = 0;
  std::vector<double> scales;  // [d_f | d_ce | d_ci] of the instance
  // the instance's parameter row (NlpStructure::parameter_nodes order) where the batch runs with per-instance
  // parameters, empty otherwise: installed on the batch-1 system before it works for this instance
  std::vector<double> params;
  double mu = 0.0;
  std::vector<double> x, s, y, z, c_e, c_i, g;
  double initial_violation = 0.0;
  std::function<bool(const FilterEntry&, double)> outer_accepts;
  int* iterations = nullptr;  // the instance's iteration count: restoration iterations count as the outer loop's do
  SolveReport* rep = nullptr;
  ExitStatus status = ExitStatus::SUCCESS;
};
// instances restored in lockstep, phases, lockstep rounds (batched Newton-step computations of the restoration loop),
// instances that used the batch-1 system for the KKT-error fallback of a line search
struct BatchRestorationStats {
  int64_t instances = 0, phases = 0, rounds = 0, fallbacks = 0;
};
// Every request enters ONE phase together and runs restoration_core()'s iteration (ipm_restoration.cpp) with its own mu, tau, filter,
// line search and counters, the device work of all instances still iterating in one masked launch per phase of the
// iteration; an instance that is through waits masked until the phase ends.  `sys`: the batch system (its
// regularization memory of the restoring instances is reset for the phase and put back, gamma_min is 0 during it);
// `single`: the batch-1 system — the multiplier estimate at exit and the KKT-error fallback run there, per instance.
// stop_after >= 0: an instance leaves after that many restoration iterations, as if accepted (the seam of
// slpx_problem_restoration_steps_batch).
void restoration_phase(NewtonSystem& sys, NewtonSystem& single, BatchFrDevice& frd, const Options& options,
                       std::vector<BatchRestorationRequest>& requests, int stop_after,
                       std::chrono::steady_clock::time_point solve_start, BatchRestorationStats& stats);

}  // namespace slpx
