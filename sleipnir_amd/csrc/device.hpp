// Device-side state of one compiled NLP on one MI355X: uploaded plans, per-batch
// value buffers, and launchers for the hot-path kernels (kernels.hip): V, the iterate, the KKT
// system and the interior-point iteration.  Three parts of it are classes of their own:
//   tape()  DeviceTape (device_tape.hpp, device_tape.hip): the uploaded tapes and every sweep launch;
//   ldlt()  DeviceLdlt (device_ldlt.hpp, device_ldlt.hip): the factorization and the solve;
//   StepChain (step_chain.hpp): the protocol of chained steps, between a sweep and the step kernel.
// The types they are made of — DevBuf, the plans on the device, KktFuse / BacksubFuse — are device_base.hpp's.
//
// Batch-major layout everywhere: buffer[b * stride + i], b = problem in the batch.
// All problems of a batch share one structure (tape, KKT plan, symbolic LDLᵀ) and
// differ only in values — the reference's analogue is multistart's one-thread-per-
// solve fan-out (include/sleipnir/optimization/multistart.hpp:52-62).
#pragma once

#include "device_base.hpp"
#include "device_ldlt.hpp"
#include "device_tape.hpp"
#include "step_chain.hpp"

namespace slpx {

class DeviceNlp {
 public:
  DeviceNlp(const NlpStructure& s, const KktPlan& k, const LdltPlan& l, int batch, int device, const Switches& sw);
  ~DeviceNlp();

  int batch() const { return m_batch; }
  void set_stream(hipStream_t s) { m_stream = s; }
  hipStream_t stream() const { return m_stream; }

  // scaling vectors: scales = [d_f, d_ce.., d_ci..]; applied to tape outputs, and
  // d_ce / d_ci also scale the dual inputs (problem.hpp:631-634).  Re-derives the
  // static part of V.
  void set_scaling(const std::vector<double>& scales);

  // state upload/download (host pointers, batch-major)
  void upload_x(const double* x);
  void upload_duals(const double* s, const double* y, const double* z);
  void upload_mu(const double* mu);  // one per batch item
  void download_V(double* V);
  void download(const double* dev, double* host, size_t count);

  // hot path (all asynchronous on stream())
  // f, c_e, c_i, g, A_e, A_i, H_f, H_c -> V.  with_reduce = false leaves the separable-sum
  // reductions (they only feed f) to the build_kkt(true) that must follow.
  void sweep_full(bool with_reduce = true);
  // The sweep of a Newton step whose factor_solve_publish() follows at once (no reductions: they ride in
  // that launch).  Where the step is the one-launch multifrontal kernel and this step follows another
  // directly (nothing else was handed the main stream in between), the sweep goes to a stream of its own
  // and the two kernels order themselves through words in memory (StepChain): the step kernel is
  // dispatched and stages its plan WHILE the sweep runs, and the sweep of the next step starts the moment
  // this step's kernel is through — no launch boundary on either side.  DESIGN.md §4, "chained steps".
  void sweep_full_for_step();
  void recover_from_chain_failure();  // after a step whose counters carry kLdltChainFailure
  int chain_failures() const { return m_chain.failures(); }
  // test hook: the next chained sweep is launched as if the step kernel before it never signalled
  void debug_break_next_chain() { m_chain.debug_break_next(); }
  void sweep_values();  // f, c_e, c_i only                   -> V
  void assemble();      // V, s, z -> lhs
  void build_kkt(bool with_reduce);  // assemble() + build_rhs() [+ reductions] as one launch
  void build_kkt_for_step(bool with_reduce);  // same, inside the launch of the factor() that must follow
  // Least-squares multiplier estimate system on the same pattern:
  // lhs = [[I + A_i^T S^-2 A_i, A_e^T],[A_e, 0]] (util/lagrange_multiplier_estimate.hpp:56-133
  // with d, t eliminated; see ipm_restoration.cpp)
  void assemble_lsq();  // V, s -> lhs
  void build_rhs();     // V, s, y, z, mu -> rhs
  // The tapes: the sweeps above fill a DeviceTape::Sweep and launch it; the parameter pools are asked of it directly
  // (DeviceTape::set_parameters says what the two forms mean)
  DeviceTape& tape() { return m_tape; }
  const DeviceTape& tape() const { return m_tape; }
  void refresh_params(const Graph& g) { m_tape.refresh_params(g); }
  void set_parameters(const double* values, bool per_instance) { m_tape.set_parameters(values, per_instance); }
  // The linear solver: its counters, factors, solution and bare launches are asked of it directly.  What follows here
  // is the orchestration that needs both sides — the system brought up to date, the riders built, then m_ldlt called.
  DeviceLdlt& ldlt() { return m_ldlt; }
  const DeviceLdlt& ldlt() const { return m_ldlt; }
  // lhs -> L, D, stats; per-problem (δ, γ), problems with active[b] == 0 are skipped
  void factor(const std::vector<double>& delta, const std::vector<double>& gamma,
              const std::vector<uint8_t>& active);
  void solve();                                     // rhs -> p (dim per batch item)
  void solve_after_factor();                        // p for the rhs that was in place at factor()
  bool step_is_one_launch() const { return m_mode.fuse_solve && m_mode.fuse_kkt; }
  bool step_is_multifrontal() const { return m_mode.mf; }
  bool factorization_is_dense() const { return m_mode.dense; }
  void solve_backsub_publish();                     // solve_after_factor() + backsub_publish(), one launch where possible
  // factor() + solve_backsub_publish(): ONE launch where every task's workgroup fits on the device at once
  void factor_solve_publish(const std::vector<double>& delta, const std::vector<double>& gamma,
                            const std::vector<uint8_t>& active);
  void refine_solution(int iters);                  // iterative refinement of the last solve() against the lhs
  // ---- residual of the solution in memory, and the pieces of its iterative refinement (kkt_refine.hip; the loop is
  // NewtonSystem::refine) ----
  // r = rhs - (lhs + diag(delta, -gamma)) p for the problems with mask[b] != 0, accumulated in double-double
  // (kkt_residual.h), into d_residual(); norm[b] = max |r_i| of those problems (a NaN or Inf in r shows as a non-finite
  // norm), the others' entries of r and norm are not touched.  (delta, gamma) are those of the factorization whose
  // factors are in memory.  Needs a factorization and a solution in memory (throws otherwise); lhs / rhs are assembled
  // at the RESIDENT state if the step that made p never stored them.  Synchronizes.
  void residual(const std::vector<uint8_t>& mask, std::vector<double>& norm);
  double* d_residual() { return m_res.p; }
  void refine_begin();             // keeps p and rhs
  void refine_solve_correction();  // residual -> rhs, solve(), the correction d kept aside, rhs = the kept one again
  void refine_apply(const std::vector<uint8_t>& accept);  // p = kept p + d where accept[b], the kept p elsewhere
  void refine_keep_solution();     // the kept p = p
  // ---- error bounds of the solution in memory (kkt_errbound.hip; the loops are NewtonSystem::error_bounds / condest) ----
  // Per problem with mask[b] != 0: norm1 = max row sum of |Kreg|; with want_bounds also berr = max |r_i| / w_i,
  // p_inf = max |p_i|, f_inf = max f_i, from the r a residual() call left in d_residual(), and w, f = |r| + rho kept
  // in memory for errbound_round().  The preconditions and the assembly of residual().  Synchronizes.
  struct ErrRowScalars {
    double berr = 0.0, norm1 = 0.0, p_inf = 0.0, f_inf = 0.0;
  };
  void errbound_rows(const std::vector<uint8_t>& mask, bool want_bounds, std::vector<ErrRowScalars>& out);
  // One round of the 1-norm estimator for every problem at once: each problem's probe vector (kind: NormEstProbe of
  // kkt_errbound.h; zeros for kProbeNone) into the right-hand side, solve(), the solution to four scalars.  scale:
  // 0 plain, 1 the probe times f before the solve, 2 the solution times f after it.  kept: which sign buffer holds the
  // kept sign vector; sign(v) goes to the other.  OVERWRITES rhs and p: between refine_begin() and errbound_restore().
  struct EstRound {
    int32_t kind = 0, j = 0, scale = 0, kept = 0;
  };
  struct EstScalars {
    double norm1 = 0.0;
    int argmax = 0;
    bool signs_repeated = false, finite = true;
  };
  void errbound_round(const std::vector<EstRound>& rounds, std::vector<EstScalars>& out);
  void errbound_restore();  // p and rhs = what refine_begin() kept, to the bit
  void backsub();                                   // p -> p_x, p_y, p_s, p_z
  void backsub_publish();                           // ... and the current attempt's counters to the host
  // Twin attempt (DeviceLdlt::step_twin): the policy loop's attempt (delta0, gamma0) and the one it would make
  // next (delta1, gamma1) in ONE launch; `mode` as IpmTwin::mode.  false: not possible now (the caller makes a
  // single attempt).  adopt_twin() makes the second attempt's factor, direction and counters the system's.
  bool factor_solve_publish_twin(double delta0, double gamma0, double delta1, double gamma1, int mode);
  // ... for a caller that wrote BOTH attempts' systems itself (restoration.hpp): the first in lhs_raw() / rhs_raw(), the
  // second in (lhs2, rhs2)
  bool factor_solve_publish_twin_written(double delta0, double gamma0, double delta1, double gamma1, int mode, const double* lhs2,
                                         const double* rhs2);
  void adopt_twin();

  // ---- interior-point iteration on the device (ipm_kernels.h; one problem) ----
  // All asynchronous on stream(); results arrive in ipm_host() after wait().
  void ipm_enable();                          // allocates the trial / correction buffers
  // [d_f | d_ce | d_ci] the termination test un-scales with (kkt_error.hpp:216-251); not
  // necessarily the scaling the tapes apply (feasibility restoration scales in its model)
  void ipm_set_error_scaling(const std::vector<double>& scales);
  void ipm_direction(double tau);             // step sizes, D_phi; trial x = x + alpha_max p_x
  void ipm_trial_point(double alpha);         // trial x = x + alpha p_x
  void sweep_values_trial();                  // f, c_e, c_i at the trial x -> trial V
  void ipm_trial_metrics(double alpha, bool s_from_ci);  // alpha < 0: the device's alpha_max
  void ipm_commit(double alpha, double alpha_z, bool s_from_ci);
  void ipm_errors(bool check_all_V, bool sums_ride = false, bool ahead = false);  // -> IpmHost::err (one launch; the last workgroup folds)
  // Look-ahead iteration: the iterate the FULL step alpha_max would give — x, s, y, z with the z reset of
  // interior_point.hpp:797-801 — in a second set of buffers, swept (values AND derivatives) and reduced to
  // IpmHost::err_ahead speculatively; when the filter accepts that trial point the buffers change roles
  // (ipm_accept_lookahead: no launch) and the iteration is complete after ONE host round trip.
  void ipm_lookahead(double tau);             // step sizes, D_phi -> IpmHost::dir; the look-ahead iterate
  // the full tape at it, into the look-ahead V (sums ride in ipm_errors).  with_reduce: the sweep finishes its sums
  // itself; skippable = false: not part of a chain ipm_lookahead flags as void (restoration.hpp makes its own iterate)
  void sweep_full_lookahead(bool with_reduce = false, bool skippable = true);
  void ipm_accept_lookahead();                // the look-ahead iterate and its V become the current ones
  void ipm_soc_accumulate(double alpha, bool first, bool s_from_ci);
  void ipm_soc_rhs();                         // -> rhs
  void ipm_soc_backsub();                     // p -> p_s, p_z with the corrected c_i - s
  void ipm_save_direction();
  void ipm_restore_direction();
  void wait();                                // busy-polls the stream
  void wait_published();                      // after ipm_trial_metrics / ipm_errors: their sequence number
  const IpmHost& ipm_host() const { return *m_ipm_host; }
  // ---- the pipelined common iteration (ipm_resident.cpp: ResidentIpm; ipm_decide.h) ----
  // Two sets of the scalar outputs: the chain of iteration k+1 is enqueued before the host has read iteration k's.
  // ipm_set_slot: where the kernels enqueued from now on leave theirs.
  void ipm_set_slot(int slot) { m_ipm_slot = slot & 1; }
  const IpmHost& ipm_host_slot(int slot) const { return m_ipm_host[slot & 1]; }
  // the iteration's state for the decision on the device (host -> device, in stream order), and what the device left
  void ipm_pipeline_upload(const struct IpmCtl& ctl);
  const struct IpmCtl& ipm_pipeline_fetch();  // device -> host (synchronizes; the pipeline is drained when the host asks)
  // the NEXT step launch (one launch) waits for the decision of the error launch in front of it
  void ipm_gate_next_step(bool on) { m_gate_next_step = on; }
  // The error launch of the iteration whose look-ahead iterate was just made current (ipm_accept_lookahead) RIDES in
  // the next step launch (a launch of two attempts: ldlt_mf_twin_kernel<.., true>) and decides there whether that step
  // counts; its scalars and verdict go to the host slot `slot_out` (err_ahead, go).  false if such a launch cannot
  // carry it (then nothing was armed).  ipm_ride_wait(): the verdict, once those scalars are in.
  bool ipm_ride_errors_in_next_step(int slot_out);
  bool ipm_ride_possible();  // (asked once per system: both attempts' tasks and the riding workgroups resident at once; SLPX_IPM_RIDE=0: never)
  bool ipm_ride_wait(int slot_out);
  bool ipm_ride_armed() const { return m_ride_next; }
  void ipm_ride_disarm() { m_ride_next = false; }
  // ipm_errors(.., ahead) that also takes the decision
  void ipm_errors_deciding(bool sums_ride);
  unsigned long long seq_expected() const { return m_seq_expected; }
  void wait_published_until(unsigned long long seq);
  // what a launch changes on the host side of the step machinery (buffer parities, pending work): saved before a
  // speculative launch, put back when the device let it pass
  struct LaunchBook {
    DeviceLdlt::Book ldlt;
    ChainLedger::Book chain;
    int kkt_pending;
    bool lhs_stale, rhs_stale;
  };
  LaunchBook save_book() const { return LaunchBook{m_ldlt.save_book(), m_chain.save(), m_kkt_pending, m_lhs_stale, m_rhs_stale}; }
  // launch_ran: the launch was not let pass at its gate — it ran with its results held back (a step that carried the
  // error launch deciding about it: MfDev::ride_verdict) and so moved the launch's OWN hand-overs on (DeviceLdlt::restore_book)
  void restore_book(const LaunchBook& b, bool launch_ran = false) {
    m_ldlt.restore_book(b.ldlt, launch_ran);
    m_chain.restore(b.chain);
    m_kkt_pending = b.kkt_pending;
    m_lhs_stale = b.lhs_stale;
    m_rhs_stale = b.rhs_stale;
  }
  double* d_V_trial() { return m_V_trial.p; }
  // the tape's separable sums (for a caller's launch that lets them ride: restoration.hip's error launch)
  const NlpStructure::SumReduce* reduces_dev() const { return m_tape.reduces_dev(); }
  int n_reduces() const { return static_cast<int>(m_tape.n_reduces()); }
  const double* tape_scales_dev() const { return m_tape.scales_dev(); }

  // device pointers for callers that keep everything resident
  double* d_x() { return m_in.p; }
  double* d_V() { return m_V.p; }
  double* d_s() { return m_s.p; }
  double* d_y() { return m_y.p; }
  double* d_z() { return m_z.p; }
  double* d_mu() { return m_mu.p; }
  // (a step whose factorization evaluated the system in place left nothing in memory: assembled on demand)
  double* d_lhs() {
    materialize_kkt();
    materialize_batch_major();
    return m_lhs.p;
  }
  double* d_rhs() {
    materialize_kkt();
    materialize_batch_major();
    return m_rhs.p;
  }
  void materialize_kkt();
  void materialize_batch_major();
  // A caller that writes the system itself (restoration.hpp: the reduced system of the restoration problem on this
  // system's pattern): the arrays as they are, and "what is there IS the current system" / "the state changed under it"
  const KktDev& kdev() const { return m_kdev; }
  double* lhs_raw() { return m_lhs.p; }
  double* rhs_raw() { return m_rhs.p; }
  void system_written_by_caller(bool lhs, bool rhs) {
    m_kkt_pending = 0;
    if (lhs) m_lhs_stale = m_lhs_in_il = false;
    if (rhs) m_rhs_stale = m_rhs_in_il = false;
  }
  void state_changed_by_caller() { m_lhs_stale = m_rhs_stale = true; }
  double* d_trial_in() { return m_trial_in.p; }
  double* d_s_ahead() { return m_s_ahead.p; }
  double* d_y_ahead() { return m_y_ahead.p; }
  double* d_z_ahead() { return m_z_ahead.p; }
  hipStream_t raw_stream() const { return m_stream.raw(); }
  // the step's direction: p is the solver's solution (ldlt().d_p(), what the library itself asks), p_s and p_z are made
  // here; the test probes read the three side by side
  double* d_p() { return m_ldlt.d_p(); }
  double* d_ps() { return m_ps.p; }
  double* d_pz() { return m_pz.p; }
  int in_stride() const { return m_s_ref.n_inputs(); }
  int v_stride() const { return m_s_ref.nV; }

  const NlpStructure& structure() const { return m_s_ref; }
  const KktPlan& kkt() const { return m_k_ref; }

 private:
  void build_kkt(bool with_reduce, bool defer);  // defer: only note the request, for the factorization that follows
  // the constructor's phases, in its order (kernels.hip)
  void choose_initial_modes();
  void upload_kkt_plan();
  void upload_inline_kkt(const struct InlineKkt& ik);
  void upload_inline_backsub(const struct InlineBacksub& ib);
  void alloc_value_buffers();
  void alloc_interleaved_buffers();
  void alloc_pinned();

  DeviceArena m_arena;  // the plan arrays uploaded by the constructor (DevBuf::upload places them here)
  const NlpStructure& m_s_ref;
  const KktPlan& m_k_ref;
  const LdltPlan& m_l_ref;
  int m_batch;
  int m_device;
  // Which kernels serve this system: written by the stages of system_choice.hpp only, from what this class measures
  const Switches m_sw;
  LaunchModes m_mode;
  PlanFacts m_plan;  // what those stages read of m_l_ref
  int m_cus = 0;  // compute units of the device
  StepChain m_chain;  // (before the stream that reports to it)
  TrackedStream m_stream{m_chain};
  // one problem: the publishing kernel also bumps a sequence number the host spins on
  volatile unsigned long long* m_h_seq = nullptr;  // pinned
  DevBuf<unsigned long long> m_seq_dev;
  unsigned long long m_seq_expected = 0;  // publishing launches enqueued so far
  DeviceTape m_tape;
  DeviceLdlt m_ldlt;  // (after what it holds references to)

  // the KKT plan, and what the hot path hands the kernels of it
  KktPlanDevice m_kplan;
  KktDev m_kdev{};
  DevBuf<int32_t> m_lhs_colptr, m_lhs_rowidx, m_lhs_rowptr, m_lhs_rowent, m_lhs_rowcol;  // refine_solution (uploaded on first use)
  DevBuf<double> m_rhs0, m_p_acc;
  // residual / refinement (kkt_refine.hip): the row map of the lhs (KktRowMap) and the buffers, all made on first use
  DevBuf<int32_t> m_rm_rowptr, m_rm_ent, m_rm_col;
  DevBuf<double> m_res, m_ref_keep_p, m_ref_keep_b, m_ref_d, m_res_reg;
  DevBuf<unsigned long long> m_res_partial, m_res_norm;
  DevBuf<uint8_t> m_res_mask;
  void residual_buffers();
  // error bounds (kkt_errbound.hip), made on first use: w, f; the workgroups' slots and a problem's scalars ([.][4]);
  // the two sign buffers ([2][batch][dim]); the commands of a round
  DevBuf<double> m_eb_w, m_eb_f;
  DevBuf<unsigned long long> m_eb_partial, m_eb_scal;
  DevBuf<int8_t> m_eb_sign;
  DevBuf<int32_t> m_eb_cmd;
  void errbound_require(const std::vector<uint8_t>& mask, const char* what);
  // per-batch values
  DevBuf<double> m_in, m_V, m_s, m_y, m_z, m_mu, m_lhs, m_rhs, m_ps, m_pz;
  int m_kkt_pending = 0;              // the factorization that follows evaluates the system (1: lhs + rhs, 2: + the tape's sums)
  KktFuse take_kkt_fuse();
  BacksubFuse backsub_fuse();  // (the counters it hands over: DeviceLdlt's)
  KktFuse kkt_fuse_for(int kkt_mode) const;
  LdltSystem system() const { return LdltSystem{m_lhs.p, m_rhs.p, m_lhs_il.p, m_rhs_il.p, m_lhs_in_il, m_rhs_in_il}; }
  void backsub_and_publish(bool publish);
  // the riders of a step launch made now (a twin launch adds its own)
  LdltStepRiders step_riders(const KktFuse& f);
  // the second attempt's p_s, p_z (a pair with m_ps, m_pz: adopt_twin), made with DeviceLdlt's twin buffers
  bool twin_ready();
  DevBuf<double> m_ps_tw, m_pz_tw;
  void launch_twin(double delta0, double gamma0, double delta1, double gamma1, int mode, const KktFuse& f, const double* lhs2,
                   const double* rhs2);
  MfRide ipm_take_ride();  // the armed riding error launch's arguments (ipm_ride_errors_in_next_step)
  IpmLookaheadArgs lookahead_args(double tau, int twin_mode);
  DevBuf<unsigned int> m_ipm_err_done;
  DevBuf<BsRow> m_bs_plan;            // BacksubFuse::plan (rows and terms share the 8-byte element size)
  DevBuf<uint4> m_bs_task_plan;
  DevBuf<int32_t> m_ent_vsrc;
  DevBuf<KktTerm> m_kkt_terms;
  DevBuf<uint2> m_task_terms;
  bool m_lhs_stale = false, m_rhs_stale = false;  // memory does not hold the system of the current state
  // batch-interleaved LDLT: the assembly kernels write the interleaved lhs / rhs themselves; *_in_il: the current
  // system is in the interleaved arrays only (a caller that wrote its own batch-major system: DeviceLdlt transposes it)
  bool m_lhs_in_il = false, m_rhs_in_il = false;
  DevBuf<double> m_lhs_il, m_rhs_il;
  std::vector<double> m_V_static;  // scaled static values (host copy)
  // interior-point iteration state (ipm_enable)
  bool m_ipm = false;
  DevBuf<double> m_s_ahead, m_y_ahead, m_z_ahead;  // with m_trial_in (x | y | z) and m_V_trial: the look-ahead iterate
  DevBuf<double> m_trial_in, m_V_trial, m_soc_ce, m_soc_cims, m_p_keep, m_ps_keep, m_pz_keep, m_ipm_alpha, m_ipm_scales, m_ipm_partial;
  IpmHost* m_ipm_host = nullptr;   // pinned, two slots (ipm_set_slot)
  int m_ipm_slot = 0;
  struct IpmCtl* m_ipm_ctl_host = nullptr;   // pinned: [0] the device's mirror, [1], [2] staging of uploads
  int m_ipm_ctl_stage = 0;
  void* m_ipm_ctl_dev = nullptr;             // IpmCtl on the device
  DevBuf<double> m_ipm_gate;
  bool m_gate_next_step = false;
  bool m_ride_next = false;
  int m_ride_slot = 0;
  double m_ride_ticket = 1.0;       // of the last riding launch (2, 3, ...: never a plain launch's 0 / 1 in IpmHost::go)
  DevBuf<double> m_ipm_ride_verdict;
  bool m_errors_decide = false;
};

}  // namespace slpx
