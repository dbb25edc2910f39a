// The linear solver of a DeviceNlp on the device: the uploaded LdltPlan, the factor and solve storage of the four
// kernel families (per-task rounds or single launch, batch-interleaved, dense plain or pivoted, the one-launch
// multifrontal step and its twin), what the host and those kernels pass each other through pinned memory, and every
// launch of an LDLT kernel (device_ldlt.hip, the only file that includes the ldlt_*_kernels.h headers).
//
// It knows nothing of tapes, V or the interior-point iteration: NLP work that rides in one of its launches comes as
// arguments — LdltSystem, KktFuse, BacksubFuse, LdltStepRiders — filled by DeviceNlp.
#pragma once

#include "device_base.hpp"
#include "step_chain.hpp"

namespace slpx {

struct MfImages;  // device_images.hpp
struct MfDev;     // ldlt_mf_kernels.h
struct MfRide;    // ipm_kernels.h

// The system a factorization or a solve reads, where DeviceNlp has it at this moment
struct LdltSystem {
  double* lhs = nullptr;  // batch-major
  double* rhs = nullptr;
  // batch-interleaved (LaunchModes::il): the arrays the kernels read; *_in_il: the current system is there already
  // (the assembly kernels wrote it), otherwise il_gather_kernel transposes the batch-major one first
  double* lhs_il = nullptr;
  double* rhs_il = nullptr;
  bool lhs_in_il = false, rhs_in_il = false;
};

// Everything of the NLP that rides in a launch of the multifrontal step kernel
struct LdltStepRiders {
  KktFuse kkt;
  BacksubFuse backsub;  // its sources, outputs and the publication word; DeviceLdlt adds the counters it hands over
  const double *lhs = nullptr, *rhs = nullptr;
  // a twin launch: the second attempt's back-substitution outputs, and its own system where the caller wrote one
  double *ps2 = nullptr, *pz2 = nullptr;
  const double *lhs2 = nullptr, *rhs2 = nullptr;
  // the chain link of a chained step (null: not chained), MfDev::chain / wait_step / this_step
  unsigned int* chain = nullptr;
  unsigned int wait_step = 0, this_step = 0;
  const double* gate = nullptr;  // MfDev::gate
  const MfRide* ride = nullptr;  // the error launch riding in a twin launch (its verdict word and ticket are in ride->fin)
};

class DeviceLdlt {
 public:
  // What DeviceNlp shares with its solver, all of it living in DeviceNlp: the stream, the launch modes both sides'
  // choice stages write, and the word the publishing kernels bump.  n_sums: the tape's separable sums (their
  // workgroups ride in the step kernel's launch: system_choice.hpp).
  struct Shared {
    TrackedStream& stream;
    LaunchModes& mode;
    const PlanFacts& facts;
    const Switches& sw;
    const int& cus;
    volatile unsigned long long* const& seq_host;
    size_t n_sums;
  };
  DeviceLdlt(const LdltPlan& l, const KktPlan& k, int batch, const Shared& sh);
  ~DeviceLdlt();
  DeviceLdlt(const DeviceLdlt&) = delete;
  DeviceLdlt& operator=(const DeviceLdlt&) = delete;

  // its share of the phases of DeviceNlp's constructor, called from that sequence (kernels.hip)
  void raise_lds_limits();
  void upload_plan();
  void upload_mf(const MfImages& im);  // the multifrontal step where every task is resident at once
  void alloc_dense_buffers();
  void alloc_value_buffers();  // (the caller synchronizes after its own)
  void arm_handover_buffers();
  void alloc_interleaved_buffers();
  void alloc_pinned();
  // dynamic LDS of the factorization with the KKT terms staged / of the backward solve with the rows staged
  // (device_images.hpp: InlineKkt::factor_lds, InlineBacksub::solve_lds)
  void set_factor_lds_inline(uint32_t bytes) { m_factor_lds_inline = bytes; }
  void set_solve_lds_inline(uint32_t bytes) { m_solve_lds_inline = bytes; }

  const LdltPlan& plan() const { return m_l; }

  // lhs -> L, D, stats; per-problem (δ, γ), problems with active[b] == 0 are skipped.  `f`: the system evaluated
  // inside the launch (only where factor_evaluates_inline())
  void factor(const std::vector<double>& delta, const std::vector<double>& gamma, const std::vector<uint8_t>& active,
              const LdltSystem& sys, const KktFuse& f);
  bool factor_evaluates_inline() const { return !m_mode.dense && !m_mode.il && m_mode.single_launch; }
  void read_stats(std::vector<LdltStats>& out);  // synchronizes
  void solve(const LdltSystem& sys);             // rhs (current: the caller saw to it) -> p (dim per batch item)
  // p for the rhs that was in place at factor(); `riding`: the back-substitution and the hand-over of the current
  // attempt's counters ride in the backward solve (the caller then notes stats_handed_to_host)
  void solve_after_factor(const LdltSystem& sys, const BacksubFuse* riding = nullptr);
  // ---- the one-launch multifrontal step ----
  bool step_possible() const { return m_mode.mf && xg_other() != nullptr; }
  // factor, solve, the riders: one launch.  Returns its workgroups (what a chained sweep after it waits for).
  unsigned int step(const std::vector<double>& delta, const std::vector<double>& gamma, const std::vector<uint8_t>& active,
                    const LdltStepRiders& r);
  // Twin attempt (ldlt_mf_twin_kernel): the policy loop's attempt (delta0, gamma0) and the one it would make next
  // (delta1, gamma1) in ONE launch; `mode` as IpmTwin::mode.  read_stats() then has the first attempt's counters,
  // read_twin_stats() the second's; adopt_twin() makes the second attempt's factor, direction and counters the
  // system's.  twin_available(): false = not possible here (the caller makes a single attempt).
  bool twin_available();
  void step_twin(double delta0, double gamma0, double delta1, double gamma1, int mode, const LdltStepRiders& r);
  LdltStats read_twin_stats() const { return m_h_stats[1]; }
  void adopt_twin();
  // workgroups per CU of the twin kernel that carries the riding error launch, at the larger of the two LDS sizes
  int riding_twin_workgroups_per_cu();
  // the launch that publishes the current attempt's counters was enqueued (seq: the number it leaves in the
  // publication word, one problem)
  void stats_handed_to_host() { m_stats_in_host = true; }
  void stats_handed_to_host(unsigned long long seq) {
    m_stats_seq = seq;
    m_stats_in_host = true;
  }

  // (delta, gamma) of the factorization whose factors of problem b are in memory (NaN: none yet)
  std::pair<double, double> factored_regularization(int b) const {
    if (static_cast<size_t>(b) >= m_fact_delta.size()) return {std::numeric_limits<double>::quiet_NaN(), 0.0};
    return {m_fact_delta[b], m_fact_gamma[b]};
  }
  bool solution_valid() const { return m_solution_valid; }  // some solve has written p
  int twin_mode() const { return m_twin_mode; }             // of the step launch in flight (IpmTwin::mode; 0: a single attempt)
  double* d_p() { return m_p.p; }
  double* d_D() { return m_D.p; }
  double* d_Lx() { return m_Lx.p; }
  const double* d_p_twin() const { return m_p_tw.p; }
  const LdltStats* stats_now() const { return m_stats.p + static_cast<size_t>(m_stats_cur) * m_batch; }  // of the current attempt
  const LdltStats* twin_stats_now() const { return m_stats_tw.p + static_cast<size_t>(m_stats_tw_cur); }
  LdltStats* stats_host() { return m_h_stats; }  // pinned read-back
  void materialize_factor();  // batch-interleaved mode: refresh the batch-major L, D copies
  // For tests of the masked launches (slpx_system_get 12 / 13): what the factorization leaves besides L and D —
  // which 0: z = D⁻¹L⁻¹Pb of the right-hand side that rode in it, [batch][n]; 1: the update blocks handed from round
  // to round, [batch][n_contrib] — batch-major whichever kernels wrote them.  Returns the count per problem.
  size_t download_factor_scratch(int which, std::vector<double>& out);
  // [batch][count] <-> the batch-interleaved layout (il_gather_kernel / il_scatter_kernel)
  void to_interleaved(const double* batch_major, int count, double* il, hipStream_t stream);
  void to_batch_major(const double* il, int count, double* batch_major);
  // returns the clocks recorded so far, then selects the round that records next
  void debug_clocks(unsigned int next_round, unsigned long long* out24);  // phase clocks of workgroup 0 (100 MHz ticks)

  // what a launch changes on the host side of the solver (buffer parities, where the counters are): saved before a
  // speculative launch, put back when the device let it pass
  struct Book {
    int stats_cur, stats_tw_cur, xg_parity, xg_tw_parity, twin_mode;
    bool stats_in_host;
    unsigned long long stats_seq;
    std::pair<double, double> factored;  // factored_regularization(0)
  };
  Book save_book() const {
    return Book{m_stats_cur, m_stats_tw_cur, m_xg_parity, m_xg_tw_parity, m_twin_mode, m_stats_in_host, m_stats_seq, factored_regularization(0)};
  }
  // launch_ran: the launch was not let pass at its gate — it ran with its results held back (a step that carried the
  // error launch deciding about it: MfDev::ride_verdict) and so moved the launch's OWN hand-overs on: the buffers the
  // backward solve hands x through have changed roles for good
  void restore_book(const Book& b, bool launch_ran) {
    m_stats_cur = b.stats_cur;
    m_stats_tw_cur = b.stats_tw_cur;
    if (!launch_ran) {
      m_xg_parity = b.xg_parity;
      m_xg_tw_parity = b.xg_tw_parity;
    }
    m_twin_mode = b.twin_mode;
    m_stats_in_host = b.stats_in_host;
    m_stats_seq = b.stats_seq;
    if (!launch_ran) note_factored(0, b.factored.first, b.factored.second);
  }

 private:
  void write_reg(const std::vector<double>& delta, const std::vector<double>& gamma, const std::vector<uint8_t>& active);
  void enqueue_factor(int parity, hipStream_t stream, const LdltSystem& sys, const KktFuse& f);
  MfDev mf_dev() const;  // the static part: task tables and images
  unsigned int launch_mf_step(int twin_mode, const double* reg, const LdltStepRiders& r);
  void book_mf_step(int twin_mode);
  void download(const double* dev, double* host, size_t count);
  // workgroups of (kernel, threads, dynamic LDS) one CU holds at once; static_lds: the larger of what is there and the kernel's
  int workgroups_per_cu(const void* kernel, int threads, size_t lds, size_t* static_lds = nullptr);

  const LdltPlan& m_l;
  const KktPlan& m_k;
  const int m_batch;
  const int m_nnz_lhs;
  TrackedStream& m_stream;
  LaunchModes& m_mode;
  const PlanFacts& m_facts;
  const Switches& m_sw;
  const int& m_cus;
  volatile unsigned long long* const& m_h_seq;
  const size_t m_n_sums;

  // the plan, and what the hot path hands the kernels of it
  LdltPlanDevice m_lplan;
  LdltDev m_ldev{};
  // the dense branch (LdltPlan::dense, ldlt_dense_kernels.h): the factors of every problem as a dim x dim matrix
  DevBuf<int32_t> m_dense_trans;  // the transpositions of the pivoted factorization (LdltPlan::dense_pivoted)
  DevBuf<double> m_dense_A;
  DevBuf<int32_t> m_dense_colptr, m_dense_rowidx;
  uint32_t m_dense_lds = 0;
  uint32_t m_factor_lds_inline = 0, m_solve_lds_inline = 0;
  // what the factors in memory are factors OF, per problem: written wherever a factorization is enqueued
  std::vector<double> m_fact_delta, m_fact_gamma;
  double m_fact_tw[2] = {0.0, 0.0};  // ... of the second attempt of a twin launch (adopt_twin)
  bool m_solution_valid = false;
  void note_factored(int b, double delta, double gamma) {
    if (m_fact_delta.empty()) {
      m_fact_delta.assign(m_batch, std::numeric_limits<double>::quiet_NaN());
      m_fact_gamma.assign(m_batch, 0.0);
    }
    m_fact_delta[b] = delta;
    m_fact_gamma[b] = gamma;
  }
  // per-batch values
  DevBuf<double> m_p, m_D, m_Lx, m_contrib, m_scontrib, m_zv, m_xg;
  DevBuf<LdltStats> m_stats;  // 2 x batch, double-buffered per factorization attempt
  int m_stats_cur = 0;
  DevBuf<double> m_reg_dev;           // device copy of m_h_reg for big batches
  std::vector<double> m_reg_shadow;   // what m_reg_dev holds (enqueue_factor)
  double* m_h_reg = nullptr;          // pinned, read by the kernels: (delta, gamma) per problem;
                                      // delta = NaN: skip the problem
  LdltStats* m_h_stats = nullptr;     // pinned read-back
  bool m_stats_in_host = false;       // the last launch already copied the counters out
  unsigned long long m_stats_seq = 0; // the publishing launch that carries the current inertia counters (one problem)
  // backward solve: x of finished columns handed to the descendants through the values (two
  // buffers, the solves alternate)
  int m_xg_parity = 0;
  DevBuf<double> m_xg2;
  double* xg_now() const { return (m_mode.xg_by_data && m_xg_parity) ? m_xg2.p : m_xg.p; }
  double* xg_other() const {
    if (!m_mode.xg_by_data) return nullptr;
    return m_xg_parity ? m_xg.p : m_xg2.p;
  }
  void xg_flip() {
    if (m_mode.xg_by_data) m_xg_parity ^= 1;
  }
  DevBuf<unsigned int> m_exit_cnt;
  // multifrontal step (ldlt_mf_kernels.h: ldlt_mf_step_kernel; SLPX_LDLT_MF=0: the pair lists)
  uint32_t m_mf_lds = 0;
  DevBuf<LdltMfTask> m_mf_tasks;
  DevBuf<LdltFront> m_mf_fronts;
  uint32_t m_mf_image_stride16 = 0;
  DevBuf<uint4> m_mf_image;        // per task: everything static it keeps in LDS, in LDS order (one copy loop)
  DevBuf<uint4> m_mf_image_desc;   // per task {first 16-byte group, groups up to the end of the KKT terms, groups of back-substitution rows, terms groups}
  DevBuf<double> m_mf_contrib;
  // the second attempt of a twin launch: its own factor, update slots, x hand-over (a pair, alternating like
  // m_xg / m_xg2), direction and counters (a pair, alternating like m_stats)
  int m_twin_mode = 0;
  DevBuf<double> m_Lx_tw, m_D_tw, m_zv_tw, m_p_tw, m_mf_contrib_tw, m_xg_tw, m_xg2_tw;
  DevBuf<LdltStats> m_stats_tw;
  int m_stats_tw_cur = 0, m_xg_tw_parity = 0;
  // batch-interleaved LDLT (ldlt_il_kernels.h)
  bool m_il_outputs_stale = false;
  DevBuf<double> m_Lx_il, m_D_il, m_contrib_il, m_scontrib_il, m_zv_il, m_xg_il;
  DevBuf<LdltStats> m_stats_part;  // [task][problem]
  DevBuf<uint32_t> m_il_meta, m_il_meta_off;  // per task: the plan slices the factor kernel stages
  uint32_t m_il_factor_lds = 0, m_il_solve_lds = 0;
  DevBuf<unsigned int> m_fround_cnt, m_bround_cnt;  // [2][batch][n_rounds]
};

}  // namespace slpx
