#include "newton.hpp"

#include "restoration.hpp"

#include "setup_timing.hpp"

#include <algorithm>
#include <future>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

namespace slpx {

// The plan of choose_ldlt_plan (system_choice.cpp), with its one diagnostic
static LdltPlan plan_for(const KktPlan& k, int n_dec, bool reference_takes_dense, const std::vector<int32_t>* user_perm,
                         const std::vector<uint8_t>& diag_has_source, int batch, const LdltOptions& lopt, const LdltOptions* pair_retry,
                         const Switches& sw) {
  std::string dense_because;
  LdltPlan l = choose_ldlt_plan(k.lhs, n_dec, reference_takes_dense, user_perm, &diag_has_source, batch, lopt, pair_retry, sw, &dense_because);
  if (!dense_because.empty() && std::getenv("SLPX_LDLT_VERBOSE"))
    std::fprintf(stderr, "ldlt: %s — the system of order %d is factored as a dense matrix\n", dense_because.c_str(), k.lhs.cols);
  return l;
}

NewtonSystem::NewtonSystem(Graph& g, const std::vector<NodeId>& x, NodeId f,
                           const std::vector<NodeId>& c_e, const std::vector<NodeId>& c_i,
                           const NewtonOptions& opt, const std::vector<int32_t>* user_perm, bool defer_device)
    : m_opt(opt), m_sw(Switches::from_environment()), m_graph(&g), m_x_nodes(x), m_ce_nodes(c_e), m_ci_nodes(c_i) {
  SetupLap lap;
  // the HIP runtime comes up (context, first allocation: 50-700 ms in a fresh process) while the
  // host compiles the model
  std::future<void> device_job;
  if (!defer_device)
    device_job = std::async(std::launch::async, [device = opt.device] {
      if (hipSetDevice(device) == hipSuccess) (void)hipFree(nullptr);
      (void)hipGetLastError();
    });
  // the KKT plan and the symbolic factorization (25 ms at N=1000) alongside the tape compiler
  auto plan_linear_algebra = [&](const NlpStructure& st) {
    m_k = build_kkt_plan(st);
    // which diagonal entries of the unregularized lhs have any source at all
    std::vector<uint8_t> diag_has_source(m_k.dim, 0);
    for (int c = 0; c < m_k.dim; ++c)
      for (int p = m_k.lhs.colptr[c]; p < m_k.lhs.colptr[c + 1]; ++p)
        if (m_k.lhs.rowidx[p] == c)
          diag_has_source[c] = (m_k.dptr[p + 1] > m_k.dptr[p]) || (m_k.pptr[p + 1] > m_k.pptr[p]);
    const LdltOptions lopt = choose_ldlt_options(opt.ldlt, opt.batch, m_k.dim, /*compiled_model=*/true, m_sw);
    const LdltOptions pair = pair_list_options(opt.ldlt, lopt);
    m_l = plan_for(m_k, st.n, m_k.reference_takes_dense(st.Ae.nnz()), user_perm, diag_has_source, opt.batch, lopt, &pair, m_sw);
  };
  m_s = build_nlp_structure(g, x, f, c_e, c_i, opt.tape, plan_linear_algebra);
  lap("= AD structure + tape compile, KKT plan, LDLT symbolic");
  reset_regularization();
  if (defer_device) return;
  device_job.get();
  finish_device();
}

NewtonSystem::~NewtonSystem() = default;

FrDevice& NewtonSystem::restoration_device() {
  if (!m_fr) m_fr = std::make_unique<FrDevice>(*m_dev);
  return *m_fr;
}

void NewtonSystem::finish_device() {
  if (m_dev) return;
  SetupLap lap;
  m_dev = std::make_unique<DeviceNlp>(m_s, m_k, m_l, m_opt.batch, m_opt.device, m_sw);
  lap("= device upload + tape JIT");
}

NewtonSystem::NewtonSystem(const CscPattern& lower, int n_dec, int m_e, const NewtonOptions& opt)
    : m_opt(opt), m_sw(Switches::from_environment()) {
  if (lower.cols != n_dec + m_e || lower.rows != lower.cols)
    throw std::runtime_error("slpx: the matrix must be square of order n + m_e");
  m_opt.batch = std::max(1, opt.batch);
  const int dim = n_dec + m_e;
  // the structure a DeviceNlp expects, with nothing in it but the sizes
  m_s.n = n_dec;
  m_s.m_e = m_e;
  m_s.m_i = 0;
  m_s.nV = 1;
  m_s.V_static_raw.assign(1, 0.0);
  m_s.V_scale_idx.assign(1, -1);
  m_s.V_is_static.assign(1, 1);
  auto empty = [](int rows, int cols) {
    CscPattern p;
    p.rows = rows;
    p.cols = cols;
    p.colptr.assign(cols + 1, 0);
    return p;
  };
  m_s.g_pat = empty(1, n_dec);
  m_s.Ae = empty(m_e, n_dec);
  m_s.Ai = empty(0, n_dec);
  m_s.Hf = empty(n_dec, n_dec);
  m_s.Hc = empty(n_dec, n_dec);
  // pattern = the caller's lower triangle plus any missing diagonal entry
  m_k.n = n_dec;
  m_k.m_e = m_e;
  m_k.m_i = 0;
  m_k.dim = dim;
  std::vector<uint8_t> diag_has_source;
  m_k.lhs = complete_diagonal(lower, m_user_lhs_map, diag_has_source);
  const int nnz = m_k.lhs.nnz();
  m_k.dptr.assign(nnz + 1, 0);
  m_k.pptr.assign(nnz + 1, 0);
  m_k.fast_src.assign(nnz, -1);
  m_k.g_src.assign(n_dec, -1);
  m_k.ai_rowptr.assign(1, 0);
  m_k.ae_rowptr.assign(m_e + 1, 0);
  const LdltOptions lopt = choose_ldlt_options(opt.ldlt, opt.batch, dim, /*compiled_model=*/false, m_sw);
  m_l = plan_for(m_k, n_dec, /*reference_takes_dense=*/false, nullptr, diag_has_source, m_opt.batch, lopt, nullptr, m_sw);
  m_dev = std::make_unique<DeviceNlp>(m_s, m_k, m_l, m_opt.batch, opt.device, m_sw);
  m_dev->set_scaling(std::vector<double>(m_s.n_scales(), 1.0));
  reset_regularization();
}

void NewtonSystem::reset_regularization() {
  m_prev_delta.assign(m_opt.batch, 0.0);
  m_prev_gamma.assign(m_opt.batch, 0.0);
}

// sparse_regularized_ldlt.hpp:64-152 is ldlt_policy.hpp: one LdltPolicy per problem and the loops that run it.  What
// follows are their launchers: what a factorization attempt is on the device for each kind of caller.
LdltPolicy NewtonSystem::start_policy(int b, bool skip_first) const {
  LdltPolicy p;
  p.start(m_s.n, m_s.m_e, m_prev_delta[b], m_prev_gamma[b], m_gamma_min, skip_first);
  return p;
}
// First attempt (:74-87): when the symbolic phase proved that a pivot is structurally zero the attempt is known to
// end in NumericalIssue (Eigen reports failure on an exactly-zero pivot), so it is not launched.
bool NewtonSystem::skip_first() const { return m_opt.skip_structurally_singular_attempt && m_l.structurally_singular_unregularized; }

// The counters of the attempt `once()` has just launched.  A chained step (DeviceNlp::sweep_full_for_step) whose sweep
// or step kernel gave up waiting for the other reports kLdltChainFailure instead of a silent wrong step: the attempt
// is redone — V swept again from the unchanged state, the system rebuilt — with the chain off.
template <class Once>
void NewtonSystem::read_stats_redoing_a_failed_chain(std::vector<LdltStats>& stats, Once&& once) {
  m_dev->ldlt().read_stats(stats);
  if (m_opt.batch != 1 || (stats[0].n_bad & kLdltChainFailure) == 0) return;
  m_dev->recover_from_chain_failure();
  m_dev->build_kkt_for_step(/*with_reduce=*/true);
  once();
  m_dev->ldlt().read_stats(stats);
}

std::vector<FactorInfo> NewtonSystem::compute(bool solve_speculatively) {
  return compute_impl(solve_speculatively ? 1 : 0);
}

// mode 0: factorization attempts only; 1: each attempt followed by solve + backsub.
std::vector<FactorInfo> NewtonSystem::compute(bool solve_speculatively, const std::vector<uint8_t>& mask) {
  if (static_cast<int>(mask.size()) != m_opt.batch) throw std::runtime_error("NewtonSystem::compute: mask length");
  return compute_impl(solve_speculatively ? 1 : 0, &mask);
}
// Every problem of the batch at once: each trip through ldlt_run_batch is one device factorization of the
// still-active problems followed by one small stats read-back.
std::vector<FactorInfo> NewtonSystem::compute_impl(int mode, const std::vector<uint8_t>* mask) {
  const int B = m_opt.batch;
  m_last_twin_launches = m_last_twin_taken = 0;
  if (mode == 1 && B == 1 && m_twin_attempts && !mask && m_dev->ldlt().twin_available()) return compute_twin();
  std::vector<uint8_t> active = mask ? *mask : std::vector<uint8_t>(B, 1);
  std::vector<LdltPolicy> pol(B);
  for (int b = 0; b < B; ++b)
    if (active[b]) pol[b] = start_policy(b, skip_first());
  const std::vector<uint8_t> started = active;
  std::vector<LdltStats> stats;
  m_last_factorizations = ldlt_run_batch(pol, active, !skip_first(), [&](const std::vector<double>& d, const std::vector<double>& g, const std::vector<uint8_t>& a) {
    // With mode 1 every factorization attempt is followed at once by the triangular solves and the
    // back-substitution, BEFORE the host has read the inertia counters: the device never idles through the host
    // round trip, and in the usual case (first attempt accepted) the step is complete when the counters arrive.
    // A rejected attempt just has its solve overwritten by the next one.
    auto once = [&] {
      if (mode == 0) {
        m_dev->factor(d, g, a);
      } else {
        m_dev->factor_solve_publish(d, g, a);
        if (m_after_attempt) m_after_attempt();
      }
    };
    once();
    read_stats_redoing_a_failed_chain(stats, once);
    return stats.data();
  });
  std::vector<FactorInfo> info(B, FactorInfo::Success);
  for (int b = 0; b < B; ++b)
    if (started[b]) info[b] = remember(b, pol[b]);
  return info;
}
FactorInfo NewtonSystem::remember(int b, const LdltPolicy& p) {
  m_prev_delta[b] = p.prev_delta;
  m_prev_gamma[b] = p.prev_gamma;
  return p.info;
}

// What compute_twin's first launch is, from the policy's memory: ipm_lookahead_kernel makes the choice between its
// two attempts on the device from the same counters and the same predicates (ldlt_policy.hpp).
LdltLaunch NewtonSystem::twin_first_launch() const { return start_policy(0, skip_first()).launch(m_twin_expect); }

bool NewtonSystem::begin_speculative_compute(bool gated) {
  if (m_spec.valid || m_opt.batch != 1 || !m_twin_attempts || !m_dev->ldlt().twin_available()) {
    m_dev->ipm_ride_disarm();
    return false;
  }
  const LdltLaunch tl = twin_first_launch();
  const DeviceNlp::LaunchBook book = m_dev->save_book();
  m_dev->build_kkt_for_step(/*with_reduce=*/false);
  m_dev->ipm_gate_next_step(gated);
  if (!m_dev->factor_solve_publish_twin(tl.d0, tl.g0, tl.d1, tl.g1, tl.mode)) {
    m_dev->ipm_gate_next_step(false);
    m_dev->ipm_ride_disarm();
    m_dev->restore_book(book);
    return false;
  }
  if (m_after_attempt) m_after_attempt();
  m_spec.valid = true;
  m_spec.have_second = true;
  m_spec.launch = tl;
  m_spec.book = book;
  return true;
}

void NewtonSystem::cancel_speculative_compute(bool launch_ran) {
  if (!m_spec.valid) return;
  m_dev->restore_book(m_spec.book, launch_ran);
  m_spec.valid = false;
}

// ldlt_run_twin's launcher for the system the device's V, s, y, z describe (set_twin_attempts)
struct NewtonSystem::TwinLauncher {
  NewtonSystem& sys;
  std::vector<LdltStats> stats;
  LdltStats second_stats{};
  bool first_launch = true;

  bool launch(const LdltLaunch& tl) {
    DeviceNlp& dev = *sys.m_dev;
    // (a later launch of the loop evaluates the system from V again, inside the launch, like the first — instead of
    // two assembly launches first)
    if (!first_launch) dev.build_kkt_for_step(/*with_reduce=*/false);
    first_launch = false;
    bool have_second = false;
    auto once = [&] {
      have_second = dev.factor_solve_publish_twin(tl.d0, tl.g0, tl.d1, tl.g1, tl.mode);
      if (!have_second) dev.factor_solve_publish({tl.d0}, {tl.g0}, {1});
      if (sys.m_after_attempt) sys.m_after_attempt();
    };
    if (sys.m_spec.valid) {
      // this launch — the policy's first of this compute — was made ahead (begin_speculative_compute) and has run
      if (sys.m_spec.launch != tl) throw std::runtime_error("slpx: the step enqueued ahead is not the one the regularization policy makes");
      sys.m_spec.valid = false;
      have_second = sys.m_spec.have_second;
    } else {
      once();
    }
    // (a twin launch itself is never chained, the single-attempt fallback of once() can be)
    sys.read_stats_redoing_a_failed_chain(stats, once);
    if (!have_second) return false;
    second_stats = dev.ldlt().read_twin_stats();
    const int n = sys.m_s.n, m_e = sys.m_s.m_e;
    const LdltVerdict v = ldlt_judge(stats[0], n, m_e, tl.mode == 2);
    ++sys.m_twin_hist[v == kLdltAccepted || v == kLdltFailed ? v
                      : v == kLdltZeroPivots               ? 3
                      : !ldlt_second_stands(tl.mode, v)     ? 4
                                                            : (ldlt_ideal(second_stats, n, m_e) ? 1 : 2)];
    return true;
  }
  const LdltStats& first() const { return stats[0]; }
  const LdltStats& second() const { return second_stats; }
  void adopt_second() { sys.m_dev->adopt_twin(); }
};

std::vector<FactorInfo> NewtonSystem::compute_twin() {
  LdltPolicy pol = start_policy(0, skip_first());
  TwinLauncher launcher{*this};
  return finish_twin_run(pol, ldlt_run_twin(pol, launcher, &m_twin_expect));
}
std::vector<FactorInfo> NewtonSystem::finish_twin_run(const LdltPolicy& pol, const LdltTwinRun& run) {
  m_last_factorizations = pol.factorizations;
  m_last_twin_launches = run.launches;
  m_last_twin_taken = run.taken;
  return {remember(0, pol)};
}

// ldlt_run_twin's launcher for a caller that writes the system of every attempt itself (AttemptHooks)
struct NewtonSystem::HookedLauncher {
  NewtonSystem& sys;
  const AttemptHooks& hooks;
  const bool twin;
  std::vector<LdltStats> stats;
  LdltStats second_stats{};
  bool first_launch = true;

  bool launch(const LdltLaunch& tl) {
    DeviceNlp& dev = *sys.m_dev;
    bool have_second = false;
    if (twin) {
      const double *lhs2 = nullptr, *rhs2 = nullptr;
      if (hooks.prepare_pair) {
        hooks.prepare_pair(tl.d0, tl.g0, tl.d1, tl.g1, &lhs2, &rhs2);
      } else {
        hooks.prepare(tl.d0, tl.g0);
        hooks.prepare_second(tl.d1, tl.g1, &lhs2, &rhs2);
      }
      have_second = dev.factor_solve_publish_twin_written(tl.d0, tl.g0, tl.d1, tl.g1, tl.mode, lhs2, rhs2);
    } else {
      hooks.prepare(tl.d0, tl.g0);
    }
    if (!have_second) dev.factor_solve_publish({tl.d0}, {tl.g0}, {1});
    // (`after` behind the FIRST launch only: a caller that expects its first attempt to be taken; the launches of a
    // ladder would each drag a chain nobody reads)
    if (hooks.after && first_launch) hooks.after(tl.d0, tl.g0);
    first_launch = false;
    dev.ldlt().read_stats(stats);
    if (have_second) second_stats = dev.ldlt().read_twin_stats();
    return have_second;
  }
  const LdltStats& first() const { return stats[0]; }
  const LdltStats& second() const { return second_stats; }
  void adopt_second() { sys.m_dev->adopt_twin(); }
};

std::vector<FactorInfo> NewtonSystem::compute_hooked(const AttemptHooks& hooks) {
  if (m_opt.batch != 1) throw std::runtime_error("slpx: compute_hooked handles one problem");
  m_hooked_chain_valid = false;
  LdltPolicy pol = start_policy(0, /*skip_first=*/false);
  HookedLauncher launcher{*this, hooks, static_cast<bool>(hooks.prepare_second) && m_dev->ldlt().twin_available()};
  const double extra = hooks.eliminated_min_pivot ? hooks.eliminated_min_pivot() : std::numeric_limits<double>::infinity();
  // (later launches hold the attempt and its delta x 10 only: no memory of what the loop's first attempt drew)
  const LdltTwinRun run = ldlt_run_twin(pol, launcher, nullptr, extra);
  m_hooked_chain_valid = hooks.after && pol.factorizations == 1;  // the accepted attempt is the one `after` followed
  return finish_twin_run(pol, run);
}

std::vector<FactorInfo> NewtonSystem::compute_hooked_batch(const BatchPrepare& prepare, const std::vector<uint8_t>& mask,
                                                           const std::vector<double>& eliminated_min_pivot) {
  const int B = m_opt.batch;
  if (static_cast<int>(mask.size()) != B || static_cast<int>(eliminated_min_pivot.size()) != B)
    throw std::runtime_error("NewtonSystem::compute_hooked_batch: one entry per problem");
  m_last_twin_launches = m_last_twin_taken = 0;
  std::vector<uint8_t> active = mask;
  std::vector<LdltPolicy> pol(B);
  for (int b = 0; b < B; ++b)
    if (active[b]) pol[b] = start_policy(b, /*skip_first=*/false);
  const std::vector<uint8_t> started = active;
  std::vector<LdltStats> stats;
  m_last_factorizations = ldlt_run_batch(
      pol, active, /*launch_for_nobody=*/false,
      [&](const std::vector<double>& d, const std::vector<double>& g, const std::vector<uint8_t>& a) {
        prepare(d, g, a);
        m_dev->system_written_by_caller(true, true);
        m_dev->factor(d, g, a);
        m_dev->ldlt().read_stats(stats);
        return stats.data();
      },
      &eliminated_min_pivot);
  // (a problem accepted in an earlier launch kept its factors and its right-hand side: later launches skip it)
  if (m_last_factorizations > 0) m_dev->solve();
  std::vector<FactorInfo> info(B, FactorInfo::Success);
  for (int b = 0; b < B; ++b)
    if (started[b]) info[b] = remember(b, pol[b]);
  return info;
}

bool NewtonSystem::factor_unregularized() {
  const int B = m_opt.batch;
  std::vector<double> zero(B, 0.0);
  std::vector<uint8_t> active(B, 1);
  m_dev->factor(zero, zero, active);
  std::vector<LdltStats> stats;
  m_dev->ldlt().read_stats(stats);
  ++m_last_factorizations;
  return std::all_of(stats.begin(), stats.begin() + B, [&](const LdltStats& st) { return ldlt_ideal(st, m_s.n, m_s.m_e); });
}

NewtonSystem::Refinement NewtonSystem::refine(int max_steps, const std::vector<uint8_t>* mask) {
  const int B = m_opt.batch;
  if (max_steps < 0) throw std::runtime_error("slpx: refine: max_steps must not be negative");
  if (mask && static_cast<int>(mask->size()) != B) throw std::runtime_error("slpx: refine: mask length");
  Refinement out;
  out.max_steps = max_steps;
  out.norms.assign(static_cast<size_t>(B) * (max_steps + 1), std::numeric_limits<double>::quiet_NaN());
  out.accepted.assign(B, 0);
  std::vector<uint8_t> active = mask ? *mask : std::vector<uint8_t>(B, 1);
  std::vector<double> norm(B), trial(B);
  m_dev->residual(active, norm);
  for (int b = 0; b < B; ++b)
    if (active[b]) {
      out.norms[static_cast<size_t>(b) * (max_steps + 1)] = norm[b];
      // nothing to gain (an exact solution keeps its bits) or nothing to measure a gain against
      if (norm[b] == 0.0 || !std::isfinite(norm[b])) active[b] = 0;
    }
  if (max_steps == 0 || std::none_of(active.begin(), active.end(), [](uint8_t a) { return a != 0; })) return out;
  m_dev->refine_begin();
  for (int k = 0; k < max_steps; ++k) {
    if (std::none_of(active.begin(), active.end(), [](uint8_t a) { return a != 0; })) break;
    m_dev->refine_solve_correction();
    m_dev->refine_apply(active);  // the candidates
    m_dev->residual(active, trial);
    bool rejected = false;
    for (int b = 0; b < B; ++b) {
      if (!active[b]) continue;
      out.norms[static_cast<size_t>(b) * (max_steps + 1) + k + 1] = trial[b];
      if (std::isfinite(trial[b]) && trial[b] < norm[b]) {
        norm[b] = trial[b];
        ++out.accepted[b];
        if (trial[b] == 0.0) active[b] = 0;  // (taken; nothing left to refine)
      } else {
        active[b] = 0;
        rejected = true;
      }
    }
    if (rejected) {
      // p = kept p + d once more for the problems that took the step (the same bits), the kept p for the others
      std::vector<uint8_t> took(B, 0);
      for (int b = 0; b < B; ++b) took[b] = out.accepted[b] == k + 1 ? 1 : 0;
      m_dev->refine_apply(took);
    }
    m_dev->refine_keep_solution();
  }
  return out;
}

void NewtonSystem::run_norm_estimator(std::vector<NormEstState>& est, bool scale_by_f) {
  const int B = m_opt.batch;
  const auto all_done = [&] { return std::all_of(est.begin(), est.end(), [](const NormEstState& e) { return e.done(); }); };
  if (all_done()) return;
  std::vector<DeviceNlp::EstRound> rounds(B);
  std::vector<DeviceNlp::EstScalars> scal;
  std::vector<int32_t> kept(B, 0);
  m_dev->refine_begin();  // keeps p and rhs
  // (every state machine ends within 11 rounds; the bound only guards the loop)
  for (int k = 0; k < 2 * kNormEstIterations + 2 && !all_done(); ++k) {
    for (int b = 0; b < B; ++b) {
      rounds[b].kind = est[b].probe();
      rounds[b].j = est[b].probe() == kProbeUnit ? est[b].unit_index() : 0;
      // ||diag(f) Kreg^-1||_1: the product with it scales the solution, the product with its transpose the probe
      rounds[b].scale = !scale_by_f ? 0 : est[b].transposed() ? 1 : 2;
      rounds[b].kept = kept[b];
    }
    m_dev->errbound_round(rounds, scal);
    for (int b = 0; b < B; ++b) {
      if (est[b].done()) continue;
      if (est[b].advance(scal[b].norm1, scal[b].argmax, scal[b].signs_repeated, scal[b].finite)) kept[b] ^= 1;
    }
  }
  m_dev->errbound_restore();
}

NewtonSystem::ErrorBounds NewtonSystem::error_bounds(const std::vector<uint8_t>* mask, bool want_ferr) {
  const int B = m_opt.batch;
  if (mask && static_cast<int>(mask->size()) != B) throw std::runtime_error("slpx: error_bounds: mask length");
  const std::vector<uint8_t> active = mask ? *mask : std::vector<uint8_t>(B, 1);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  ErrorBounds out;
  out.berr.assign(B, nan);
  out.ferr.assign(B, nan);
  out.solves.assign(B, 0);
  std::vector<double> norm;
  m_dev->residual(active, norm);
  std::vector<DeviceNlp::ErrRowScalars> rows;
  m_dev->errbound_rows(active, /*want_bounds=*/true, rows);
  for (int b = 0; b < B; ++b)
    if (active[b]) out.berr[b] = rows[b].berr;
  if (!want_ferr) return out;
  std::vector<NormEstState> est(B, NormEstState(m_k.dim));
  for (int b = 0; b < B; ++b) {
    if (!active[b]) est[b].finish(nan);
    // no scale to measure against: 0 if nothing is to be measured, +inf otherwise (a NaN in f stays one)
    else if (rows[b].p_inf == 0.0) est[b].finish(rows[b].f_inf == 0.0 ? 0.0 : rows[b].f_inf != rows[b].f_inf ? nan : std::numeric_limits<double>::infinity());
  }
  run_norm_estimator(est, /*scale_by_f=*/true);
  for (int b = 0; b < B; ++b) {
    if (!active[b]) continue;
    out.ferr[b] = rows[b].p_inf == 0.0 ? est[b].estimate() : est[b].estimate() / rows[b].p_inf;
    out.solves[b] = est[b].solves();
  }
  return out;
}

NewtonSystem::Condest NewtonSystem::condest(const std::vector<uint8_t>* mask) {
  const int B = m_opt.batch;
  if (mask && static_cast<int>(mask->size()) != B) throw std::runtime_error("slpx: condest: mask length");
  const std::vector<uint8_t> active = mask ? *mask : std::vector<uint8_t>(B, 1);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  Condest out;
  out.norm1.assign(B, nan);
  out.inv_norm1.assign(B, nan);
  out.solves.assign(B, 0);
  std::vector<DeviceNlp::ErrRowScalars> rows;
  m_dev->errbound_rows(active, /*want_bounds=*/false, rows);
  std::vector<NormEstState> est(B, NormEstState(m_k.dim));
  for (int b = 0; b < B; ++b)
    if (!active[b]) est[b].finish(nan);
  run_norm_estimator(est, /*scale_by_f=*/false);
  for (int b = 0; b < B; ++b) {
    if (!active[b]) continue;
    out.norm1[b] = rows[b].norm1;
    out.inv_norm1[b] = est[b].estimate();
    out.solves[b] = est[b].solves();
  }
  return out;
}

std::vector<FactorInfo> NewtonSystem::newton_step(bool refresh_ad) {
  // SLPX_HOST_TIMING=1: where the host's time per step goes (printed every 1000 steps)
  static const bool timing = std::getenv("SLPX_HOST_TIMING") != nullptr;
  if (!timing) {
    if (refresh_ad) m_dev->sweep_full_for_step();
    m_dev->build_kkt_for_step(/*with_reduce=*/refresh_ad);
    return compute(/*solve_speculatively=*/true);
  }
  using clk = std::chrono::steady_clock;
  static double t_sweep = 0, t_rest = 0;
  static long n = 0;
  const auto t0 = clk::now();
  if (refresh_ad) m_dev->sweep_full_for_step();
  const auto t1 = clk::now();
  m_dev->build_kkt_for_step(/*with_reduce=*/refresh_ad);
  auto res = compute(/*solve_speculatively=*/true);
  const auto t2 = clk::now();
  t_sweep += std::chrono::duration<double, std::micro>(t1 - t0).count();
  t_rest += std::chrono::duration<double, std::micro>(t2 - t1).count();
  if (++n % 1000 == 0) {
    std::fprintf(stderr, "slpx host timing: sweep launch %.2f us, launch + wait for the verdict %.2f us per step\n",
                 t_sweep / 1000, t_rest / 1000);
    t_sweep = t_rest = 0;
  }
  return res;
}

}  // namespace slpx
