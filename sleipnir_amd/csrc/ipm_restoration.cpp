// The host side of feasibility restoration (util/feasibility_restoration.hpp:26-628): what a phase
// starts from, its iteration on the outer problem's compiled system (restoration.hpp: FrDevice), the least-squares
// multiplier estimate that ends it, and the entry points of ipm.hpp that hand its pieces to the batched loop and the tests.
#include "ipm_drivers.hpp"

#include "ipm_formulas.h"
#include "restoration.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace slpx {

namespace {

using namespace ipm_host;
using Want = LineSearch::Want;
using End = LineSearch::End;

// feasibility_restoration.hpp:26-101: p, n >= 0 with p - n = c minimising the barrier
// problem  rho (p + n) - mu (ln p + ln n)
void compute_p_n(const Vec& c, double rho, double mu, Vec& p, Vec& n) {
  p.resize(c.size());
  n.resize(c.size());
  for (size_t row = 0; row < c.size(); ++row) {
    const double a_ = rho, b_ = rho * c[row] - mu, c_ = -mu * c[row] / 2.0;
    n[row] = (-b_ + std::sqrt(b_ * b_ - 4.0 * a_ * c_)) / (2.0 * a_);
    p[row] = c[row] + n[row];
  }
}

}  // namespace

// feasibility_restoration.hpp:391-432: what a restoration phase starts from (ipm.hpp)
RestorationEntry restoration_entry(const NlpStructure& ost, const Vec& scales, const Vec& x, const Vec& s, double mu, const Vec& c_e,
                                   const Vec& c_i) {
  const int n = ost.n, m_e = ost.m_e, m_i = ost.m_i, M = 2 * m_e + 2 * m_i;
  constexpr double rho = 1e3;
  RestorationEntry out;

  Vec cis(m_i);
  for (int j = 0; j < m_i; ++j) cis[j] = c_i[j] - s[j];
  const double fr_mu = std::max({mu, norm_inf(c_e.data(), m_e), norm_inf(cis.data(), m_i)});  // :396-397
  const double zeta = std::sqrt(fr_mu);
  out.fr_mu = fr_mu;

  Vec p_e, n_e, p_i, n_i;
  compute_p_n(c_e, rho, fr_mu, p_e, n_e);  // :400-401
  compute_p_n(cis, rho, fr_mu, p_i, n_i);

  // the restoration iterate (:408-423): X = [x | p_e | n_e | p_i | n_i], S = [s | 1...], y = 0, Z = fr_mu / S (.. / p, n)
  Vec& X = out.X;
  X.reserve(n + M);
  for (const Vec* v : {static_cast<const Vec*>(&x), static_cast<const Vec*>(&p_e), static_cast<const Vec*>(&n_e),
                       static_cast<const Vec*>(&p_i), static_cast<const Vec*>(&n_i)})
    X.insert(X.end(), v->begin(), v->end());
  out.S.assign(m_i + M, 1.0);
  out.y.assign(m_e, 0.0);
  Vec& Z = out.Z;
  std::copy(s.begin(), s.end(), out.S.begin());
  Z.reserve(m_i + M);
  for (int j = 0; j < m_i; ++j) Z.push_back(fr_mu * (1.0 / s[j]));
  for (int e = 0; e < M; ++e) Z.push_back(fr_mu * (1.0 / X[n + e]));
  out.x_r = x;
  Vec& w = out.w;
  w.resize(n);
  for (int k = 0; k < n; ++k) w[k] = zeta * std::min(1.0 / (x[k] * x[k]), 1.0);  // zeta D_R (:404-405)

  // the error measure un-scales with {1, d_ce, [d_ci, 1...]} (:425-432); the bound rows' 1 is implied
  Vec& fr_scales = out.fr_scales;
  fr_scales.assign(1 + m_e + m_i, 1.0);
  for (int j = 0; j < m_e; ++j) fr_scales[1 + j] = scales[1 + j];
  for (int j = 0; j < m_i; ++j) fr_scales[1 + m_e + j] = scales[1 + m_e + j];
  return out;
}

namespace {

// (the restoration problem itself is never built as a model: restoration.hpp — its extra variables are eliminated from
// the Newton-KKT system in closed form and the rest runs on the outer problem's own compiled system)

// util/lagrange_multiplier_estimate.hpp:56-133: least-squares (y, z) of
//   [A_e 0; A_i -S] [A_e 0; A_i -S]^T [y; z] = [A_e 0; A_i -S] [g; -mu 1].
// Eliminating the auxiliary unknowns of the equivalent equality-constrained QP gives a
// system with the KKT pattern this NewtonSystem already has a symbolic factorization for:
//   [I + A_i^T S^-2 A_i   A_e^T] [ d ]   [-g + mu A_i^T S^-1 1]
//   [A_e                  0    ] [-y ] = [0                   ],  z = mu S^-1 1 - S^-2 A_i d
// V must hold g, A_e, A_i at the current x.
bool lagrange_multiplier_estimate(NewtonSystem& sys, const Vec& V, const Vec& s, double mu, Vec& y,
                                  Vec& z, SolveReport& rep) {
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n, m_e = st.m_e, m_i = st.m_i, dim = n + m_e;
  VView cur{st, V};
  Vec rhs(dim, 0.0), sinv_mu(m_i);
  const Vec g = cur.g_dense();
  for (int i = 0; i < n; ++i) rhs[i] = -g[i];
  for (int j = 0; j < m_i; ++j) sinv_mu[j] = mu / s[j];
  add_At_v(st.Ai, cur.Ai(), nullptr, sinv_mu.data(), 1.0, rhs);

  Vec zeros_e(std::max(1, m_e), 0.0), ones_i(std::max(1, m_i), 1.0);
  dev.upload_duals(s.data(), zeros_e.data(), ones_i.data());
  dev.assemble_lsq();
  SLPX_HIP_CHECK(hipMemcpyAsync(dev.d_rhs(), rhs.data(), dim * sizeof(double), hipMemcpyHostToDevice,
                                dev.stream()));
  // The reference factors this system without any regularization (a SimplicialLDLT of its own,
  // :107): the top-left block I + A_i^T S^-2 A_i is positive definite, so delta = gamma = 0 is
  // tried first whatever the KKT pattern's structural zeros say — starting the usual loop at
  // delta = 1e-4 instead perturbed the estimate by 1e-4 relative (tests/test_restoration_gpu.py).
  // Only a rank-deficient A_e falls back to the regularizing loop, with its own history.
  // Only when that breaks down (a constraint row the elimination order could not pair with a
  // variable is a zero pivot without gamma; a rank-deficient A_e) the regularizing loop runs,
  // with its own history — and three steps of iterative refinement against the unregularized
  // matrix take its delta, gamma out of the answer again.
  bool regularized = false;
  if (sys.factor_unregularized()) {
    ++rep.factorizations;
  } else {
    const auto saved = sys.regularization_state();
    sys.reset_regularization();
    const auto info = sys.compute();
    rep.factorizations += 1 + sys.last_factorizations();
    sys.set_regularization_state(saved);
    if (info[0] != FactorInfo::Success) return false;
    regularized = true;
  }
  dev.solve();
  ++rep.solves;
  if (regularized) {
    dev.refine_solution(3);
    rep.solves += 3;
  }
  Vec p(dim);
  dev.download(dev.ldlt().d_p(), p.data(), dim);
  y.assign(m_e, 0.0);
  for (int j = 0; j < m_e; ++j) y[j] = -p[n + j];
  Vec aid(m_i, 0.0);
  for (int c = 0; c < n; ++c)
    for (int q = st.Ai.colptr[c]; q < st.Ai.colptr[c + 1]; ++q) aid[st.Ai.rowidx[q]] += cur.Ai()[q] * p[c];
  z.assign(m_i, 0.0);
  for (int j = 0; j < m_i; ++j) {
    z[j] = z_reset(mu / s[j] - aid[j] / (s[j] * s[j]), mu, s[j]);  // :125-130
  }
  return true;
}

// The restoration problem as the user's iteration callbacks see it (slpx.h: slpx_iteration_info inside restoration):
// n + 2 m_e + 2 m_i variables [x | p_e | n_e | p_i | n_i], m_i + 2 m_e + 2 m_i inequality rows, the matrices of
// feasibility_restoration.hpp:434-593 as value arrays over static patterns.  Only built when a solve with user
// callbacks enters restoration; the solver itself never forms these.
struct RestorationView {
  NlpStructure st;
  std::vector<double> V;
};
void build_restoration_view(const NlpStructure& o, RestorationView& v) {
  NlpStructure& t = v.st;
  const int n = o.n, m_e = o.m_e, m_i = o.m_i, M = 2 * m_e + 2 * m_i;
  t.n = n + M;
  t.m_e = m_e;
  t.m_i = m_i + M;
  auto cols = [&](CscPattern& p, int rows) {
    p.rows = rows;
    p.cols = t.n;
    p.colptr.assign(1, 0);
    p.rowidx.clear();
  };
  auto close = [](CscPattern& p) { p.colptr.push_back(static_cast<int32_t>(p.rowidx.size())); };
  cols(t.g_pat, 1);
  for (int c = 0; c < t.n; ++c) {
    t.g_pat.rowidx.push_back(0);
    close(t.g_pat);
  }
  cols(t.Ae, m_e);
  cols(t.Ai, t.m_i);
  cols(t.Hf, t.n);
  cols(t.Hc, t.n);
  for (int c = 0; c < n; ++c) {
    for (int q = o.Ae.colptr[c]; q < o.Ae.colptr[c + 1]; ++q) t.Ae.rowidx.push_back(o.Ae.rowidx[q]);
    for (int q = o.Ai.colptr[c]; q < o.Ai.colptr[c + 1]; ++q) t.Ai.rowidx.push_back(o.Ai.rowidx[q]);
    t.Hf.rowidx.push_back(c);
    for (int q = o.Hc.colptr[c]; q < o.Hc.colptr[c + 1]; ++q) t.Hc.rowidx.push_back(o.Hc.rowidx[q]);
    close(t.Ae), close(t.Ai), close(t.Hf), close(t.Hc);
  }
  for (int e = 0; e < M; ++e) {  // columns of p_e, n_e, p_i, n_i (:499-573)
    if (e < 2 * m_e) t.Ae.rowidx.push_back(e % m_e);
    if (e >= 2 * m_e) t.Ai.rowidx.push_back((e - 2 * m_e) % m_i);
    t.Ai.rowidx.push_back(m_i + e);
    close(t.Ae), close(t.Ai), close(t.Hf), close(t.Hc);
  }
  t.off_f = 0;
  t.off_ce = 1;
  t.off_ci = t.off_ce + t.m_e;
  t.off_g = t.off_ci + t.m_i;
  t.off_Ae = t.off_g + t.g_pat.nnz();
  t.off_Ai = t.off_Ae + t.Ae.nnz();
  t.off_Hf = t.off_Ai + t.Ai.nnz();
  t.off_Hc = t.off_Hf + t.Hf.nnz();
  t.nV = t.off_Hc + t.Hc.nnz();
}
void fill_restoration_view(const NlpStructure& o, RestorationView& v, const Vec& Vo, const Vec& x_ext, const Vec& x_r, const Vec& w,
                           double rho) {
  const NlpStructure& t = v.st;
  const int n = o.n, m_e = o.m_e, m_i = o.m_i, M = 2 * m_e + 2 * m_i;
  Vec& V = v.V;
  V.assign(t.nV, 0.0);
  const double* pn = x_ext.data() + n;
  double f = 0.0;
  for (int e = 0; e < M; ++e) f += rho * pn[e];
  for (int k = 0; k < n; ++k) f += 0.5 * w[k] * (x_ext[k] - x_r[k]) * (x_ext[k] - x_r[k]);
  V[t.off_f] = f;
  for (int j = 0; j < m_e; ++j) V[t.off_ce + j] = Vo[o.off_ce + j] - pn[j] + pn[m_e + j];
  for (int r = 0; r < m_i; ++r) V[t.off_ci + r] = Vo[o.off_ci + r] - pn[2 * m_e + r] + pn[2 * m_e + m_i + r];
  for (int e = 0; e < M; ++e) V[t.off_ci + m_i + e] = pn[e];
  for (int k = 0; k < n; ++k) V[t.off_g + k] = w[k] * (x_ext[k] - x_r[k]);
  for (int e = 0; e < M; ++e) V[t.off_g + n + e] = rho;
  int qe = t.off_Ae, qi = t.off_Ai, qh = t.off_Hc;
  for (int c = 0; c < n; ++c) {
    for (int q = o.Ae.colptr[c]; q < o.Ae.colptr[c + 1]; ++q) V[qe++] = Vo[o.off_Ae + q];
    for (int q = o.Ai.colptr[c]; q < o.Ai.colptr[c + 1]; ++q) V[qi++] = Vo[o.off_Ai + q];
    V[t.off_Hf + c] = w[c];
    for (int q = o.Hc.colptr[c]; q < o.Hc.colptr[c + 1]; ++q) V[qh++] = Vo[o.off_Hc + q];
  }
  for (int e = 0; e < M; ++e) {
    const bool minus = e < m_e || (e >= 2 * m_e && e < 2 * m_e + m_i);  // p_e, p_i enter their constraint with -1
    if (e < 2 * m_e) V[qe++] = minus ? -1.0 : 1.0;
    else V[qi++] = minus ? -1.0 : 1.0;
    V[qi++] = 1.0;
  }
}

// kkt_error.hpp:92-146 (1-norm variant) of the restoration problem, on the host: the rare fallback of the line search
// (interior_point.hpp:691-716).  Vo = the OUTER problem's V at x; X = [x | p_e | n_e | p_i | n_i], S, Z = the five
// inequality blocks.
double restoration_kkt_error_one_norm(const NlpStructure& o, const Vec& Vo, const Vec& X, const Vec& S, const Vec& y, const Vec& Z,
                                      const Vec& x_r, const Vec& w, double rho, double mu) {
  const int n = o.n, m_e = o.m_e, m_i = o.m_i, M = 2 * m_e + 2 * m_i;
  const double* pn = X.data() + n;
  Vec dual(n + M, 0.0);
  for (int k = 0; k < n; ++k) dual[k] = w[k] * (X[k] - x_r[k]);
  for (int c = 0; c < n; ++c) {
    for (int q = o.Ae.colptr[c]; q < o.Ae.colptr[c + 1]; ++q) dual[c] -= Vo[o.off_Ae + q] * y[o.Ae.rowidx[q]];
    for (int q = o.Ai.colptr[c]; q < o.Ai.colptr[c + 1]; ++q) dual[c] -= Vo[o.off_Ai + q] * Z[o.Ai.rowidx[q]];
  }
  for (int j = 0; j < m_e; ++j) {
    dual[n + j] = rho + y[j] - Z[m_i + j];
    dual[n + m_e + j] = rho - y[j] - Z[m_i + m_e + j];
  }
  for (int r = 0; r < m_i; ++r) {
    dual[n + 2 * m_e + r] = rho + Z[r] - Z[m_i + 2 * m_e + r];
    dual[n + 2 * m_e + m_i + r] = rho - Z[r] - Z[m_i + 2 * m_e + m_i + r];
  }
  double err = norm_1(dual.data(), n + M);
  for (int j = 0; j < m_e; ++j) err += std::abs(Vo[o.off_ce + j] - pn[j] + pn[m_e + j]);
  for (int r = 0; r < m_i; ++r) {
    const double c = Vo[o.off_ci + r] - pn[2 * m_e + r] + pn[2 * m_e + m_i + r];
    err += std::abs(S[r] * Z[r] - mu) + std::abs(c - S[r]);
  }
  for (int e = 0; e < M; ++e) err += std::abs(S[m_i + e] * Z[m_i + e] - mu) + std::abs(pn[e] - S[m_i + e]);
  return err;
}

// interior_point.hpp:129-878 on the restoration problem (in_feasibility_restoration = true), the counterpart of
// ipm_core_resident for it: the iterate stays on the device — x, s_0, y, z_0 in the outer system's buffers, p, n and
// their slacks and duals in the FrDevice —, every Newton step is a factorization of the reduced system on the outer
// system's plan (NewtonSystem::compute_hooked), and the host decides on a few dozen scalars.  `accept_exit` is the
// callback the reference appends (interior_point.hpp:729-752): the outer filter's verdict on the restoration iterate,
// from the outer problem's quantities the error launch reduces along.
ExitStatus restoration_core(NewtonSystem& sys, FrDevice& fr, const std::vector<IterationCallback>& user_callbacks,
                            const std::function<bool(const FrErrOut&)>& accept_exit, const Options& options, const Vec& x_r, const Vec& w,
                            Vec& X, Vec& S, Vec& y, Vec& Z, double& mu, int& iterations, SolveReport& rep, clk::time_point solve_start) {
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n, m_e = st.m_e, m_i = st.m_i, M = 2 * m_e + 2 * m_i, mi_ext = m_i + M;
  constexpr double rho = 1e3;
  const FrHost& H = fr.host();

  sys.reset_regularization();
  sys.set_gamma_min(0.0);  // :350-352

  bool host_current = true;
  auto pull_state = [&] {
    if (host_current) return;
    dev.download(dev.d_x(), X.data(), n);
    if (m_i) {
      dev.download(dev.d_s(), S.data(), m_i);
      dev.download(dev.d_z(), Z.data(), m_i);
    }
    if (m_e) dev.download(dev.d_y(), y.data(), m_e);
    fr.download_state(X.data() + n, S.data() + m_i, Z.data() + m_i);
    host_current = true;
  };
  auto finish = [&](ExitStatus st_) {
    pull_state();
    dev.state_changed_by_caller();
    return st_;
  };

  auto t_setup = clk::now();
  dev.sweep_full();  // :245-251: the outer tape at (x, y, z_0) is the restoration problem's c_e, c_i, A_e, A_i, H_c
  fr.errors(/*check_all_V=*/true, mu);
  fr.wait_published();
  FrErrOut cur = H.err;
  if (cur.e.finite == 0.0) return finish(ExitStatus::NONFINITE_INITIAL_GUESS);  // :283-286

  const double mu_min = barrier_floor(1.0, options.tolerance);  // (the restoration cost is not scaled)
  double tau = kTauMin;
  Filter filter{cur.e.viol};  // :303
  int full_step_rejected_counter = 0;
  LineSearch ls;
  // (the error measures: m_i + M inequality rows; the scaling {1, d_ce, [d_ci, 1...]} is never the identity here)
  double E_0 = ipm_E_0(cur.e, m_e, mi_ext, /*identity_scaling=*/false);  // :361-362
  rep.t_setup += since(t_setup);

  RestorationView view;
  Vec Vo;
  bool previous_took_first_attempt = true;  // ... of the regularization policy

  while (E_0 > options.tolerance) {
    if (const ExitStatus exit = infeasible_or_diverging(cur.e, m_e, mi_ext); exit != ExitStatus::SUCCESS) return finish(exit);  // :387-408

    if (!user_callbacks.empty()) {
      pull_state();
      Vo.resize(st.nV);
      dev.download_V(Vo.data());
      if (view.st.n == 0) build_restoration_view(st, view);
      fill_restoration_view(st, view, Vo, X, x_r, w, rho);
      for (const auto& cb : user_callbacks)
        if (cb({iterations, X, S, y, Z, view.V, &view.st, true})) return finish(ExitStatus::CALLBACK_REQUESTED_STOP);
    }
    if (accept_exit(cur)) return finish(ExitStatus::CALLBACK_REQUESTED_STOP);

    // ---- Newton step (:426-482) on the reduced system, then speculatively: the full direction, its step sizes, the
    // first trial point and its filter entry ----
    auto t0 = clk::now();
    // Two attempts of the regularization policy per launch (NewtonSystem::compute_hooked): the one it is at and the one
    // it would make next — a restoration phase rejects its unregularized attempt iteration after iteration (H_c with the
    // restoration's own multipliers is indefinite), and climbs the ladder from delta = 1e-4 (:95-98, :127-130) every few
    // iterations: each rejected attempt used to be a launch and a round trip of its own.  The chain behind a launch —
    // the look-ahead iteration, as in ipm_core_resident: the whole iterate the full step would give, the full tape at it,
    // its error norms — follows the FIRST attempt, and only where the previous iteration took its first attempt; a
    // direction taken from a second attempt gets its chain when the policy has settled.
    NewtonSystem::AttemptHooks hooks;
    auto chain = [&](double d) {
      fr.expand(d, mu, tau, /*soc=*/false, /*ahead=*/true);
      dev.sweep_full_lookahead(/*with_reduce=*/false, /*skippable=*/false);  // (the separable sums ride in the error launch)
      fr.errors(false, mu, /*ahead=*/true, /*sums_ride=*/true);
    };
    hooks.prepare = [&](double d, double) { fr.build(d, mu, /*soc=*/false, /*rhs_only=*/false); };
    hooks.prepare_second = [&](double d, double, const double** lhs2, const double** rhs2) {
      fr.build(d, mu, /*soc=*/false, /*rhs_only=*/false, /*second=*/true);
      *lhs2 = fr.second_lhs();
      *rhs2 = fr.second_rhs();
    };
    hooks.prepare_pair = [&](double d0, double, double d1, double, const double** lhs2, const double** rhs2) {
      fr.build_pair(d0, d1, mu);
      *lhs2 = fr.second_lhs();
      *rhs2 = fr.second_rhs();
    };
    if (previous_took_first_attempt) hooks.after = [&](double d, double) { chain(d); };
    // (the eliminated rows' pivots without regularization: reduced with this iterate's error norms)
    hooks.eliminated_min_pivot = [&] { return cur.eliminated_min_pivot; };
    auto info = sys.compute_hooked(hooks);
    previous_took_first_attempt = sys.last_factorizations() == 1;
    if (info[0] == FactorInfo::Success && !sys.last_hooked_chain_valid()) chain(sys.hessian_regularization()[0]);
    if (info[0] == FactorInfo::Success) fr.wait_published();
    rep.factorizations += sys.last_factorizations();
    rep.solves += sys.last_factorizations();
    rep.value_sweeps += sys.last_factorizations();
    rep.t_kkt_decomp += since(t0);
    if (info[0] != FactorInfo::Success) return finish(ExitStatus::FACTORIZATION_FAILED);  // :463-465
    const double delta = sys.hessian_regularization()[0];
    rep.delta = delta;
    rep.gamma = sys.constraint_jacobian_regularization()[0];

    t0 = clk::now();
    const FilterEntry current_entry{cur.e.f - mu * cur.e.logsum, cur.e.viol};
    ls.start(filter, full_step_rejected_counter, mu, current_entry, H.dir.alpha_max, H.dir.alpha_z, H.dir.D_phi);  // :488-509
    static const bool fr_debug = std::getenv("SLPX_FR_DEBUG") != nullptr;
    if (fr_debug) {
      std::fprintf(stderr, "fr: it %d mu %.3e delta %.1e gamma %.1e nfact %d | alpha_max %.3e alpha_z %.3e D_phi %.3e emin %.3e | cur f %.6e viol %.6e logsum %.6e | trial f %.6e viol %.6e logsum %.6e fin %g\n",
                   iterations, mu, delta, rep.gamma, sys.last_factorizations(), ls.alpha_max, ls.alpha_z, H.dir.D_phi, H.dir.eliminated_min_pivot, cur.e.f, cur.e.viol,
                   cur.e.logsum, H.err_ahead.e.f, H.err_ahead.e.viol, H.err_ahead.e.logsum, H.err_ahead.e.finite);
    }
    bool have_trial = true;       // the chain behind the step evaluated alpha_max, as the complete look-ahead iterate
    bool took_lookahead = false;  // ... and the filter took it

    // (a step below the floor fails this phase at once: there is no restoration to call from here)
    while (!ls.call_feasibility_restoration && ls.want != Want::Done) switch (ls.want) {
      case Want::Eval: {
        const bool from_ahead = have_trial;
        if (!have_trial) {
          fr.trial_point(ls.t_alpha);
          dev.sweep_values_trial();
          fr.trial_metrics(ls.t_alpha, mu);
          fr.wait_published();
          ++rep.value_sweeps;
        }
        have_trial = false;
        ls.on_trial(from_ahead ? IpmTrialOut{H.err_ahead.e.f, H.err_ahead.e.viol, H.err_ahead.e.logsum, H.err_ahead.e.finite} : H.trial);
        took_lookahead = from_ahead && ls.end == End::Newton;
        break;
      }
      case Want::SocSolve:  // :601-633: new right-hand side, SAME factorization
        if (ls.soc_first) fr.save_direction();
        fr.soc_accumulate(ls.alpha_soc, ls.soc_first);
        fr.build(delta, mu, /*soc=*/true, /*rhs_only=*/true);
        dev.solve();
        ++rep.solves;
        fr.expand(delta, mu, tau, /*soc=*/true);
        dev.sweep_values_trial();
        fr.trial_metrics(-1.0, mu);
        fr.wait_published();
        ++rep.value_sweeps;
        ls.on_soc_solve(H.dir.alpha_max, H.dir.alpha_z);
        ls.on_trial(H.trial);  // (SocEval: the chain above evaluated the corrected trial point already)
        if (!ls.on_correction) fr.restore_direction();  // the corrections failed: back to the Newton direction
        break;
      case Want::KktEval: {  // :691-716 — rare: on the host, with the iterate pulled over
        const double alpha_max = ls.t_alpha, alpha_z = ls.t_alpha_z;
        host_current = false;
        pull_state();
        Vo.resize(st.nV);
        dev.download_V(Vo.data());
        const double current_kkt = restoration_kkt_error_one_norm(st, Vo, X, S, y, Z, x_r, w, rho, mu);
        Vec p_x, p_y, ps0, pz0, dpn(M), psx(M), pzx(M);
        download_direction(dev, n, m_e, m_i, p_x, p_y, ps0, pz0);
        fr.download_direction(dpn.data(), psx.data(), pzx.data());
        Vec Xt(X), St(S), yt(y), Zt(Z);
        for (int k = 0; k < n; ++k) Xt[k] += alpha_max * p_x[k];
        for (int e = 0; e < M; ++e) {
          Xt[n + e] += alpha_max * dpn[e];
          St[m_i + e] += alpha_max * psx[e];
          Zt[m_i + e] += alpha_z * pzx[e];
        }
        for (int r = 0; r < m_i; ++r) {
          St[r] += alpha_max * ps0[r];
          Zt[r] += alpha_z * pz0[r];
        }
        for (int j = 0; j < m_e; ++j) yt[j] += alpha_z * p_y[j];
        // A_e, A_i at the trial point: a full sweep there, then the iterate back in place
        dev.upload_x(Xt.data());
        dev.upload_duals(St.data(), yt.data(), Zt.data());
        dev.sweep_full();
        Vec Vt(st.nV);
        dev.download_V(Vt.data());
        dev.upload_x(X.data());
        dev.upload_duals(S.data(), y.data(), Z.data());
        dev.sweep_full();
        ls.on_kkt_errors(current_kkt, restoration_kkt_error_one_norm(st, Vt, Xt, St, yt, Zt, x_r, w, rho, mu));
        break;
      }
      default: break;
    }
    const double alpha = ls.alpha, alpha_z = ls.alpha_z;
    rep.t_line_search += since(t0);
    if (ls.call_feasibility_restoration) return finish(ExitStatus::FEASIBILITY_RESTORATION_FAILED);  // :721-723

    t0 = clk::now();
    host_current = false;
    if (took_lookahead) {
      fr.accept_lookahead();  // :775-801 happened in the look-ahead launch; the buffers change roles
      cur = H.err_ahead;      // :809-812 and the norms: already there
    } else {
      fr.commit(ls.end == End::Fallback ? ls.alpha_max : alpha, alpha_z, mu);  // :775-801
      // AD refresh (:809-812) and every norm the next decisions need
      dev.sweep_full();
      fr.errors(false, mu);
      fr.wait_published();
      cur = H.err;
    }
    rep.t_ad_refresh += since(t0);

    E_0 = ipm_E_0(cur.e, m_e, mi_ext, /*identity_scaling=*/false);
    if (E_0 > options.tolerance)  // :819-832
      update_barrier_parameter(mu, mu_min, tau, filter, [&](double m) { return ipm_E_mu(cur.e, m, m_e, mi_ext); });
    if (options.diagnostics)
      print_iteration(iterations, E_0, cur.e.f, cur.e.viol, mu, rep, alpha, alpha_z, sys.last_factorizations(), "  (restoration)");
    ++iterations;
    if (iterations >= options.max_iterations) return finish(ExitStatus::MAX_ITERATIONS_EXCEEDED);
    if (since(solve_start) > options.timeout) return finish(ExitStatus::TIMEOUT);
  }
  return finish(ExitStatus::SUCCESS);
}

}  // namespace

// feasibility_restoration.hpp:347-628 (interior-point variant).  g = the outer problem's dense gradient at x.
ExitStatus feasibility_restoration(NewtonSystem& outer, const Vec& scales, const std::vector<IterationCallback>& user_callbacks,
                                   const std::function<bool(const FilterEntry&, double)>& outer_accepts, const Options& options,
                                   Vec& x, Vec& s, Vec& y, Vec& z, double mu, int& iterations, SolveReport& rep,
                                   clk::time_point solve_start, const Vec& c_e, const Vec& c_i, const Vec& g, double initial_violation) {
  const NlpStructure& ost = outer.structure();
  const int n = ost.n, m_i = ost.m_i;
  ++rep.restorations;

  RestorationEntry entry = restoration_entry(ost, scales, x, s, mu, c_e, c_i);
  const double fr_mu = entry.fr_mu;

  DeviceNlp& dev = outer.device();
  const auto t_build = clk::now();
  dev.ipm_enable();  // (the trial buffers)
  FrDevice& fr = outer.restoration_device();
  rep.t_restoration_setup += since(t_build);

  Vec &X = entry.X, &S = entry.S, &fr_y = entry.y, &Z = entry.Z;
  const Vec &x_r = entry.x_r, &w = entry.w, &fr_scales = entry.fr_scales;

  const Vec s_outer(s);
  fr.begin(x_r.data(), w.data(), g.data(), s_outer.data(), mu, X.data() + n, S.data() + m_i, Z.data() + m_i, fr_scales);
  dev.upload_x(X.data());
  dev.upload_duals(S.data(), fr_y.data(), Z.data());

  // the callback the reference appends (interior_point.hpp:729-752): leave once the OUTER filter accepts the
  // restoration iterate and the violation dropped by 10 %
  auto accept_exit = [&](const FrErrOut& e) {
    const FilterEntry trial_entry{e.f_outer - mu * e.logsum_outer, e.viol_outer};
    return trial_entry.constraint_violation < 0.9 * initial_violation && outer_accepts(trial_entry, e.dphi_outer);
  };

  const auto saved_regularization = outer.regularization_state();
  double mu_fr = fr_mu;
  const int it_before = iterations;
  const auto t_inner = clk::now();
  const double outer_error = rep.final_error;
  const ExitStatus status = restoration_core(outer, fr, user_callbacks, accept_exit, options, x_r, w, X, S, fr_y, Z, mu_fr, iterations,
                                             rep, solve_start);
  outer.set_regularization_state(saved_regularization);
  outer.set_gamma_min(1e-10);
  rep.final_error = outer_error;
  rep.restoration_iterations += iterations - it_before;
  rep.t_restoration += since(t_inner);

  std::copy(X.begin(), X.begin() + n, x.begin());
  std::copy(S.begin(), S.begin() + m_i, s.begin());

  if (status == ExitStatus::CALLBACK_REQUESTED_STOP) {
    // back to the original problem: least-squares multipliers at the new point (:606-617)
    if (!restoration_multiplier_estimate(outer, x, s, y, z, mu, rep)) return ExitStatus::FACTORIZATION_FAILED;
    return ExitStatus::SUCCESS;
  } else if (status == ExitStatus::SUCCESS) {
    return ExitStatus::LOCALLY_INFEASIBLE;
  }
  return ExitStatus::FEASIBILITY_RESTORATION_FAILED;
}

ExitStatus feasibility_restoration_steps(NewtonSystem& sys, const std::vector<double>& scales,
                                         const Options& options, std::vector<double>& x,
                                         std::vector<double>& s, std::vector<double>& y,
                                         std::vector<double>& z, double mu, int steps,
                                         SolveReport* report) {
  const NlpStructure& st = sys.structure();
  SolveReport local;
  SolveReport& rep = report ? *report : local;
  rep = SolveReport{};
  // c_e, c_i at x (the caller of feasibility_restoration holds them, interior_point.hpp:721-727)
  DeviceNlp& dev = sys.device();
  Vec V(st.nV);
  dev.upload_x(x.data());
  dev.upload_duals(s.data(), y.data(), z.data());
  dev.sweep_full();
  dev.download_V(V.data());
  const Vec c_e(V.begin() + st.off_ce, V.begin() + st.off_ce + st.m_e);
  const Vec c_i(V.begin() + st.off_ci, V.begin() + st.off_ci + st.m_i);
  int iterations = 0;
  const std::vector<IterationCallback> stop{
      [steps](const IterationInfo& info) { return info.iteration >= steps; }};
  const Vec g = VView{st, V}.g_dense();
  double violation = norm_1(c_e.data(), st.m_e);
  for (int j = 0; j < st.m_i; ++j) violation += std::abs(c_i[j] - s[j]);
  const auto never = [](const FilterEntry&, double) { return false; };
  return feasibility_restoration(sys, scales, stop, never, options, x, s, y, z, mu, iterations, rep, clk::now(), c_e, c_i, g,
                                 violation);
}

ExitStatus feasibility_restoration_handoff(NewtonSystem& sys, const std::vector<double>& scales,
                                           const std::function<bool(const FilterEntry&, double)>& outer_accepts,
                                           const Options& options, std::vector<double>& x, std::vector<double>& s,
                                           std::vector<double>& y, std::vector<double>& z, double mu, int& iterations,
                                           SolveReport& report, std::chrono::steady_clock::time_point solve_start,
                                           const std::vector<double>& c_e, const std::vector<double>& c_i,
                                           const std::vector<double>& g, double initial_violation) {
  return feasibility_restoration(sys, scales, {}, outer_accepts, options, x, s, y, z, mu, iterations, report, solve_start, c_e,
                                 c_i, g, initial_violation);
}

bool restoration_multiplier_estimate(NewtonSystem& outer, const std::vector<double>& x, const std::vector<double>& s,
                                     std::vector<double>& y, std::vector<double>& z, double mu, SolveReport& rep) {
  DeviceNlp& dev = outer.device();
  Vec V(outer.structure().nV);
  dev.upload_x(x.data());
  dev.upload_duals(s.data(), y.data(), z.data());
  dev.sweep_full();
  dev.download_V(V.data());
  return lagrange_multiplier_estimate(outer, V, s, mu, y, z, rep);
}

double restoration_kkt_error(const NlpStructure& o, const std::vector<double>& Vo, const std::vector<double>& X,
                             const std::vector<double>& S, const std::vector<double>& y, const std::vector<double>& Z,
                             const std::vector<double>& x_r, const std::vector<double>& w, double mu) {
  return restoration_kkt_error_one_norm(o, Vo, X, S, y, Z, x_r, w, /*rho=*/1e3, mu);
}

}  // namespace slpx
