// The reference's other two solvers on the same device Newton step:
// Problem::solve sends problems without constraints to newton() and problems with equality
// constraints only to sqp() (problem.hpp:335, 403).  Both are the interior-point iteration
// with its inequality machinery taken out — but not quite the m_i = 0 special case of it: SQP
// moves y with the primal step size (the IPM would take alpha_z = 1), Newton's line search
// goes down to alpha = 1e-20 and ends in LINE_SEARCH_FAILED instead of a restoration phase.
// Host-resident drivers (one value sweep per trial point crosses PCIe): these are the small
// problems of the reference's unit tests, not the benchmark path.
#include "ipm_drivers.hpp"

#include <algorithm>
#include <cmath>

namespace slpx {

namespace {

using namespace ipm_host;
using Want = LineSearch::Want;

// sqp.hpp:98-604
ExitStatus sqp_core(NewtonSystem& sys, const Vec& scales, const std::vector<IterationCallback>& callbacks,
                    const Options& options, Vec& x, Vec& y, int& iterations, SolveReport& rep,
                    clk::time_point solve_start) {
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n, m_e = st.m_e, dim = n + m_e;
  const Vec none;  // no slacks, no inequality multipliers
  double mu0 = 0.0;

  sys.reset_regularization();
  sys.set_gamma_min(1e-10);  // sparse_regularized_ldlt.hpp:197 (the constructor of sqp.hpp:238-240 passes none)

  Vec V(st.nV), Vtrial(st.nV);
  auto refresh_full = [&](const Vec& xx, const Vec& yy) {
    dev.upload_x(xx.data());
    dev.upload_duals(none.data(), yy.data(), none.data());
    dev.sweep_full();
    dev.download_V(V.data());
  };
  auto eval_values = [&](const Vec& xx) {
    dev.upload_x(xx.data());
    dev.sweep_values();
    dev.download(dev.d_V(), Vtrial.data(), static_cast<size_t>(st.off_g));
    ++rep.value_sweeps;
  };

  auto t_setup = clk::now();
  refresh_full(x, y);  // :182-186
  VView cur{st, V};
  Vec g = cur.g_dense();
  if (m_e > n) return ExitStatus::TOO_FEW_DOFS;                                   // :205-210
  if (!all_finite(V.data(), st.nV)) return ExitStatus::NONFINITE_INITIAL_GUESS;  // :213-216

  double f = cur.f();
  Vec c_e(cur.c_e(), cur.c_e() + m_e);
  Filter filter{norm_1(c_e.data(), m_e)};  // :220
  int full_step_rejected_counter = 0;
  LineSearch ls;
  const bool identity = scaling_is_identity(st, scales);
  auto E0_of = [&](const Vec& gg, const Vec& ce, const Vec& yy) {
    return kkt_error_impl<ErrType::INF_NORM_SCALED>(st, gg, cur.Ae(), ce.data(), nullptr, nullptr, none, yy, none,
                                                    0.0, identity ? nullptr : &scales);
  };
  double E_0 = E0_of(g, c_e, y);  // :253-254
  rep.t_setup = since(t_setup);

  Vec p_x(n), p_y(m_e), trial_x, trial_y, trial_c_e(m_e);
  double trial_f = 0.0;
  // f, c_e at trial_x: the trial point's numbers for the line search (no slacks: no barrier term)
  auto trial_out = [&] {
    eval_values(trial_x);
    trial_f = Vtrial[st.off_f];
    std::copy(Vtrial.begin() + st.off_ce, Vtrial.begin() + st.off_ce + m_e, trial_c_e.begin());
    const bool finite = std::isfinite(trial_f) && all_finite(trial_c_e.data(), m_e);
    return IpmTrialOut{trial_f, norm_1(trial_c_e.data(), m_e), 0.0, finite ? 1.0 : 0.0};
  };
  Vec no_s, no_z;  // (no inequality rows: download_direction leaves them alone)

  while (E_0 > options.tolerance) {
    // :277-292 infeasibility / divergence checks
    if (equality_rows_locally_infeasible(st, cur.Ae(), c_e)) return ExitStatus::LOCALLY_INFEASIBLE;
    if (norm_inf(x.data(), n) > 1e10 || !all_finite(x.data(), n)) return ExitStatus::DIVERGING_ITERATES;
    for (const auto& cb : callbacks)
      if (cb({iterations, x, none, y, none, V, &st, false})) return ExitStatus::CALLBACK_REQUESTED_STOP;

    // ---- Newton-KKT step on the device: [H A_e^T; A_e 0] [p_x; -p_y] = -[g - A_e^T y; c_e] (:305-346) ----
    auto t0 = clk::now();
    dev.upload_x(x.data());
    dev.upload_duals(none.data(), y.data(), none.data());
    dev.upload_mu(&mu0);
    dev.assemble();
    dev.build_rhs();
    rep.t_kkt_build += since(t0);
    t0 = clk::now();
    auto info = sys.compute(/*solve_speculatively=*/true);
    rep.factorizations += sys.last_factorizations();
    rep.t_kkt_decomp += since(t0);
    if (info[0] != FactorInfo::Success) return ExitStatus::FACTORIZATION_FAILED;  // :336-338
    rep.delta = sys.hessian_regularization()[0];
    rep.gamma = sys.constraint_jacobian_regularization()[0];
    t0 = clk::now();
    rep.solves += sys.last_factorizations();
    download_direction(dev, n, m_e, 0, p_x, p_y, no_s, no_z);
    rep.t_kkt_solve += since(t0);

    t0 = clk::now();
    const FilterEntry current_entry{f, norm_1(c_e.data(), m_e)};
    double D_phi = 0.0;  // :360
    for (int i = 0; i < n; ++i) D_phi += g[i] * p_x[i];
    // The interior-point line search with alpha_max = 1 and no barrier term.  y moves with the primal step: this
    // driver reads ls.alpha (ls.t_alpha) alone, and a correction keeps the full step (:435: alpha_soc is never recomputed).
    ls.start(filter, full_step_rejected_counter, 0.0, current_entry, 1.0, 1.0, D_phi);
    Vec soc_px(n), soc_py(m_e), c_e_soc;

    while (ls.want != Want::Done) switch (ls.want) {
      case Want::Eval:  // :364-384
        trial_x = axpy(x, ls.t_alpha, p_x);
        trial_y = axpy(y, ls.t_alpha, p_y);
        ls.on_trial(trial_out());
        break;
      case Want::SocSolve: {  // :397-468: new bottom rows of the rhs, SAME factorization
        if (ls.soc_first) c_e_soc = c_e;
        for (int j = 0; j < m_e; ++j) c_e_soc[j] = ls.alpha_soc * c_e_soc[j] + trial_c_e[j];  // :435
        Vec rhs(dim, 0.0);
        for (int i = 0; i < n; ++i) rhs[i] = -g[i];
        add_At_v(st.Ae, cur.Ae(), nullptr, y.data(), 1.0, rhs);
        for (int j = 0; j < m_e; ++j) rhs[n + j] = -c_e_soc[j];
        SLPX_HIP_CHECK(hipMemcpyAsync(dev.d_rhs(), rhs.data(), dim * sizeof(double), hipMemcpyHostToDevice,
                                      dev.stream()));
        dev.solve();
        ++rep.solves;
        download_direction(dev, n, m_e, 0, soc_px, soc_py, no_s, no_z);
        ls.on_soc_solve(ls.alpha_max, ls.alpha_max);
        break;
      }
      case Want::SocEval:
        trial_x = axpy(x, ls.t_alpha, soc_px);
        trial_y = axpy(y, ls.t_alpha, soc_py);
        ls.on_trial(trial_out());
        break;
      case Want::KktEval: {  // :492-517
        const double current_kkt = kkt_error_impl<ErrType::ONE_NORM>(st, g, cur.Ae(), c_e.data(), nullptr, nullptr, none,
                                                                     y, none, 0.0, nullptr);
        trial_x = axpy(x, ls.t_alpha, p_x);
        trial_y = axpy(y, ls.t_alpha, p_y);
        Vec Vt(st.nV);
        dev.upload_x(trial_x.data());
        dev.upload_duals(none.data(), trial_y.data(), none.data());
        dev.sweep_full();
        dev.download_V(Vt.data());
        VView tv{st, Vt};
        ls.on_kkt_errors(current_kkt, kkt_error_impl<ErrType::ONE_NORM>(st, tv.g_dense(), tv.Ae(), tv.c_e(), nullptr, nullptr,
                                                                        none, trial_y, none, 0.0, nullptr));
        break;
      }
      case Want::Done: break;
    }
    const double alpha = ls.alpha;
    rep.t_line_search += since(t0);

    if (ls.call_feasibility_restoration) {  // :521-556
      refresh_full(x, y);  // the device V describes x again (the fallback above moved it)
      const double f_x = cur.f();
      const FilterEntry initial_entry{f_x, norm_1(c_e.data(), m_e)};
      const Vec g_here = cur.g_dense();
      auto outer_accepts = [&, alpha](const FilterEntry& trial_entry, double D_phi_restoration) {
        return filter.try_add(initial_entry, trial_entry, D_phi_restoration, alpha);
      };
      // feasibility_restoration.hpp:103-345: the interior-point variant with no inequality rows
      // of the original problem and mu = tolerance / 10
      Vec s_none, z_none;
      const ExitStatus fr_status = feasibility_restoration(sys, scales, callbacks, outer_accepts, options, x, s_none, y, z_none,
                                                           options.tolerance / 10.0, iterations, rep, solve_start, c_e, Vec{}, g_here,
                                                           initial_entry.constraint_violation);
      if (fr_status != ExitStatus::SUCCESS) return fr_status;
      sys.set_gamma_min(1e-10);
    } else {
      x = trial_x;
      y = trial_y;
    }
    auto t1 = clk::now();
    refresh_full(x, y);  // :574-577
    rep.t_ad_refresh += since(t1);
    g = cur.g_dense();
    f = cur.f();
    std::copy(cur.c_e(), cur.c_e() + m_e, c_e.begin());
    E_0 = E0_of(g, c_e, y);
    rep.final_error = E_0;
    if (options.diagnostics)
      print_iteration(iterations, E_0, f, norm_1(c_e.data(), m_e), 0.0, rep, alpha, alpha, sys.last_factorizations(), "  (sqp)");
    ++iterations;
    if (iterations >= options.max_iterations) return ExitStatus::MAX_ITERATIONS_EXCEEDED;
    if (since(solve_start) > options.timeout) return ExitStatus::TIMEOUT;
  }
  return ExitStatus::SUCCESS;
}

// newton.hpp:51-292
ExitStatus newton_core(NewtonSystem& sys, const Vec& scales, const std::vector<IterationCallback>& callbacks,
                       const Options& options, Vec& x, int& iterations, SolveReport& rep,
                       clk::time_point solve_start) {
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n;
  const Vec none;
  double mu0 = 0.0;
  sys.reset_regularization();
  sys.set_gamma_min(1e-10);  // no equality rows: unused

  Vec V(st.nV), Vtrial(st.nV);
  auto refresh_full = [&](const Vec& xx) {
    dev.upload_x(xx.data());
    dev.sweep_full();
    dev.download_V(V.data());
  };
  auto eval_f = [&](const Vec& xx) {
    dev.upload_x(xx.data());
    dev.sweep_values();
    dev.download(dev.d_V(), Vtrial.data(), static_cast<size_t>(st.off_g));
    ++rep.value_sweeps;
    return Vtrial[st.off_f];
  };
  refresh_full(x);
  VView cur{st, V};
  Vec g = cur.g_dense();
  if (!all_finite(V.data(), st.nV)) return ExitStatus::NONFINITE_INITIAL_GUESS;  // :125-127
  Filter filter{0.0};  // :131
  NewtonSearch search;   // (a search of its own, newton.hpp:201-243: no corrections, no restoration, a floor of 1e-20)
  search.f = cur.f();
  const bool identity = scaling_is_identity(st, scales);
  auto E0_of = [&](const Vec& gg) {
    return kkt_error_impl<ErrType::INF_NORM_SCALED>(st, gg, nullptr, nullptr, nullptr, nullptr, none, none, none, 0.0,
                                                    identity ? nullptr : &scales);
  };
  double E_0 = E0_of(g);
  Vec p_x(n), trial_x;
  while (E_0 > options.tolerance) {
    if (norm_inf(x.data(), n) > 1e10 || !all_finite(x.data(), n)) return ExitStatus::DIVERGING_ITERATES;  // :164
    for (const auto& cb : callbacks)
      if (cb({iterations, x, none, none, none, V, &st, false})) return ExitStatus::CALLBACK_REQUESTED_STOP;
    // H p_x = -g (:182-190)
    auto t0 = clk::now();
    dev.upload_x(x.data());
    dev.upload_mu(&mu0);
    dev.assemble();
    dev.build_rhs();
    auto info = sys.compute(/*solve_speculatively=*/true);
    rep.factorizations += sys.last_factorizations();
    rep.solves += sys.last_factorizations();
    rep.t_kkt_decomp += since(t0);
    if (info[0] != FactorInfo::Success) return ExitStatus::FACTORIZATION_FAILED;
    rep.delta = sys.hessian_regularization()[0];
    dev.download(dev.ldlt().d_p(), p_x.data(), n);

    t0 = clk::now();
    double D_phi = 0.0;
    for (int i = 0; i < n; ++i) D_phi += g[i] * p_x[i];
    search.start(filter, D_phi);
    while (search.want != NewtonSearch::Want::Done) {
      if (search.want == NewtonSearch::Want::Eval) {
        trial_x = axpy(x, search.t_alpha, p_x);
        const double trial_f = eval_f(trial_x);
        search.on_trial(trial_f, std::isfinite(trial_f));
        continue;
      }
      const double current_kkt = norm_1(g.data(), n);  // KktEval
      trial_x = axpy(x, NewtonSearch::alpha_max, p_x);
      Vec Vt(st.nV);
      dev.upload_x(trial_x.data());
      dev.sweep_full();
      dev.download_V(Vt.data());
      VView tv{st, Vt};
      const Vec tg = tv.g_dense();
      search.on_kkt_errors(current_kkt, norm_1(tg.data(), n), tv.f());
    }
    if (search.failed) return ExitStatus::LINE_SEARCH_FAILED;
    rep.t_line_search += since(t0);
    x = trial_x;
    refresh_full(x);  // :254-255
    g = cur.g_dense();
    E_0 = E0_of(g);
    rep.final_error = E_0;
    if (options.diagnostics)
      print_iteration(iterations, E_0, search.f, 0.0, 0.0, rep, search.alpha, search.alpha, sys.last_factorizations(), "  (newton)");
    ++iterations;
    if (iterations >= options.max_iterations) return ExitStatus::MAX_ITERATIONS_EXCEEDED;
    if (since(solve_start) > options.timeout) return ExitStatus::TIMEOUT;
  }
  return ExitStatus::SUCCESS;
}

}  // namespace

ExitStatus sqp(NewtonSystem& sys, const std::vector<double>& scales, const std::vector<IterationCallback>& callbacks,
               const Options& options, std::vector<double>& x, std::vector<double>* y_out, SolveReport* report) {
  return sqp(sys, scales, callbacks, options, x, y_out, report, nullptr);
}

ExitStatus sqp(NewtonSystem& sys, const std::vector<double>& scales, const std::vector<IterationCallback>& callbacks,
               const Options& options, std::vector<double>& x, std::vector<double>* y_out, SolveReport* report,
               const WarmStart* warm) {
  const auto solve_start = clk::now();
  SolveReport local;
  SolveReport& rep = report ? *report : local;
  rep = SolveReport{};
  const int m_e = sys.structure().m_e;
  Vec y(m_e, 0.0);  // problem.hpp:503-504
  if (warm) {
    check_warm_length(warm->y, m_e, "y");
    if (any_bad(x) || any_bad(warm->y)) {
      if (y_out) *y_out = y;
      return ExitStatus::NONFINITE_INITIAL_GUESS;
    }
    if (!warm->y.empty())
      for (int j = 0; j < m_e; ++j) y[j] = warm_scale_dual(warm->y[j], scales[1 + j], scales[0]);
  }
  int iterations = 0;
  const ExitStatus status = sqp_core(sys, scales, callbacks, options, x, y, iterations, rep, solve_start);
  if (y_out) *y_out = y;
  rep.iterations = iterations;
  rep.t_total = since(solve_start);
  return status;
}

ExitStatus newton(NewtonSystem& sys, const std::vector<double>& scales, const std::vector<IterationCallback>& callbacks,
                  const Options& options, std::vector<double>& x, SolveReport* report) {
  const auto solve_start = clk::now();
  SolveReport local;
  SolveReport& rep = report ? *report : local;
  rep = SolveReport{};
  int iterations = 0;
  const ExitStatus status = newton_core(sys, scales, callbacks, options, x, iterations, rep, solve_start);
  rep.iterations = iterations;
  rep.t_total = since(solve_start);
  return status;
}

}  // namespace slpx
