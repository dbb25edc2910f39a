// The interior-point solver's entry: the problem scaling, the driver that keeps the vectors on the host, the choice
// between it and the device-resident one (ipm_resident.cpp), and interior_point() with its warm start.  (Feasibility
// restoration: ipm_restoration.cpp; the SQP and Newton solvers: sqp_newton.cpp.)
#include "ipm_drivers.hpp"

#include "ipm_formulas.h"

#include <algorithm>
#include <cmath>

namespace slpx {

namespace {

using namespace ipm_host;
using Want = LineSearch::Want;

}  // namespace

std::vector<double> compute_problem_scaling(const NlpStructure& s, const std::vector<double>& V) {
  constexpr double g_max = 100.0;
  std::vector<double> scales(s.n_scales(), 1.0);
  double gn = 0.0;
  for (int p = 0; p < s.g_pat.nnz(); ++p) gn = std::max(gn, std::abs(V[s.off_g + p]));
  scales[0] = std::min(1.0, g_max / gn);
  std::vector<double> rn(s.m_e, 0.0);
  for (int p = 0; p < s.Ae.nnz(); ++p) rn[s.Ae.rowidx[p]] = std::max(rn[s.Ae.rowidx[p]], std::abs(V[s.off_Ae + p]));
  for (int j = 0; j < s.m_e; ++j) scales[1 + j] = std::min(g_max / rn[j], 1.0);
  rn.assign(s.m_i, 0.0);
  for (int p = 0; p < s.Ai.nnz(); ++p) rn[s.Ai.rowidx[p]] = std::max(rn[s.Ai.rowidx[p]], std::abs(V[s.off_Ai + p]));
  for (int j = 0; j < s.m_i; ++j) scales[1 + s.m_e + j] = std::min(g_max / rn[j], 1.0);
  return scales;
}

// interior_point.hpp:129-878: the iteration proper, on caller-owned iterates (the
// restoration phase re-enters it with in_feasibility_restoration = true).
ExitStatus ipm_core_host(NewtonSystem& sys, const Vec& scales,
                         const std::vector<IterationCallback>& callbacks, const Options& options,
                         bool in_feasibility_restoration, Vec& x, Vec& s, Vec& y, Vec& z, double& mu,
                         int& iterations, SolveReport& rep, clk::time_point solve_start) {
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n, m_e = st.m_e, m_i = st.m_i, dim = n + m_e;

  sys.reset_regularization();
  sys.set_gamma_min(in_feasibility_restoration ? 0.0 : 1e-10);  // :350-352

  Vec V(st.nV), Vtrial(st.nV);
  auto refresh_full = [&](const Vec& xx, const Vec& yy, const Vec& zz) {
    dev.upload_x(xx.data());
    dev.upload_duals(s.data(), yy.data(), zz.data());
    dev.sweep_full();
    dev.download_V(V.data());
  };
  // forward-only sweep at a trial point; fills the f, c_e, c_i head of Vtrial
  auto eval_values = [&](const Vec& xx) {
    dev.upload_x(xx.data());
    dev.sweep_values();
    dev.download(dev.d_V(), Vtrial.data(), static_cast<size_t>(st.off_g));
    ++rep.value_sweeps;
  };

  auto t_setup = clk::now();
  refresh_full(x, y, z);  // :245-251
  VView cur{st, V};
  Vec g = cur.g_dense();

  if (m_e > n) return ExitStatus::TOO_FEW_DOFS;  // :274
  if (!all_finite(V.data(), st.nV)) return ExitStatus::NONFINITE_INITIAL_GUESS;  // :283-286

  const double mu_min = barrier_floor(scales[0], options.tolerance);
  double tau = kTauMin;

  double f = cur.f();
  Vec c_e(cur.c_e(), cur.c_e() + m_e), c_i(cur.c_i(), cur.c_i() + m_i);

  auto violation = [&](const Vec& ce, const Vec& ci, const Vec& ss) {
    double v = norm_1(ce.data(), m_e);
    for (int j = 0; j < m_i; ++j) v += std::abs(ci[j] - ss[j]);
    return v;
  };
  Filter filter{violation(c_e, c_i, s)};  // :303
  int full_step_rejected_counter = 0;
  LineSearch ls;
  const bool identity = scaling_is_identity(st, scales);
  auto E0_of = [&](const Vec& gg, const Vec& ce, const Vec& ci, const Vec& ss, const Vec& yy,
                   const Vec& zz) {
    return kkt_error_impl<ErrType::INF_NORM_SCALED>(st, gg, cur.Ae(), ce.data(), cur.Ai(),
                                                    ci.data(), ss, yy, zz, 0.0,
                                                    identity ? nullptr : &scales);
  };
  double E_0 = E0_of(g, c_e, c_i, s, y, z);  // :361-362
  rep.t_setup = since(t_setup);

  Vec p(dim), p_x(n), p_y(m_e), p_s(m_i), p_z(m_i);
  Vec trial_x, trial_s, trial_y, trial_z, trial_c_e(m_e), trial_c_i(m_i);
  double trial_f = 0.0;

  while (E_0 > options.tolerance) {
    // :387-408 infeasibility / divergence checks
    if (equality_rows_locally_infeasible(st, cur.Ae(), c_e)) return ExitStatus::LOCALLY_INFEASIBLE;
    if (m_i > 0) {
      Vec cplus(m_i), t(n, 0.0);
      for (int j = 0; j < m_i; ++j) cplus[j] = std::min(c_i[j], 0.0);
      add_At_v(st.Ai, cur.Ai(), nullptr, cplus.data(), 1.0, t);
      double nt = 0.0, nc = 0.0;
      for (double v : t) nt += v * v;
      for (double v : cplus) nc += v * v;
      if (std::sqrt(nt) < 1e-6 && std::sqrt(nc) > 1e-6) return ExitStatus::LOCALLY_INFEASIBLE;
    }
    if (norm_inf(x.data(), n) > 1e10 || !all_finite(x.data(), n) || norm_inf(s.data(), m_i) > 1e10 ||
        !all_finite(s.data(), m_i))
      return ExitStatus::DIVERGING_ITERATES;

    for (const auto& cb : callbacks)
      if (cb({iterations, x, s, y, z, V, &st, in_feasibility_restoration})) return ExitStatus::CALLBACK_REQUESTED_STOP;

    // ---- Newton step on the device (:426-482) ----
    auto t0 = clk::now();
    dev.upload_x(x.data());
    dev.upload_duals(s.data(), y.data(), z.data());
    dev.upload_mu(&mu);
    dev.assemble();
    dev.build_rhs();
    rep.t_kkt_build += since(t0);  // enqueue time only: no host sync between the phases
    t0 = clk::now();
    // factorization attempts, each followed at once by solve + back-substitution
    auto info = sys.compute(/*solve_speculatively=*/true);
    rep.factorizations += sys.last_factorizations();
    rep.t_kkt_decomp += since(t0);
    if (info[0] != FactorInfo::Success) return ExitStatus::FACTORIZATION_FAILED;  // :463-465
    rep.delta = sys.hessian_regularization()[0];
    rep.gamma = sys.constraint_jacobian_regularization()[0];

    t0 = clk::now();
    rep.solves += sys.last_factorizations();
    download_direction(dev, n, m_e, m_i, p_x, p_y, p_s, p_z);
    rep.t_kkt_solve += since(t0);

    t0 = clk::now();
    const FilterEntry current_entry = make_entry(f, s, c_e.data(), m_e, c_i.data(), mu);
    double D_phi = 0.0;  // :508-509
    for (int i = 0; i < n; ++i) D_phi += g[i] * p_x[i];
    {
      double t = 0.0;
      for (int j = 0; j < m_i; ++j) t += (1.0 / s[j]) * p_s[j];
      D_phi -= mu * t;
    }
    ls.start(filter, full_step_rejected_counter, mu, current_entry, ftb(s, p_s, tau), ftb(z, p_z, tau), D_phi);  // :488, :497

    // f, c_e, c_i at trial_x; the trial point's four numbers for the line search
    auto trial_values = [&] {
      eval_values(trial_x);
      trial_f = Vtrial[st.off_f];
      std::copy(Vtrial.begin() + st.off_ce, Vtrial.begin() + st.off_ce + m_e, trial_c_e.begin());
      std::copy(Vtrial.begin() + st.off_ci, Vtrial.begin() + st.off_ci + m_i, trial_c_i.begin());
    };
    auto trial_out = [&] {
      const bool finite = std::isfinite(trial_f) && all_finite(trial_c_e.data(), m_e) && all_finite(trial_c_i.data(), m_i);
      double logsum = 0.0;
      for (int j = 0; j < m_i; ++j) logsum += std::log(trial_s[j]);
      return IpmTrialOut{trial_f, violation(trial_c_e, trial_c_i, trial_s), logsum, finite ? 1.0 : 0.0};
    };
    Vec soc_px(n), soc_ps(m_i), soc_py(m_e), soc_pz(m_i), c_e_soc, cims_soc(m_i);  // the corrected direction, its c_e, c_i - s

    while (ls.want != Want::Done) switch (ls.want) {
      case Want::Eval: {  // :513-528
        trial_x = axpy(x, ls.t_alpha, p_x);
        trial_values();
        bool all_pos = true;
        for (double v : c_i) all_pos = all_pos && v > 0.0;
        if (options.feasible_ipm && all_pos) trial_s = trial_c_i;
        else trial_s = axpy(s, ls.t_alpha, p_s);
        trial_y = axpy(y, ls.t_alpha_z, p_y);
        trial_z = axpy(z, ls.t_alpha_z, p_z);
        ls.on_trial(trial_out());
        break;
      }
      case Want::SocSolve: {  // :601-633: new rhs, SAME factorization
        if (ls.soc_first) {
          c_e_soc = c_e;
          for (int j = 0; j < m_i; ++j) cims_soc[j] = c_i[j] - s[j];
        }
        for (int j = 0; j < m_e; ++j) c_e_soc[j] = soc_accumulate(ls.alpha_soc, c_e_soc[j], trial_c_e[j]);
        for (int j = 0; j < m_i; ++j) cims_soc[j] = soc_accumulate(ls.alpha_soc, cims_soc[j], trial_c_i[j]) - trial_s[j];
        // rhs (:613-616) is O(nnz(A)) host work on the downloaded Jacobians
        Vec rhs(dim, 0.0);
        {
          Vec t(m_i);
          for (int j = 0; j < m_i; ++j) t[j] = soc_rhs_multiplier(mu, s[j], z[j], cims_soc[j]);
          for (int i = 0; i < n; ++i) rhs[i] = -g[i];
          add_At_v(st.Ae, cur.Ae(), nullptr, y.data(), 1.0, rhs);
          add_At_v(st.Ai, cur.Ai(), nullptr, t.data(), 1.0, rhs);
          for (int j = 0; j < m_e; ++j) rhs[n + j] = -c_e_soc[j];
        }
        SLPX_HIP_CHECK(hipMemcpyAsync(dev.d_rhs(), rhs.data(), dim * sizeof(double),
                                      hipMemcpyHostToDevice, dev.stream()));
        dev.solve();
        ++rep.solves;
        dev.download(dev.ldlt().d_p(), p.data(), dim);
        std::copy(p.begin(), p.begin() + n, soc_px.begin());
        for (int j = 0; j < m_e; ++j) soc_py[j] = -p[n + j];
        {  // p_s, p_z with the corrected c_i - s (:479-480)
          Vec aipx(m_i, 0.0);
          for (int c = 0; c < n; ++c)
            for (int q = st.Ai.colptr[c]; q < st.Ai.colptr[c + 1]; ++q)
              aipx[st.Ai.rowidx[q]] += cur.Ai()[q] * soc_px[c];
          for (int j = 0; j < m_i; ++j) {
            const double sinv = 1.0 / s[j];
            soc_ps[j] = cims_soc[j] + aipx[j];
            soc_pz[j] = backsub_pz_sinv(mu, sinv, z[j], soc_ps[j]);
          }
        }
        ls.on_soc_solve(ftb(s, soc_ps, tau), ftb(z, soc_pz, tau));
        break;
      }
      case Want::SocEval:
        trial_x = axpy(x, ls.t_alpha, soc_px);
        trial_s = axpy(s, ls.t_alpha, soc_ps);
        trial_y = axpy(y, ls.t_alpha_z, soc_py);
        trial_z = axpy(z, ls.t_alpha_z, soc_pz);
        trial_values();
        ls.on_trial(trial_out());
        break;
      case Want::KktEval: {  // :692-706
        const double current_kkt = kkt_error_impl<ErrType::ONE_NORM>(
            st, g, cur.Ae(), c_e.data(), cur.Ai(), c_i.data(), s, y, z, mu, nullptr);
        trial_x = axpy(x, ls.t_alpha, p_x);
        trial_s = axpy(s, ls.t_alpha, p_s);
        trial_y = axpy(y, ls.t_alpha_z, p_y);
        trial_z = axpy(z, ls.t_alpha_z, p_z);
        // needs g, A_e, A_i at the trial point: full sweep into a scratch copy
        Vec Vkeep = V;
        refresh_full(trial_x, trial_y, trial_z);
        Vec Vt = V;
        V = Vkeep;
        VView tv{st, Vt};
        trial_f = tv.f();
        std::copy(tv.c_e(), tv.c_e() + m_e, trial_c_e.begin());
        std::copy(tv.c_i(), tv.c_i() + m_i, trial_c_i.begin());
        ls.on_kkt_errors(current_kkt, kkt_error_impl<ErrType::ONE_NORM>(st, tv.g_dense(), tv.Ae(), trial_c_e.data(), tv.Ai(),
                                                                        trial_c_i.data(), trial_s, trial_y, trial_z, mu, nullptr));
        break;
      }
      case Want::Done: break;
    }
    const double alpha = ls.alpha, alpha_z = ls.alpha_z;
    rep.t_line_search += since(t0);

    if (ls.call_feasibility_restoration) {  // :721-771
      if (in_feasibility_restoration) return ExitStatus::FEASIBILITY_RESTORATION_FAILED;

      const FilterEntry initial_entry = current_entry;
      // Leave restoration once the outer filter accepts the restoration iterate and the violation dropped by 10 %
      // (:729-752); the restoration iteration reduces the outer problem's quantities at its iterate on the device
      auto outer_accepts = [&](const FilterEntry& trial_entry, double D_phi_restoration) {
        return filter.try_add(initial_entry, trial_entry, D_phi_restoration, alpha);
      };
      const ExitStatus fr_status = feasibility_restoration(sys, scales, callbacks, outer_accepts, options, x, s, y, z, mu, iterations,
                                                           rep, solve_start, c_e, c_i, g, initial_entry.constraint_violation);
      if (fr_status != ExitStatus::SUCCESS) return fr_status;
      trial_x = x;
      trial_values();
    } else {
      x = trial_x;
      s = trial_s;
      y = trial_y;
      z = trial_z;
      for (int j = 0; j < m_i; ++j) z[j] = z_reset(z[j], mu, s[j]);  // :797-801
    }
    f = trial_f;
    c_e = trial_c_e;
    c_i = trial_c_i;

    // AD refresh (:809-812)
    t0 = clk::now();
    refresh_full(x, y, z);
    g = cur.g_dense();
    rep.t_ad_refresh += since(t0);

    E_0 = E0_of(g, c_e, c_i, s, y, z);
    if (E_0 > options.tolerance)  // :819-832
      update_barrier_parameter(mu, mu_min, tau, filter, [&](double m) {
        return kkt_error_impl<ErrType::INF_NORM_SCALED>(st, g, cur.Ae(), c_e.data(), cur.Ai(), c_i.data(), s, y, z, m, nullptr);
      });
    if (options.diagnostics) print_iteration(iterations, E_0, f, violation(c_e, c_i, s), mu, rep, alpha, alpha_z, sys.last_factorizations());
    ++iterations;
    rep.final_error = E_0;
    if (iterations >= options.max_iterations) return ExitStatus::MAX_ITERATIONS_EXCEEDED;
    if (since(solve_start) > options.timeout) return ExitStatus::TIMEOUT;
  }
  rep.final_error = E_0;
  return ExitStatus::SUCCESS;
}

// SLPX_IPM_RESIDENT=0 keeps the O(n) logic between Newton steps on the host (the round-1
// arrangement; kept as the cross-check of the device-resident iteration).
ExitStatus ipm_core(NewtonSystem& sys, const Vec& scales, const std::vector<IterationCallback>& callbacks,
                    const Options& options, bool in_feasibility_restoration, Vec& x, Vec& s, Vec& y, Vec& z,
                    double& mu, int& iterations, SolveReport& rep, clk::time_point solve_start) {
  return (sys.switches().ipm_resident ? ipm_core_resident : ipm_core_host)(sys, scales, callbacks, options,
                                                        in_feasibility_restoration, x, s, y, z, mu, iterations,
                                                        rep, solve_start);
}

ExitStatus interior_point(NewtonSystem& sys, const std::vector<double>& scales,
                          const std::vector<IterationCallback>& callbacks, const Options& options,
                          std::vector<double>& x, std::vector<double>* s_out,
                          std::vector<double>* y_out, std::vector<double>* z_out,
                          SolveReport* report) {
  return interior_point(sys, scales, callbacks, options, x, s_out, y_out, z_out, report, nullptr, nullptr, nullptr);
}

ExitStatus interior_point(NewtonSystem& sys, const std::vector<double>& scales,
                          const std::vector<IterationCallback>& callbacks, const Options& options,
                          std::vector<double>& x, std::vector<double>* s_out, std::vector<double>* y_out,
                          std::vector<double>* z_out, SolveReport* report, const WarmStart* warm,
                          const double* c_i_unit, WarmStartResult* result) {
  const NlpStructure& st = sys.structure();
  const auto solve_start = clk::now();
  SolveReport local;
  SolveReport& rep = report ? *report : local;
  rep = SolveReport{};
  // interior_point.hpp:74-79
  Vec s(st.m_i, 1.0), y(st.m_e, 0.0), z(st.m_i, 1.0);
  double mu = 0.1 * scales[0];
  if (result) *result = WarmStartResult{};
  if (warm) {  // warm_start.h, steps 1-5
    const int m_e = st.m_e, m_i = st.m_i;
    check_warm_length(warm->s, m_i, "s");
    check_warm_length(warm->y, m_e, "y");
    check_warm_length(warm->z, m_i, "z");
    if (c_i_unit == nullptr) throw std::runtime_error("warm start: c_i at x0 is missing");
    if (any_bad(x) || any_bad(warm->s) || any_bad(warm->y) || any_bad(warm->z) || warm_bad(warm->mu)) {
      if (s_out) *s_out = s;
      if (y_out) *y_out = y;
      if (z_out) *z_out = z;
      if (result) result->mu = mu;
      return ExitStatus::NONFINITE_INITIAL_GUESS;
    }
    const double d_f = scales[0];
    const double* d_ce = scales.data() + 1;
    const double* d_ci = scales.data() + 1 + m_e;
    const bool has_s = !warm->s.empty(), has_z = !warm->z.empty();
    double sum = 0.0, count = 0.0;
    if (has_s && has_z)
      for (int j = 0; j < m_i; ++j) {
        const double sj = warm_scale_s(warm->s[j], d_ci[j]), zj = warm_scale_dual(warm->z[j], d_ci[j], d_f);
        if (warm_counts(sj, zj)) {
          sum += sj * zj;
          count += 1.0;
        }
      }
    mu = warm_mu(sum, count, warm->mu, d_f, barrier_floor(d_f, options.tolerance));
    if (!warm->y.empty())
      for (int j = 0; j < m_e; ++j) y[j] = warm_scale_dual(warm->y[j], d_ce[j], d_f);
    int repaired = 0;
    for (int j = 0; j < m_i; ++j) {
      const double d = d_ci[j];
      s[j] = warm_slack(has_s, has_s ? warm_scale_s(warm->s[j], d) : 0.0, d * c_i_unit[j], mu, &repaired);
      z[j] = warm_dual(has_z, has_z ? warm_scale_dual(warm->z[j], d, d_f) : 0.0, mu, s[j], &repaired);
    }
    if (result) result->repaired = repaired;
  }
  int iterations = 0;
  const ExitStatus status = ipm_core(sys, scales, callbacks, options, false, x, s, y, z, mu, iterations, rep, solve_start);
  rep.t_total = since(solve_start);
  if (s_out) *s_out = s;
  if (y_out) *y_out = y;
  if (z_out) *z_out = z;
  if (result) result->mu = mu;
  rep.iterations = iterations;
  return status;
}

}  // namespace slpx
