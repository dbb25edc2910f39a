#include "ipm.hpp"

#include "ipm_formulas.h"
#include "ipm_line_search.hpp"
#include "restoration.hpp"
#include "warm_start.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace slpx {

namespace {

using namespace ipm_host;
using Want = LineSearch::Want;
using End = LineSearch::End;

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

namespace {

ExitStatus feasibility_restoration(NewtonSystem& outer, const Vec& scales, const std::vector<IterationCallback>& user_callbacks,
                                   const std::function<bool(const FilterEntry&, double)>& outer_accepts, const Options& options,
                                   Vec& x, Vec& s, Vec& y, Vec& z, double mu, int& iterations, SolveReport& rep,
                                   clk::time_point solve_start, const Vec& c_e, const Vec& c_i, const Vec& g, double initial_violation);

// interior_point.hpp:129-878: the iteration proper, on caller-owned iterates (the
// restoration phase re-enters it with in_feasibility_restoration = true).
ExitStatus ipm_core_host(NewtonSystem& sys, const Vec& scales,
                         const std::vector<IterationCallback>& callbacks, const Options& options,
                         bool in_feasibility_restoration, Vec& x, Vec& s, Vec& y, Vec& z, double& mu,
                         int& iterations, SolveReport& rep, clk::time_point solve_start) {
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n, m_e = st.m_e, m_i = st.m_i, dim = n + m_e;
  auto finish = [&](ExitStatus st_) { return st_; };

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

  if (m_e > n) return finish(ExitStatus::TOO_FEW_DOFS);  // :274
  if (!all_finite(V.data(), st.nV)) return finish(ExitStatus::NONFINITE_INITIAL_GUESS);  // :283-286

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
    if (m_e > 0) {
      Vec t(n, 0.0);
      add_At_v(st.Ae, cur.Ae(), nullptr, c_e.data(), 1.0, t);
      double nt = 0.0, nc = 0.0;
      for (double v : t) nt += v * v;
      for (double v : c_e) nc += v * v;
      if (std::sqrt(nt) < 1e-6 && std::sqrt(nc) > 1e-2) return finish(ExitStatus::LOCALLY_INFEASIBLE);
    }
    if (m_i > 0) {
      Vec cplus(m_i), t(n, 0.0);
      for (int j = 0; j < m_i; ++j) cplus[j] = std::min(c_i[j], 0.0);
      add_At_v(st.Ai, cur.Ai(), nullptr, cplus.data(), 1.0, t);
      double nt = 0.0, nc = 0.0;
      for (double v : t) nt += v * v;
      for (double v : cplus) nc += v * v;
      if (std::sqrt(nt) < 1e-6 && std::sqrt(nc) > 1e-6) return finish(ExitStatus::LOCALLY_INFEASIBLE);
    }
    if (norm_inf(x.data(), n) > 1e10 || !all_finite(x.data(), n) || norm_inf(s.data(), m_i) > 1e10 ||
        !all_finite(s.data(), m_i))
      return finish(ExitStatus::DIVERGING_ITERATES);

    for (const auto& cb : callbacks)
      if (cb({iterations, x, s, y, z, V, &st, in_feasibility_restoration})) return finish(ExitStatus::CALLBACK_REQUESTED_STOP);

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
    if (info[0] != FactorInfo::Success) return finish(ExitStatus::FACTORIZATION_FAILED);  // :463-465
    rep.delta = sys.hessian_regularization()[0];
    rep.gamma = sys.constraint_jacobian_regularization()[0];

    auto download_step = [&](Vec& px, Vec& py, Vec& ps, Vec& pz) {
      dev.download(dev.ldlt().d_p(), p.data(), dim);
      std::copy(p.begin(), p.begin() + n, px.begin());
      for (int j = 0; j < m_e; ++j) py[j] = -p[n + j];
      if (m_i) {
        dev.download(dev.d_ps(), ps.data(), m_i);
        dev.download(dev.d_pz(), pz.data(), m_i);
      }
    };
    t0 = clk::now();
    rep.solves += sys.last_factorizations();
    download_step(p_x, p_y, p_s, p_z);
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
      if (in_feasibility_restoration) return finish(ExitStatus::FEASIBILITY_RESTORATION_FAILED);

      const FilterEntry initial_entry = current_entry;
      // Leave restoration once the outer filter accepts the restoration iterate and the violation dropped by 10 %
      // (:729-752); the restoration iteration reduces the outer problem's quantities at its iterate on the device
      auto outer_accepts = [&](const FilterEntry& trial_entry, double D_phi_restoration) {
        return filter.try_add(initial_entry, trial_entry, D_phi_restoration, alpha);
      };
      const ExitStatus fr_status = feasibility_restoration(sys, scales, callbacks, outer_accepts, options, x, s, y, z, mu, iterations,
                                                           rep, solve_start, c_e, c_i, g, initial_entry.constraint_violation);
      if (fr_status != ExitStatus::SUCCESS) return finish(fr_status);
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
    if (iterations >= options.max_iterations) return finish(ExitStatus::MAX_ITERATIONS_EXCEEDED);
    if (since(solve_start) > options.timeout) return finish(ExitStatus::TIMEOUT);
  }
  rep.final_error = E_0;
  return finish(ExitStatus::SUCCESS);
}

// The same iteration with the iterate, the step and every O(n) vector RESIDENT ON THE
// DEVICE (ipm_kernels.h): per iteration the host reads the
// inertia counters plus ~30 scalars (step sizes, directional derivative, filter entry of
// the trial point, error norms) and decides; it never sees a vector.  The kernels for the
// step sizes, the first trial point and its merit quantities are enqueued speculatively
// behind the Newton step, so the common iteration has two synchronizations: one after
// [step + first trial], one after [iterate update + AD refresh + error norms].
// Rare branches (the KKT-error fallback of the line search, feasibility restoration, user
// callbacks) pull the iterate to the host and reuse the host code above.
ExitStatus ipm_core_resident(NewtonSystem& sys, const Vec& scales,
                             const std::vector<IterationCallback>& callbacks, const Options& options,
                             bool in_feasibility_restoration, Vec& x, Vec& s, Vec& y, Vec& z, double& mu,
                             int& iterations, SolveReport& rep, clk::time_point solve_start) {
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n, m_e = st.m_e, m_i = st.m_i, dim = n + m_e;
  dev.ipm_enable();
  dev.ipm_set_error_scaling(scales);
  // (two sets of the scalar outputs, taken in turn by the iterations: the pipelined common iteration below enqueues
  // iteration k+1's launches before the host has read iteration k's)
  int slot = 0;
  dev.ipm_set_slot(slot);
  const IpmHost* Hp = &dev.ipm_host_slot(slot);
#define H (*Hp)

  sys.reset_regularization();
  sys.set_gamma_min(in_feasibility_restoration ? 0.0 : 1e-10);  // :350-352

  bool host_current = true;  // x, s, y, z on the host mirror the device iterate
  auto pull_state = [&] {
    if (host_current) return;
    dev.download(dev.d_x(), x.data(), n);
    if (m_i) {
      dev.download(dev.d_s(), s.data(), m_i);
      dev.download(dev.d_z(), z.data(), m_i);
    }
    if (m_e) dev.download(dev.d_y(), y.data(), m_e);
    host_current = true;
  };
  auto push_state = [&] {
    dev.upload_x(x.data());
    dev.upload_duals(s.data(), y.data(), z.data());
    host_current = true;
  };
  long twin_launches = 0, twin_taken = 0;
  bool spec_in_flight = false;  // the NEXT iteration's step and chain are enqueued already (and will run)
  bool spec_rides = false;      // ... and that step carries its own verdict (it runs whatever that is)
  long pipelined = 0, passed = 0;
  auto finish = [&](ExitStatus st_) {
    if (spec_in_flight) {  // (the step enqueued ahead runs for nothing: wait for it, forget it)
      dev.wait_published();
      sys.cancel_speculative_compute(/*launch_ran=*/spec_rides);
      spec_in_flight = false;
    }
    sys.set_after_attempt(nullptr);
    sys.set_twin_attempts(false);
    dev.ipm_set_slot(0);
    pull_state();
    if (std::getenv("SLPX_TWIN_VERBOSE")) {
      std::fprintf(stderr, "slpx pipelined iterations: %ld decided on the device, %ld steps enqueued ahead passed, of %d iterations\n",
                   pipelined, passed, iterations);
      const long* h = sys.twin_histogram();
      std::fprintf(stderr, "slpx twin attempts: %ld launches held two attempts, the policy took the second of %ld (%d factorizations, %d iterations); "
                   "first attempts of this system so far: %ld accepted, %ld / %ld with the failure the second stood for and the second accepted / not, "
                   "%ld with zero pivots, %ld with the other inertia failure, %ld failed\n",
                   twin_launches, twin_taken, rep.factorizations, iterations, h[0], h[1], h[2], h[3], h[4], h[5]);
    }
    return st_;
  };

  auto t_setup = clk::now();
  push_state();
  dev.upload_mu(&mu);
  double mu_on_device = mu;
  dev.sweep_full(/*with_reduce=*/false);  // :245-251 (the separable sums ride in the error launch)
  dev.ipm_errors(/*check_all_V=*/true, /*sums_ride=*/true);
  dev.wait_published();
  IpmErrOut cur = H.err;  // scalars of the current iterate

  if (m_e > n) return finish(ExitStatus::TOO_FEW_DOFS);                        // :274
  if (cur.finite == 0.0) return finish(ExitStatus::NONFINITE_INITIAL_GUESS);  // :283-286

  const double mu_min = barrier_floor(scales[0], options.tolerance);
  double tau = kTauMin;
  Filter filter{cur.viol};  // :303
  int full_step_rejected_counter = 0;
  LineSearch ls;
  const bool identity = scaling_is_identity(st, scales);
  const bool lookahead = sys.switches().ipm_lookahead;
  double E_0 = ipm_E_0(cur, m_e, m_i, identity);  // :361-362
  rep.t_setup = since(t_setup);

  // ---- the pipelined common iteration (ipm_decide.h) ----
  // Most iterations end the same way: the filter takes the full step the look-ahead launch evaluated, the error is
  // above the tolerance, the barrier parameter stays.  Those decisions are then taken ON THE DEVICE, by the launch that
  // reduces the look-ahead iterate's norms — and the next iteration's step, with its chain, is enqueued as soon as this
  // iteration's factorization is accepted, BEFORE the verdict exists.  The deciding launch RIDES in that step's launch
  // (DeviceNlp::ipm_ride_errors_in_next_step): the step factors beside it and holds its results back until the verdict
  // is in; if the host has to look (a rejected step, a barrier update, convergence, anything rare) the step has run for
  // nothing and what was enqueued behind it passes.  (SLPX_IPM_RIDE=0, or where the riding workgroups do not fit beside
  // the tasks: the deciding launch in front of the step, which reads the word it leaves and passes if told to.)
  // The host then only follows: one poll per iteration, no launch on the critical path.
  // SLPX_IPM_PIPELINE=0: every iteration decided by the host, as before.
  const bool pipeline_on = lookahead && callbacks.empty() && !options.feasible_ipm && sys.switches().ipm_pipeline;
  const bool ride_on = pipeline_on && dev.ipm_ride_possible();  // (SLPX_IPM_RIDE=0: the error launch in front of the gated step)
  bool ctl_current = false;      // the device's copy of (filter, current iterate's entry, mu) is the host's
  bool filter_on_device = false; // ... and newer than the host's: the device took decisions since
  auto sync_filter_from_device = [&] {
    if (!filter_on_device) return;
    filter.from_state(dev.ipm_pipeline_fetch().filter);
    filter_on_device = false;
  };
  auto upload_ctl = [&]() -> bool {
    static thread_local IpmCtl c;
    if (!filter.to_state(c.filter)) return false;
    c.mu = mu;
    c.mu_min = mu_min;
    c.tolerance = options.tolerance;
    c.cur_f = cur.f;
    c.cur_logsum = cur.logsum;
    c.cur_viol = cur.viol;
    c.m_e = m_e;
    c.m_i = m_i;
    c.identity_scaling = identity ? 1 : 0;
    dev.ipm_pipeline_upload(c);
    ctl_current = true;
    return true;
  };

  // host copies for the rare branches
  Vec V, p(dim), p_x(n), p_y(m_e), p_s(m_i), p_z(m_i);
  auto pull_V = [&] {
    V.resize(st.nV);
    dev.download_V(V.data());
  };

  while (E_0 > options.tolerance) {
    if (const ExitStatus exit = infeasible_or_diverging(cur, m_e, m_i); exit != ExitStatus::SUCCESS) return finish(exit);  // :387-408

    if (!callbacks.empty()) {
      pull_state();
      pull_V();
      for (const auto& cb : callbacks)
        if (cb({iterations, x, s, y, z, V, &st, in_feasibility_restoration})) return finish(ExitStatus::CALLBACK_REQUESTED_STOP);
      push_state();  // a callback may have used this system's device buffers (restoration does)
    }

    // ---- Newton step (:426-482), then speculatively: step sizes, first trial point ----
    auto t0 = clk::now();
    const bool s_from_ci = options.feasible_ipm && cur.ci_all_pos != 0.0;
    const bool ahead = lookahead && !s_from_ci;
    if (mu != mu_on_device) {
      dev.upload_mu(&mu);
      mu_on_device = mu;
    }
    const bool resumed = spec_in_flight;  // this iteration's first launch (and chain) were enqueued by the one before
    spec_in_flight = false;
    // will THIS iteration's chain decide?  (its state on the device must be the host's, or the device's own)
    bool deciding = pipeline_on && ahead && (resumed || ctl_current || upload_ctl());
    if (!deciding) ctl_current = false;
    if (!resumed) dev.build_kkt_for_step(/*with_reduce=*/false);
    // Look-ahead (DeviceNlp::ipm_lookahead): instead of only f, c_e, c_i at the first trial point, the
    // WHOLE next iterate the full step would give — updated s, y, z, the full tape at it, the error norms
    // of :809-832 — is computed speculatively behind the step kernel, in a second set of buffers.  Most
    // iterations take the first trial point: the iteration is then complete when these numbers arrive
    // (one host round trip, four launches), and nothing is computed twice.  The feasible-IPM option
    // derives the trial s from the trial c_i (:520-526): it keeps the trial-values chain below.
    // (the error launch of a deciding chain comes LATER: riding in the next step's launch — it decides whether that
    // step counts while the step factors — or on its own where no step is enqueued ahead)
    const bool errors_later = deciding && ride_on;
    sys.set_after_attempt([&] {
      if (ahead) {
        dev.ipm_lookahead(tau);
        dev.sweep_full_lookahead();
        if (errors_later) {
        } else if (deciding) dev.ipm_errors_deciding(/*sums_ride=*/true);
        else dev.ipm_errors(false, /*sums_ride=*/true, /*ahead=*/true);
      } else {
        dev.ipm_direction(tau);
        dev.sweep_values_trial();
        dev.ipm_trial_metrics(-1.0, s_from_ci);
      }
    });
    // (twin attempts, NewtonSystem::compute_twin: the look-ahead launch takes the direction of whichever of a
    // launch's two attempts the regularization policy takes — the other after_attempt chain does not)
    sys.set_twin_attempts(ahead);
    auto info = sys.compute(/*solve_speculatively=*/true);
    twin_launches += sys.last_twin_launches();
    twin_taken += sys.last_twin_taken();
    // ---- the next iteration's step, ahead of this one's verdict ----
    bool spec = false, rode = false;
    if (deciding && info[0] == FactorInfo::Success && iterations + 2 < options.max_iterations) {
      dev.ipm_accept_lookahead();  // (the roles the buffers have if the device takes the step; put back below if not)
      dev.ipm_set_slot(slot ^ 1);
      // (the chain of the step enqueued ahead decides too: the device's state is its own by then)
      if (errors_later) rode = dev.ipm_ride_errors_in_next_step(slot);
      spec = sys.begin_speculative_compute(/*gated=*/!rode);
      if (!spec) {
        rode = false;
        dev.ipm_accept_lookahead();
        dev.ipm_set_slot(slot);
      }
    }
    if (errors_later && !rode) {
      if (spec) throw std::logic_error("slpx: a step enqueued ahead of its own verdict");
      dev.ipm_errors_deciding(/*sums_ride=*/true);  // (nothing was enqueued ahead: the error launch on its own)
    }
    const unsigned long long seq_this = dev.seq_expected();  // a chain that holds its error launch ends with this publication
    sys.set_twin_attempts(false);
    sys.set_after_attempt(nullptr);
    bool device_took_it = false;
    if (rode) {
      device_took_it = dev.ipm_ride_wait(slot);  // (the riding launch's scalars are in when its verdict is)
    } else {
      dev.wait_published_until(seq_this);  // compute() returns when the inertia counters are in; the trial chain may still run
      device_took_it = spec && H.go != 0.0;
    }
    if (spec) {
      if (device_took_it) {
        // the device took this iteration's decisions (ipm_decide.h): the filter accepted the full step, the
        // error is above the tolerance, mu stays; the next step is on its way.  The host follows.
        ++pipelined;
        rep.factorizations += sys.last_factorizations();
        rep.solves += sys.last_factorizations();
        rep.value_sweeps += sys.last_factorizations();
        rep.t_kkt_decomp += since(t0);
        rep.delta = sys.hessian_regularization()[0];
        rep.gamma = sys.constraint_jacobian_regularization()[0];
        full_step_rejected_counter = 0;
        host_current = false;
        filter_on_device = true;
        cur = H.err_ahead;
        E_0 = ipm_E_0(cur, m_e, m_i, identity);
        if (options.diagnostics)
          print_iteration(iterations, E_0, cur.f, cur.viol, mu, rep, H.dir.alpha_max, H.dir.alpha_z, sys.last_factorizations());
        ++iterations;
        rep.final_error = E_0;
        slot ^= 1;
        Hp = &dev.ipm_host_slot(slot);
        spec_in_flight = true;
        spec_rides = rode;
        if (since(solve_start) > options.timeout) return finish(ExitStatus::TIMEOUT);
        continue;
      }
      // the host has to look: what was enqueued ahead passes (a gated step at once; a step that carried its own verdict
      // runs and holds its results back, the chain behind it passes) — as if it had never been launched.  No waiting for
      // any of it: what the host enqueues next runs behind it in the stream's order, and it writes nothing the host or a
      // later launch reads but its sequence numbers.
      ++passed;
      sys.cancel_speculative_compute(/*launch_ran=*/rode);  // (a step that carried its own verdict ran, and held its results back)
      dev.ipm_accept_lookahead();
      dev.ipm_set_slot(slot);
    }
    ctl_current = false;  // (whatever happens below changes the filter, the iterate or mu on the host's side)
    sync_filter_from_device();
    rep.factorizations += sys.last_factorizations();
    rep.solves += sys.last_factorizations();
    rep.value_sweeps += sys.last_factorizations();
    rep.t_kkt_decomp += since(t0);
    if (info[0] != FactorInfo::Success) return finish(ExitStatus::FACTORIZATION_FAILED);  // :463-465
    rep.delta = sys.hessian_regularization()[0];
    rep.gamma = sys.constraint_jacobian_regularization()[0];

    t0 = clk::now();
    const FilterEntry current_entry{cur.f - mu * cur.logsum, cur.viol};
    ls.start(filter, full_step_rejected_counter, mu, current_entry, H.dir.alpha_max, H.dir.alpha_z, H.dir.D_phi);  // :488-509
    bool have_trial = true;       // the speculative chain already evaluated alpha_max
    bool took_lookahead = false;  // ... as the complete look-ahead iterate, and the filter took it

    while (ls.want != Want::Done) switch (ls.want) {
      case Want::Eval: {
        const bool from_ahead = have_trial && ahead;
        if (!have_trial) {
          dev.ipm_trial_point(ls.t_alpha);
          dev.sweep_values_trial();
          dev.ipm_trial_metrics(ls.t_alpha, s_from_ci);
          dev.wait_published();
          ++rep.value_sweeps;
        }
        have_trial = false;
        ls.on_trial(from_ahead ? IpmTrialOut{H.err_ahead.f, H.err_ahead.viol, H.err_ahead.logsum, H.err_ahead.finite} : H.trial);
        took_lookahead = from_ahead && ls.end == End::Newton;
        break;
      }
      case Want::SocSolve:  // :601-633: new rhs, SAME factorization, all on the device
        if (ls.soc_first) dev.ipm_save_direction();
        dev.ipm_soc_accumulate(ls.alpha_soc, ls.soc_first, ls.soc_first && s_from_ci);
        dev.ipm_soc_rhs();
        dev.solve();
        ++rep.solves;
        dev.ipm_soc_backsub();
        dev.ipm_direction(tau);  // step sizes of the corrected direction + its trial point
        dev.sweep_values_trial();
        dev.ipm_trial_metrics(-1.0, false);
        dev.wait_published();
        ++rep.value_sweeps;
        ls.on_soc_solve(H.dir.alpha_max, H.dir.alpha_z);
        ls.on_trial(H.trial);  // (SocEval: the chain above evaluated the corrected trial point already)
        if (!ls.on_correction) dev.ipm_restore_direction();  // the corrections failed: back to the Newton direction
        break;
      case Want::KktEval: {  // :691-716 — rare: on the host, with the iterate pulled over
        pull_state();
        pull_V();
        VView cv{st, V};
        const Vec g = cv.g_dense();
        const double current_kkt = kkt_error_impl<ErrType::ONE_NORM>(st, g, cv.Ae(), cv.c_e(), cv.Ai(),
                                                                     cv.c_i(), s, y, z, mu, nullptr);
        dev.download(dev.ldlt().d_p(), p.data(), dim);
        std::copy(p.begin(), p.begin() + n, p_x.begin());
        for (int j = 0; j < m_e; ++j) p_y[j] = -p[n + j];
        if (m_i) {
          dev.download(dev.d_ps(), p_s.data(), m_i);
          dev.download(dev.d_pz(), p_z.data(), m_i);
        }
        const Vec trial_x = axpy(x, ls.t_alpha, p_x), trial_s = axpy(s, ls.t_alpha, p_s),
                  trial_y = axpy(y, ls.t_alpha_z, p_y), trial_z = axpy(z, ls.t_alpha_z, p_z);
        // needs g, A_e, A_i at the trial point: full sweep there, then put the iterate back
        dev.upload_x(trial_x.data());
        dev.upload_duals(s.data(), trial_y.data(), trial_z.data());
        dev.sweep_full();
        Vec Vt(st.nV);
        dev.download_V(Vt.data());
        push_state();
        // the device V must describe x again (feasibility_restoration.hpp:393-394 evaluates at
        // the current iterate): the restoration entry below, and the next step if the fallback
        // accepts, read it
        dev.sweep_full();
        VView tv{st, Vt};
        ls.on_kkt_errors(current_kkt, kkt_error_impl<ErrType::ONE_NORM>(st, tv.g_dense(), tv.Ae(), tv.c_e(), tv.Ai(), tv.c_i(),
                                                                        trial_s, trial_y, trial_z, mu, nullptr));
        break;
      }
      default: break;
    }
    const double alpha = ls.alpha, alpha_z = ls.alpha_z;
    const bool call_feasibility_restoration = ls.call_feasibility_restoration;
    rep.t_line_search += since(t0);

    t0 = clk::now();
    if (call_feasibility_restoration) {  // :721-771 — rare: host vectors, as in ipm_core_host
      if (in_feasibility_restoration) return finish(ExitStatus::FEASIBILITY_RESTORATION_FAILED);
      pull_state();
      pull_V();
      VView cv{st, V};
      const Vec g = cv.g_dense();
      const Vec c_e(cv.c_e(), cv.c_e() + m_e), c_i(cv.c_i(), cv.c_i() + m_i);
      const double f = cv.f();
      const FilterEntry initial_entry = make_entry(f, s, c_e.data(), m_e, c_i.data(), mu);
      // Leave restoration once the outer filter accepts the restoration iterate and the
      // violation dropped by 10 % (:729-752).
      auto outer_accepts = [&](const FilterEntry& trial_entry, double D_phi_restoration) {
        return filter.try_add(initial_entry, trial_entry, D_phi_restoration, alpha);
      };
      const ExitStatus fr_status = feasibility_restoration(sys, scales, callbacks, outer_accepts, options, x, s, y, z, mu, iterations,
                                                           rep, solve_start, c_e, c_i, g, initial_entry.constraint_violation);
      if (fr_status != ExitStatus::SUCCESS) return finish(fr_status);
      push_state();
    } else {
      if (took_lookahead) {
        dev.ipm_accept_lookahead();  // :775-801 happened in ipm_lookahead_kernel; the buffers change roles
      } else {  // :775-801; the feasible-IPM choice of s holds for a trial point along the Newton direction only
        dev.ipm_commit(ls.end == End::Fallback ? ls.alpha_max : alpha, alpha_z, s_from_ci && ls.end == End::Newton);
      }
      host_current = false;
    }

    // AD refresh (:809-812) and every norm the next decisions need
    if (took_lookahead && !call_feasibility_restoration) {
      cur = H.err_ahead;  // already there: the look-ahead chain swept and reduced this iterate
    } else {
      dev.sweep_full(/*with_reduce=*/false);
      dev.ipm_errors(false, /*sums_ride=*/true);
      dev.wait_published();
      cur = H.err;
    }
    rep.t_ad_refresh += since(t0);

    E_0 = ipm_E_0(cur, m_e, m_i, identity);
    if (E_0 > options.tolerance)  // :819-832
      update_barrier_parameter(mu, mu_min, tau, filter, [&](double m) { return ipm_E_mu(cur, m, m_e, m_i); });
    if (options.diagnostics) print_iteration(iterations, E_0, cur.f, cur.viol, mu, rep, alpha, alpha_z, sys.last_factorizations());
    ++iterations;
    rep.final_error = E_0;
    if (iterations >= options.max_iterations) return finish(ExitStatus::MAX_ITERATIONS_EXCEEDED);
    if (since(solve_start) > options.timeout) return finish(ExitStatus::TIMEOUT);
  }
  rep.final_error = E_0;
  return finish(ExitStatus::SUCCESS);
}

#undef H

// SLPX_IPM_RESIDENT=0 keeps the O(n) logic between Newton steps on the host (the round-1
// arrangement; kept as the cross-check of the device-resident iteration).
ExitStatus ipm_core(NewtonSystem& sys, const Vec& scales, const std::vector<IterationCallback>& callbacks,
                    const Options& options, bool in_feasibility_restoration, Vec& x, Vec& s, Vec& y, Vec& z,
                    double& mu, int& iterations, SolveReport& rep, clk::time_point solve_start) {
  return (sys.switches().ipm_resident ? ipm_core_resident : ipm_core_host)(sys, scales, callbacks, options,
                                                        in_feasibility_restoration, x, s, y, z, mu, iterations,
                                                        rep, solve_start);
}

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
  const int n = st.n, m_e = st.m_e, m_i = st.m_i, M = 2 * m_e + 2 * m_i, dim = n + m_e, mi_ext = m_i + M;
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
        Vec p(dim), ps0(m_i), pz0(m_i), dpn(M), psx(M), pzx(M);
        dev.download(dev.ldlt().d_p(), p.data(), dim);
        if (m_i) {
          dev.download(dev.d_ps(), ps0.data(), m_i);
          dev.download(dev.d_pz(), pz0.data(), m_i);
        }
        fr.download_direction(dpn.data(), psx.data(), pzx.data());
        Vec Xt(X), St(S), yt(y), Zt(Z);
        for (int k = 0; k < n; ++k) Xt[k] += alpha_max * p[k];
        for (int e = 0; e < M; ++e) {
          Xt[n + e] += alpha_max * dpn[e];
          St[m_i + e] += alpha_max * psx[e];
          Zt[m_i + e] += alpha_z * pzx[e];
        }
        for (int r = 0; r < m_i; ++r) {
          St[r] += alpha_max * ps0[r];
          Zt[r] += alpha_z * pz0[r];
        }
        for (int j = 0; j < m_e; ++j) yt[j] += alpha_z * (-p[n + j]);
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

}  // namespace

// ---------------------------------------------------------------------------
// The reference's other two solvers on the same device Newton step:
// Problem::solve sends problems without constraints to newton() and problems with equality
// constraints only to sqp() (problem.hpp:335, 403).  Both are the interior-point iteration
// with its inequality machinery taken out — but not quite the m_i = 0 special case of it: SQP
// moves y with the primal step size (the IPM would take alpha_z = 1), Newton's line search
// goes down to alpha = 1e-20 and ends in LINE_SEARCH_FAILED instead of a restoration phase.
// Host-resident drivers (one value sweep per trial point crosses PCIe): these are the small
// problems of the reference's unit tests, not the benchmark path.
// ---------------------------------------------------------------------------
namespace {

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

  Vec p(dim), p_x(n), p_y(m_e), trial_x, trial_y, trial_c_e(m_e);
  double trial_f = 0.0;
  // f, c_e at trial_x: the trial point's numbers for the line search (no slacks: no barrier term)
  auto trial_out = [&] {
    eval_values(trial_x);
    trial_f = Vtrial[st.off_f];
    std::copy(Vtrial.begin() + st.off_ce, Vtrial.begin() + st.off_ce + m_e, trial_c_e.begin());
    const bool finite = std::isfinite(trial_f) && all_finite(trial_c_e.data(), m_e);
    return IpmTrialOut{trial_f, norm_1(trial_c_e.data(), m_e), 0.0, finite ? 1.0 : 0.0};
  };
  auto solve_step = [&](Vec& px, Vec& py) {
    dev.download(dev.ldlt().d_p(), p.data(), dim);
    std::copy(p.begin(), p.begin() + n, px.begin());
    for (int j = 0; j < m_e; ++j) py[j] = -p[n + j];
  };

  while (E_0 > options.tolerance) {
    // :277-292 infeasibility / divergence checks
    if (m_e > 0) {
      Vec t(n, 0.0);
      add_At_v(st.Ae, cur.Ae(), nullptr, c_e.data(), 1.0, t);
      double nt = 0.0, nc = 0.0;
      for (double v : t) nt += v * v;
      for (double v : c_e) nc += v * v;
      if (std::sqrt(nt) < 1e-6 && std::sqrt(nc) > 1e-2) return ExitStatus::LOCALLY_INFEASIBLE;
    }
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
    solve_step(p_x, p_y);
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
        solve_step(soc_px, soc_py);
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

namespace {
void check_warm_length(const Vec& v, int want, const char* what) {
  if (!v.empty() && static_cast<int>(v.size()) != want)
    throw std::runtime_error(std::string("warm start: ") + what + " has the wrong length");
}
bool any_bad(const Vec& v) {
  for (double e : v)
    if (warm_bad(e)) return true;
  return false;
}
}  // namespace

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
