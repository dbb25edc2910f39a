// The batched lockstep drivers of models without inequality constraints (eq_batch.hpp): SQP (sqp.hpp:98-604) and
// Newton (newton.hpp:51-292) as sqp_core / newton_core (ipm.cpp) restate them, per instance.  The loop is that of
// interior_point_batch: one Newton step for every running instance, the line search in rounds of masked launches,
// commit, refresh, exits.  The decisions are the shared host code's (LineSearch, Filter, ipm_E_0,
// infeasible_or_diverging) on the scalars of batch_errors_kernel; only Newton's own search (newton.hpp:201-243: no
// corrections, no restoration, a floor of 1e-20) is spelled out here, as it is in newton_core.
#include "eq_batch.hpp"

#include <optional>

#include "ipm_line_search.hpp"

namespace slpx {

using namespace ipm_host;

namespace {

using Want = LineSearch::Want;

struct Instance {
  bool running = false;
  ExitStatus status = ExitStatus::SUCCESS;
  Vec scales;
  bool identity = false;  // problem_scaling.hpp:111-113
  int iterations = 0;
  SolveReport rep;
  std::optional<Filter> filter;
  int full_step_rejected_counter = 0;
  IpmErrOut cur{};  // the last refresh's reductions
  double E_0 = 0.0;
  double f = 0.0;  // Newton: the cost the filter compares with (the accepted trial point's, newton.hpp:246-247)
  double D_phi = 0.0;
  FilterEntry current_entry;
  LineSearch ls;  // SQP: where the instance stands in its line search; Newton: `want` and `alpha` of its own search
};

constexpr double kNewtonAlphaMin = 1e-20;  // newton.hpp:138-139

void eq_batch(bool newton, NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
              const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out) {
  const auto solve_start = clk::now();
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int B = sys.batch(), n = st.n, m_e = st.m_e, ns = st.n_scales();
  if (static_cast<int>(x0.size()) != B * n || static_cast<int>(scales.size()) != B * ns || static_cast<int>(run.size()) != B)
    throw std::runtime_error("eq_batch: wrong lengths");
  if (st.m_i != 0) throw std::runtime_error("eq_batch: a problem without inequality constraints only");
  if (newton != (m_e == 0)) throw std::runtime_error("eq_batch: newton_batch takes m_e == 0, sqp_batch m_e > 0");
  SolveReport& rep = out.report;
  out.driver = newton ? 3 : 2;
  out.rounds = out.handoffs = 0;

  BatchEqDevice bd(sys);
  bd.set_scales(scales);
  sys.reset_regularization();
  sys.set_gamma_min(1e-10);  // sparse_regularized_ldlt.hpp:197

  std::vector<Instance> inst(B);
  for (int b = 0; b < B; ++b) {
    Instance& I = inst[b];
    I.scales.assign(scales.begin() + static_cast<size_t>(b) * ns, scales.begin() + static_cast<size_t>(b + 1) * ns);
    I.identity = scaling_is_identity(st, I.scales);
    I.running = run[b] != 0;
  }
  bd.set_iterate(x0, Vec(static_cast<size_t>(B) * m_e, 0.0));  // problem.hpp:503-504: y = 0
  const Vec mu0(B, 0.0);

  // the per-instance parameters of the next launches, for the instances `pred` selects
  auto launch_for = [&](auto pred) {
    bool any = false;
    for (int b = 0; b < B; ++b) {
      const Instance& I = inst[b];
      bd.active[b] = pred(I) ? 1 : 0;
      any = any || bd.active[b];
      // Newton's fallback looks at the full step (newton.hpp:226); every other trial point is at t_alpha
      bd.alpha[b] = newton && I.ls.want == Want::KktEval ? 1.0 : I.ls.t_alpha;
      bd.alpha_soc[b] = I.ls.alpha_soc;
      bd.mode[b] = I.ls.on_correction ? 1 : 0;
      bd.first[b] = I.ls.soc_first ? 1 : 0;
    }
    if (any) bd.upload();
    return any;
  };
  auto running = [](const Instance& I) { return I.running; };
  auto finish = [&](Instance& I, ExitStatus s_) {
    I.status = s_;
    I.running = false;
    I.ls.want = Want::Done;
  };
  Vec err, dphi, met, err_cur, err_trial;
  auto take_refresh = [&](Instance& I, int b) {
    I.cur = err_of(err.data() + static_cast<size_t>(b) * kBatchErrN);
    // (m_i = 0, and for Newton m_e = 0 too: the divisors of the scale factors are 0, the quotients NaN, and fmax
    // drops a NaN as std::max does one in its second argument: both factors are 1, as on the host)
    I.E_0 = ipm_E_0(I.cur, m_e, 0, I.identity);
  };

  // ---- setup (sqp.hpp:182-254, newton.hpp:108-150) ----
  auto t0 = clk::now();
  if (launch_for(running)) bd.refresh(err);
  for (int b = 0; b < B; ++b) {
    Instance& I = inst[b];
    if (!I.running) continue;
    take_refresh(I, b);
    if (m_e > n) {  // sqp.hpp:205-210
      finish(I, ExitStatus::TOO_FEW_DOFS);
      continue;
    }
    if (err[static_cast<size_t>(b) * kBatchErrN + BE_V_BAD] != 0.0) {  // sqp.hpp:213-216, newton.hpp:125-127
      finish(I, ExitStatus::NONFINITE_INITIAL_GUESS);
      continue;
    }
    I.f = I.cur.f;
    I.filter.emplace(I.cur.viol);  // sqp.hpp:220 (||c_e||_1), newton.hpp:131 (0)
    if (!(I.E_0 > options.tolerance)) finish(I, ExitStatus::SUCCESS);
  }
  rep.t_setup = since(t0);

  while (true) {
    // sqp.hpp:277-292, newton.hpp:164: infeasibility (where there are rows) / divergence, from the last refresh
    for (auto& I : inst) {
      if (!I.running) continue;
      const ExitStatus exit = infeasible_or_diverging(I.cur, m_e, 0);
      if (exit != ExitStatus::SUCCESS) finish(I, exit);
    }
    if (!launch_for(running)) break;

    // ---- Newton-KKT step of every running instance (sqp.hpp:305-346, newton.hpp:182-190) ----
    t0 = clk::now();
    dev.upload_mu(mu0.data());
    dev.assemble();
    dev.build_rhs();
    rep.t_kkt_build += since(t0);
    t0 = clk::now();
    const std::vector<FactorInfo> info = sys.compute(/*solve_speculatively=*/true, bd.active);
    ++out.rounds;
    rep.factorizations += sys.last_factorizations();
    rep.solves += sys.last_factorizations();
    rep.t_kkt_decomp += since(t0);
    t0 = clk::now();
    bd.direction(dphi);
    rep.t_kkt_solve += since(t0);

    t0 = clk::now();
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running) continue;
      if (info[b] != FactorInfo::Success) {  // sqp.hpp:336-338
        finish(I, ExitStatus::FACTORIZATION_FAILED);
        continue;
      }
      I.D_phi = dphi[b];
      if (newton) {
        I.current_entry = FilterEntry{I.f, 0.0};
        I.ls.on_correction = false;
        I.ls.call_feasibility_restoration = false;
        I.ls.alpha = I.ls.t_alpha = 1.0;
        I.ls.want = Want::Eval;
      } else {
        // the interior-point line search with alpha_max = 1 and no barrier term; y moves with the primal step
        I.current_entry = FilterEntry{I.cur.f, I.cur.viol};
        I.ls.start(*I.filter, I.full_step_rejected_counter, 0.0, I.current_entry, 1.0, 1.0, I.D_phi);
      }
    }

    // ---- the line search in rounds: one masked launch per kind of work still wanted ----
    while (true) {
      if (launch_for([](const Instance& I) { return I.running && I.ls.want == Want::SocSolve; })) {
        bd.soc_step();
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          ++rep.solves;
          inst[b].ls.on_soc_solve(inst[b].ls.alpha_max, inst[b].ls.alpha_max);  // a correction keeps the full step
        }
      }
      if (launch_for([](const Instance& I) { return I.running && (I.ls.want == Want::Eval || I.ls.want == Want::SocEval); })) {
        bd.trial_values(met);
        ++rep.value_sweeps;
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          Instance& I = inst[b];
          const double* m = met.data() + 3 * b;  // f, ||c_e||_1, non-finite count
          if (!newton) {
            I.ls.on_trial(IpmTrialOut{m[0], m[1], 0.0, m[2] == 0.0 ? 1.0 : 0.0});
            continue;
          }
          // newton.hpp:201-243
          double& alpha = I.ls.alpha;
          if (m[2] == 0.0 && I.filter->try_add(I.current_entry, FilterEntry{m[0], 0.0}, I.D_phi, alpha)) {
            I.f = m[0];
            I.ls.want = Want::Done;
            continue;
          }
          alpha *= kAlphaReduction;
          I.ls.t_alpha = alpha;
          if (alpha < kNewtonAlphaMin) {
            if (m[2] != 0.0) finish(I, ExitStatus::LINE_SEARCH_FAILED);  // (a non-finite cost has no fallback)
            else I.ls.want = Want::KktEval;
          }
        }
      }
      if (launch_for([](const Instance& I) { return I.running && I.ls.want == Want::KktEval; })) {
        bd.kkt_fallback(err_cur, err_trial);
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          Instance& I = inst[b];
          const double* ec = err_cur.data() + static_cast<size_t>(b) * kBatchErrN;
          const double* et = err_trial.data() + static_cast<size_t>(b) * kBatchErrN;
          if (!newton) {
            I.ls.on_kkt_errors(error_one_norm(ec), error_one_norm(et));
          } else if (error_one_norm(et) <= kFallbackDecrease * error_one_norm(ec)) {  // ||g||_1 (newton.hpp:225-236)
            I.ls.t_alpha = 1.0;  // (the full step is what is committed)
            I.f = et[BE_F];
            I.ls.want = Want::Done;
          } else {
            finish(I, ExitStatus::LINE_SEARCH_FAILED);
          }
        }
      }
      bool searching = false;
      for (const auto& I : inst) searching = searching || (I.running && I.ls.want != Want::Done);
      if (!searching) break;
    }
    rep.t_line_search += since(t0);

    // ---- commit ----
    if (launch_for([](const Instance& I) { return I.running && !I.ls.call_feasibility_restoration; })) bd.commit();

    // ---- feasibility restoration on the batch-1 system (sqp.hpp:521-556), one instance at a time ----
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running || !I.ls.call_feasibility_restoration) continue;
      const auto t_fr = clk::now();
      ++out.handoffs;
      Vec x, y, V, s_none, z_none;
      bd.get_instance(b, x, y, V);
      VView cur{st, V};
      const Vec c_e(cur.c_e(), cur.c_e() + m_e), g = cur.g_dense();
      const FilterEntry initial_entry = I.current_entry;
      auto outer_accepts = [&](const FilterEntry& trial_entry, double D_phi_restoration) {
        return I.filter->try_add(initial_entry, trial_entry, D_phi_restoration, I.ls.alpha);
      };
      single.device().set_scaling(I.scales);
      const auto reg = sys.regularization_state();
      single.set_regularization_state({{reg.first[b]}, {reg.second[b]}});
      const ExitStatus fr_status =
          feasibility_restoration_handoff(single, I.scales, outer_accepts, options, x, s_none, y, z_none, options.tolerance / 10.0,
                                          I.iterations, I.rep, solve_start, c_e, Vec{}, g, initial_entry.constraint_violation);
      single.set_gamma_min(1e-10);
      rep.t_restoration += since(t_fr);
      if (fr_status != ExitStatus::SUCCESS) finish(I, fr_status);
      bd.put_instance(b, x, y);
    }

    // ---- AD refresh (sqp.hpp:574-577, newton.hpp:254-255), the error, exits ----
    t0 = clk::now();
    if (launch_for(running)) bd.refresh(err);
    rep.t_ad_refresh += since(t0);
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running) continue;
      take_refresh(I, b);
      ++I.iterations;
      if (I.iterations >= options.max_iterations) finish(I, ExitStatus::MAX_ITERATIONS_EXCEEDED);
    }
    const bool timed_out = since(solve_start) > options.timeout;  // the timeout is the whole batch's
    for (auto& I : inst) {
      if (!I.running) continue;
      if (timed_out) finish(I, ExitStatus::TIMEOUT);
      else if (!(I.E_0 > options.tolerance)) finish(I, ExitStatus::SUCCESS);  // (the loop's condition)
    }
  }

  // ---- results ----
  Vec X, Y;
  bd.get_iterate(X, Y);
  out.status.resize(B);
  out.x.resize(static_cast<size_t>(B) * n);
  out.s.clear();
  out.y.assign(static_cast<size_t>(B) * m_e, 0.0);
  out.z.clear();
  out.cost.resize(B);
  out.iterations.resize(B);
  out.restorations.resize(B);
  const auto& reg_delta = sys.hessian_regularization();
  const auto& reg_gamma = sys.constraint_jacobian_regularization();
  for (int b = 0; b < B; ++b) {
    if (!run[b]) continue;
    const Instance& I = inst[b];
    out.status[b] = I.status;
    std::copy(X.begin() + static_cast<size_t>(b) * n, X.begin() + static_cast<size_t>(b + 1) * n,
              out.x.begin() + static_cast<size_t>(b) * n);
    std::copy(Y.begin() + static_cast<size_t>(b) * m_e, Y.begin() + static_cast<size_t>(b + 1) * m_e,
              out.y.begin() + static_cast<size_t>(b) * m_e);
    out.cost[b] = I.cur.f / I.scales[0];
    out.iterations[b] = I.iterations;
    out.restorations[b] = I.rep.restorations;
    rep.iterations += I.iterations;
    rep.restorations += I.rep.restorations;
    rep.restoration_iterations += I.rep.restoration_iterations;
    rep.final_error = std::max(rep.final_error, I.E_0);
    rep.delta = std::max(rep.delta, reg_delta[b]);
    rep.gamma = std::max(rep.gamma, reg_gamma[b]);
  }
  rep.t_total = since(solve_start);
}

}  // namespace

void sqp_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
               const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out) {
  eq_batch(/*newton=*/false, sys, single, scales, options, x0, run, out);
}

void newton_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
                  const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out) {
  eq_batch(/*newton=*/true, sys, single, scales, options, x0, run, out);
}

}  // namespace slpx
