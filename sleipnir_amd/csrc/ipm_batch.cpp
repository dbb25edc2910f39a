// The batched lockstep driver (ipm_batch.hpp).  Each instance's decisions are taken by the code the single-problem
// drivers run (ipm_line_search.hpp: the line search machine, the barrier update, the exits; ipm_decide.h: the error
// measures), from a few scalars per instance; the vectors stay on the device (BatchIpmDevice) and every piece of
// work runs in one masked launch with the other instances that need it at the same point of their iteration.
#include "ipm_batch.hpp"

#include <cstring>
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
  double mu = 0.0, mu_min = 0.0, tau = kTauMin;
  int iterations = 0;
  SolveReport rep;
  std::optional<Filter> filter;
  int full_step_rejected_counter = 0;
  IpmErrOut cur{};  // the last refresh's reductions
  double E_0 = 0.0;
  bool s_from_ci = false;
  FilterEntry current_entry;
  LineSearch ls;  // where the instance stands in its line search: the device work it waits for
};

}  // namespace

void interior_point_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales,
                          const Options& options, const std::vector<double>& x0, const std::vector<uint8_t>& run,
                          BatchSolveResult& out) {
  const auto solve_start = clk::now();
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int B = sys.batch(), n = st.n, m_e = st.m_e, m_i = st.m_i, ns = st.n_scales();
  if (static_cast<int>(x0.size()) != B * n || static_cast<int>(scales.size()) != B * ns || static_cast<int>(run.size()) != B)
    throw std::runtime_error("interior_point_batch: wrong lengths");
  if (m_i == 0) throw std::runtime_error("interior_point_batch: a problem with inequality constraints only");
  SolveReport& rep = out.report;
  out.driver = 1;
  out.rounds = out.handoffs = 0;

  BatchIpmDevice bd(sys);
  bd.set_scales(scales);
  sys.reset_regularization();
  sys.set_gamma_min(1e-10);  // :350-352

  std::vector<Instance> inst(B);
  for (int b = 0; b < B; ++b) {
    Instance& I = inst[b];
    I.scales.assign(scales.begin() + static_cast<size_t>(b) * ns, scales.begin() + static_cast<size_t>(b + 1) * ns);
    I.mu = 0.1 * I.scales[0];  // interior_point.hpp:74-79
    I.running = run[b] != 0;
  }
  bd.set_iterate(x0, Vec(static_cast<size_t>(B) * m_i, 1.0), Vec(static_cast<size_t>(B) * m_e, 0.0),
                 Vec(static_cast<size_t>(B) * m_i, 1.0));

  // the per-instance parameters of the next launches, for the instances `pred` selects
  auto launch_for = [&](auto pred) {
    bool any = false;
    for (int b = 0; b < B; ++b) {
      const Instance& I = inst[b];
      bd.active[b] = pred(I) ? 1 : 0;
      any = any || bd.active[b];
      bd.mu[b] = I.mu;
      bd.tau[b] = I.tau;
      bd.alpha[b] = I.ls.t_alpha;
      bd.alpha_z[b] = I.ls.t_alpha_z;
      bd.alpha_soc[b] = I.ls.alpha_soc;
      bd.mode[b] = I.ls.on_correction ? 1 : 0;
      bd.s_from_ci[b] = I.s_from_ci ? 1 : 0;
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
  Vec err, dir, met, sd, err_cur, err_trial;
  // the refreshed point's scalars (f, violation, feasible_ipm's choice of s) of instance b
  auto take_refresh = [&](Instance& I, int b) {
    I.cur = err_of(err.data() + static_cast<size_t>(b) * kBatchErrN);
    I.s_from_ci = options.feasible_ipm && I.cur.ci_all_pos != 0.0;
    I.E_0 = ipm_E_0(I.cur, m_e, m_i, /*identity_scaling=*/false);  // (a problem with inequality rows is always scaled)
  };

  // ---- setup (:245-362) ----
  auto t0 = clk::now();
  if (launch_for(running)) bd.refresh(err);
  for (int b = 0; b < B; ++b) {
    Instance& I = inst[b];
    if (!I.running) continue;
    take_refresh(I, b);
    if (m_e > n) {  // :274
      finish(I, ExitStatus::TOO_FEW_DOFS);
      continue;
    }
    if (err[static_cast<size_t>(b) * kBatchErrN + BE_V_BAD] != 0.0) {  // :283-286
      finish(I, ExitStatus::NONFINITE_INITIAL_GUESS);
      continue;
    }
    I.mu_min = barrier_floor(I.scales[0], options.tolerance);
    I.filter.emplace(I.cur.viol);  // :303
    if (!(I.E_0 > options.tolerance)) finish(I, ExitStatus::SUCCESS);
  }
  rep.t_setup = since(t0);

  while (true) {
    // :387-408 infeasibility / divergence checks, from the last refresh
    for (auto& I : inst) {
      if (!I.running) continue;
      const ExitStatus exit = infeasible_or_diverging(I.cur, m_e, m_i);
      if (exit != ExitStatus::SUCCESS) finish(I, exit);
    }
    if (!launch_for(running)) break;

    // ---- Newton step of every running instance (:426-482): the system's s, y, z, V are the last refresh's ----
    t0 = clk::now();
    dev.upload_mu(bd.mu.data());
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
    bd.newton_direction(dir);  // alpha_max, alpha_z, D_phi (:488-509)
    rep.t_kkt_solve += since(t0);

    t0 = clk::now();
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running) continue;
      if (info[b] != FactorInfo::Success) {  // :463-465
        finish(I, ExitStatus::FACTORIZATION_FAILED);
        continue;
      }
      I.current_entry = FilterEntry{I.cur.f - I.mu * I.cur.logsum, I.cur.viol};
      I.ls.start(*I.filter, I.full_step_rejected_counter, I.mu, I.current_entry, dir[3 * b], dir[3 * b + 1], dir[3 * b + 2]);
    }

    // ---- the line search in rounds: one masked launch per kind of work still wanted ----
    while (true) {
      if (launch_for([](const Instance& I) { return I.running && I.ls.want == Want::SocSolve; })) {
        bd.soc_step(sd);
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          ++rep.solves;
          inst[b].ls.on_soc_solve(sd[2 * b], sd[2 * b + 1]);
        }
      }
      if (launch_for([](const Instance& I) { return I.running && (I.ls.want == Want::Eval || I.ls.want == Want::SocEval); })) {
        bd.trial_values(met);
        ++rep.value_sweeps;
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          const double* m = met.data() + 4 * b;  // f, violation, sum ln s, non-finite count
          inst[b].ls.on_trial(IpmTrialOut{m[0], m[1], m[2], m[3] == 0.0 ? 1.0 : 0.0});
        }
      }
      if (launch_for([](const Instance& I) { return I.running && I.ls.want == Want::KktEval; })) {
        bd.kkt_fallback(err_cur, err_trial);
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          inst[b].ls.on_kkt_errors(error_one_norm(err_cur.data() + static_cast<size_t>(b) * kBatchErrN),
                                   error_one_norm(err_trial.data() + static_cast<size_t>(b) * kBatchErrN));
        }
      }
      bool searching = false;
      for (const auto& I : inst) searching = searching || (I.running && I.ls.want != Want::Done);
      if (!searching) break;
    }
    rep.t_line_search += since(t0);

    // ---- commit (:773-801) ----
    if (launch_for([](const Instance& I) { return I.running && !I.ls.call_feasibility_restoration; })) bd.commit();

    // ---- feasibility restoration on the batch-1 system (:721-771), one instance at a time ----
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running || !I.ls.call_feasibility_restoration) continue;
      const auto t_fr = clk::now();
      ++out.handoffs;
      Vec x, s, y, z, V;
      bd.get_instance(b, x, s, y, z, V);
      VView cur{st, V};
      const Vec c_e(cur.c_e(), cur.c_e() + m_e), c_i(cur.c_i(), cur.c_i() + m_i), g = cur.g_dense();
      const FilterEntry initial_entry = I.current_entry;
      auto outer_accepts = [&](const FilterEntry& trial_entry, double D_phi_restoration) {
        return I.filter->try_add(initial_entry, trial_entry, D_phi_restoration, I.ls.alpha);
      };
      single.device().set_scaling(I.scales);
      const auto reg = sys.regularization_state();
      single.set_regularization_state({{reg.first[b]}, {reg.second[b]}});
      const ExitStatus fr_status = feasibility_restoration_handoff(single, I.scales, outer_accepts, options, x, s, y, z, I.mu,
                                                                   I.iterations, I.rep, solve_start, c_e, c_i, g,
                                                                   initial_entry.constraint_violation);
      rep.t_restoration += since(t_fr);
      if (fr_status != ExitStatus::SUCCESS) finish(I, fr_status);
      bd.put_instance(b, x, s, y, z);
    }

    // ---- AD refresh (:809-812), errors and barrier update (:814-832), exits (:834-878) ----
    t0 = clk::now();
    if (launch_for(running)) bd.refresh(err);
    rep.t_ad_refresh += since(t0);
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running) continue;
      take_refresh(I, b);
      if (I.E_0 > options.tolerance)
        update_barrier_parameter(I.mu, I.mu_min, I.tau, *I.filter, [&](double mu) { return ipm_E_mu(I.cur, mu, m_e, m_i); });
      ++I.iterations;
      if (I.iterations >= options.max_iterations) finish(I, ExitStatus::MAX_ITERATIONS_EXCEEDED);
    }
    const bool timed_out = since(solve_start) > options.timeout;  // the timeout is the whole batch's
    for (auto& I : inst) {
      if (!I.running) continue;
      if (timed_out) finish(I, ExitStatus::TIMEOUT);
      else if (!(I.E_0 > options.tolerance)) finish(I, ExitStatus::SUCCESS);  // (the loop's condition, :383)
    }
  }

  // ---- results ----
  Vec X, S, Y, Z;
  bd.get_iterate(X, S, Y, Z);
  out.status.resize(B);
  out.x.resize(static_cast<size_t>(B) * n);
  out.s.assign(static_cast<size_t>(B) * m_i, 0.0);
  out.y.assign(static_cast<size_t>(B) * m_e, 0.0);
  out.z.assign(static_cast<size_t>(B) * m_i, 0.0);
  out.cost.resize(B);
  out.iterations.resize(B);
  out.restorations.resize(B);
  const auto& reg_delta = sys.hessian_regularization();
  const auto& reg_gamma = sys.constraint_jacobian_regularization();
  for (int b = 0; b < B; ++b) {
    if (!run[b]) continue;
    const Instance& I = inst[b];
    auto copy = [&](const Vec& src, Vec& dst, int len) {
      std::copy(src.begin() + static_cast<size_t>(b) * len, src.begin() + static_cast<size_t>(b + 1) * len,
                dst.begin() + static_cast<size_t>(b) * len);
    };
    out.status[b] = I.status;
    copy(X, out.x, n);
    copy(S, out.s, m_i);
    copy(Y, out.y, m_e);
    copy(Z, out.z, m_i);
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

}  // namespace slpx
