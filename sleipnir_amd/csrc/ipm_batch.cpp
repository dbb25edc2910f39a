// The batched lockstep driver (ipm_batch.hpp).  Each instance's decisions are ipm_core_host's (ipm.cpp), line for
// line, taken from a few scalars per instance; the vectors stay on the device (BatchIpmDevice) and every piece of
// work runs in one masked launch with the other instances that need it at the same point of their iteration.
#include "ipm_batch.hpp"

#include <cstring>
#include <optional>

#include "ipm_host.hpp"

namespace slpx {

using namespace ipm_host;

namespace {

constexpr double kAlphaReduction = 0.5, kAlphaMin = 1e-7, kTauMin = 0.99;

// where an instance stands in the line search (interior_point.hpp:512-716): the device work it waits for
enum class Phase {
  None,      // not searching
  Eval,      // f, c_e, c_i at the trial point (:512-523)
  SocSolve,  // the second-order correction's solve with the same factorization (:598-640)
  SocEval,   // f, c_e, c_i at the corrected trial point (:641)
  KktEval,   // everything at the full step, for the KKT-error fallback (:691-716)
};

struct Instance {
  bool running = false;
  ExitStatus status = ExitStatus::SUCCESS;
  Vec scales;
  double mu = 0.0, mu_min = 0.0, tau = kTauMin;
  int iterations = 0;
  SolveReport rep;
  std::optional<Filter> filter;
  int full_step_rejected_counter = 0;
  const double* err = nullptr;  // the last refresh's reductions (BatchErr)
  double f = 0.0, violation = 0.0, E_0 = 0.0;
  bool s_from_ci = false;
  // the iteration's direction and line search
  double alpha_max = 1.0, alpha = 1.0, alpha_z = 1.0, D_phi = 0.0;
  FilterEntry current_entry;
  bool call_feasibility_restoration = false;
  Phase phase = Phase::None;
  int t_mode = 0;  // the trial point's direction: 0 Newton, 1 correction
  double t_alpha = 0.0, t_alpha_z = 0.0;
  // second-order corrections (:566-668)
  bool soc_first = false;
  double alpha_soc = 0.0, alpha_z_soc = 0.0, soc_violation = 0.0;
  int soc_it = 0;
};

// util/kkt_error.hpp:92-146 from the reductions of batch_errors_kernel
double scaled_s(double dual_1, double count) { return std::max(100.0, dual_1 / count) / 100.0; }
double error_unscaled(const double* e, int m_e, int m_i) {  // E_0 (:361-362, the un-scaled measure)
  const double s_d = scaled_s(e[BE_YU1] + e[BE_ZU1], double(m_e + m_i)), s_c = scaled_s(e[BE_ZU1], double(m_i));
  return std::max({e[BE_DUALU_INF] / s_d, e[BE_COMPU_INF] / s_c, e[BE_CEU_INF], e[BE_CISU_INF]});
}
double error_mu(const double* e, int m_e, int m_i, double mu) {  // E_mu (:819-832); max |s z - mu| from max, min s z
  const double s_d = scaled_s(e[BE_Y1] + e[BE_Z1], double(m_e + m_i)), s_c = scaled_s(e[BE_Z1], double(m_i));
  const double comp = std::max({0.0, e[BE_SZ_MAX] - mu, mu - e[BE_SZ_MIN]});
  return std::max({e[BE_DUAL_INF] / s_d, comp / s_c, e[BE_CE_INF], e[BE_CIS_INF]});
}
double error_one_norm(const double* e) { return e[BE_DUAL_1] + e[BE_COMP_1] + e[BE_CE_1] + e[BE_CIS_1]; }

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
      bd.alpha[b] = I.t_alpha;
      bd.alpha_z[b] = I.t_alpha_z;
      bd.alpha_soc[b] = I.alpha_soc;
      bd.mode[b] = I.t_mode;
      bd.s_from_ci[b] = I.s_from_ci ? 1 : 0;
      bd.first[b] = I.soc_first ? 1 : 0;
    }
    if (any) bd.upload();
    return any;
  };
  auto running = [](const Instance& I) { return I.running; };
  auto finish = [&](Instance& I, ExitStatus s_) {
    I.status = s_;
    I.running = false;
    I.phase = Phase::None;
  };
  Vec err, dir, met, sd, err_cur, err_trial;
  // the refreshed point's scalars (f, violation, feasible_ipm's choice of s) of instance b
  auto take_refresh = [&](Instance& I, int b) {
    I.err = err.data() + static_cast<size_t>(b) * kBatchErrN;
    I.f = I.err[BE_F];
    I.violation = I.err[BE_CE_1] + I.err[BE_CIS_1];
    I.s_from_ci = options.feasible_ipm && I.err[BE_CI_NONPOS] == 0.0;
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
    if (I.err[BE_V_BAD] != 0.0) {  // :283-286
      finish(I, ExitStatus::NONFINITE_INITIAL_GUESS);
      continue;
    }
    I.mu_min = I.scales[0] * options.tolerance / 10.0;  // :294
    I.filter.emplace(I.violation);                        // :303
    I.E_0 = error_unscaled(I.err, m_e, m_i);              // :361-362
    if (!(I.E_0 > options.tolerance)) finish(I, ExitStatus::SUCCESS);
  }
  rep.t_setup = since(t0);

  auto update_barrier = [](Instance& I) {  // :308-333
    I.mu = std::max(I.mu_min, std::min(0.2 * I.mu, std::pow(I.mu, 1.5)));
    I.tau = std::max(kTauMin, 1.0 - I.mu);
    I.filter->reset();
  };

  // ---- the line search of one instance, between its device rounds (:512-716) ----
  auto request_eval = [&](Instance& I) {
    I.t_mode = 0;
    I.t_alpha = I.alpha;
    I.t_alpha_z = I.alpha_z;
    I.phase = Phase::Eval;
  };
  // what follows a rejected trial point once the corrections (if any) failed (:675-716)
  auto after_rejection = [&](Instance& I) {
    if (I.alpha == I.alpha_max) ++I.full_step_rejected_counter;
    if (I.full_step_rejected_counter >= 4 &&
        I.filter->max_constraint_violation > I.current_entry.constraint_violation / 10.0 &&
        I.filter->last_rejection_due_to_filter()) {  // :677-684
      I.filter->max_constraint_violation *= 0.1;
      I.filter->reset();
      request_eval(I);
      return;
    }
    I.alpha *= kAlphaReduction;
    if (I.alpha < kAlphaMin) {  // :691-716: the full step's KKT error against the current one
      I.t_mode = 0;
      I.t_alpha = I.alpha_max;
      I.t_alpha_z = I.alpha_z;
      I.phase = Phase::KktEval;
      return;
    }
    request_eval(I);
  };
  auto trial_entry_of = [&](const Instance& I, const double* m) {
    return FilterEntry{m[0] - I.mu * m[2], m[1]};
  };
  auto on_eval = [&](Instance& I, const double* m) {  // m = {f, violation, sum ln s, non-finite count}
    if (m[3] != 0.0) {
      I.alpha *= kAlphaReduction;
      if (I.alpha < kAlphaMin) {
        I.call_feasibility_restoration = true;
        I.phase = Phase::None;
        return;
      }
      request_eval(I);
      return;
    }
    if (I.filter->try_add(I.current_entry, trial_entry_of(I, m), I.D_phi, I.alpha)) {
      I.phase = Phase::None;
      return;
    }
    const double next_violation = m[1];
    if (I.alpha == I.alpha_max && next_violation >= I.violation) {  // :566-668
      I.alpha_soc = I.alpha;
      I.soc_violation = next_violation;
      I.soc_it = 0;
      I.soc_first = true;
      I.phase = Phase::SocSolve;
      return;
    }
    after_rejection(I);
  };
  auto on_soc_eval = [&](Instance& I, const double* m) {
    if (I.filter->try_add(I.current_entry, trial_entry_of(I, m), I.D_phi, I.alpha)) {
      I.alpha = I.alpha_soc;
      I.alpha_z = I.alpha_z_soc;
      I.phase = Phase::None;
      return;
    }
    const double next_violation = m[1];
    if (next_violation > 0.99 * I.soc_violation || ++I.soc_it >= 5) {
      after_rejection(I);
      return;
    }
    I.soc_violation = next_violation;
    I.soc_first = false;
    I.phase = Phase::SocSolve;
  };

  while (true) {
    // :387-408 infeasibility / divergence checks, from the last refresh
    for (auto& I : inst) {
      if (!I.running) continue;
      const double* e = I.err;
      if (m_e > 0 && std::sqrt(e[BE_AETCE2]) < 1e-6 && std::sqrt(e[BE_CE2]) > 1e-2) {
        finish(I, ExitStatus::LOCALLY_INFEASIBLE);
        continue;
      }
      if (std::sqrt(e[BE_AITCM2]) < 1e-6 && std::sqrt(e[BE_CM2]) > 1e-6) {
        finish(I, ExitStatus::LOCALLY_INFEASIBLE);
        continue;
      }
      if (e[BE_X_INF] > 1e10 || e[BE_X_BAD] != 0.0 || e[BE_S_INF] > 1e10 || e[BE_S_BAD] != 0.0)
        finish(I, ExitStatus::DIVERGING_ITERATES);
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
      I.alpha_max = dir[3 * b];
      I.alpha = I.alpha_max;
      I.call_feasibility_restoration = I.alpha < kAlphaMin;
      I.alpha_z = dir[3 * b + 1];
      I.D_phi = dir[3 * b + 2];
      I.current_entry = FilterEntry{I.f - I.mu * I.err[BE_LOGSUM], I.violation};
      request_eval(I);
    }

    // ---- the line search in rounds: one masked launch per kind of work still wanted ----
    while (true) {
      if (launch_for([](const Instance& I) { return I.running && I.phase == Phase::SocSolve; })) {
        bd.soc_step(sd);
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          Instance& I = inst[b];
          ++rep.solves;
          I.alpha_soc = sd[2 * b];
          I.alpha_z_soc = sd[2 * b + 1];
          I.t_mode = 1;
          I.t_alpha = I.alpha_soc;
          I.t_alpha_z = I.alpha_z_soc;
          I.phase = Phase::SocEval;
        }
      }
      if (launch_for([](const Instance& I) { return I.running && (I.phase == Phase::Eval || I.phase == Phase::SocEval); })) {
        bd.trial_values(met);
        ++rep.value_sweeps;
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          if (inst[b].phase == Phase::Eval) on_eval(inst[b], met.data() + 4 * b);
          else on_soc_eval(inst[b], met.data() + 4 * b);
        }
      }
      if (launch_for([](const Instance& I) { return I.running && I.phase == Phase::KktEval; })) {
        bd.kkt_fallback(err_cur, err_trial);
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          Instance& I = inst[b];
          const double current_kkt = error_one_norm(err_cur.data() + static_cast<size_t>(b) * kBatchErrN);
          const double next_kkt = error_one_norm(err_trial.data() + static_cast<size_t>(b) * kBatchErrN);
          if (!(next_kkt <= 0.999 * current_kkt)) I.call_feasibility_restoration = true;
          I.phase = Phase::None;
        }
      }
      bool searching = false;
      for (const auto& I : inst) searching = searching || (I.running && I.phase != Phase::None);
      if (!searching) break;
    }
    rep.t_line_search += since(t0);

    // ---- commit (:773-801) ----
    for (auto& I : inst)
      if (I.running && !I.call_feasibility_restoration && I.alpha == I.alpha_max) I.full_step_rejected_counter = 0;
    if (launch_for([](const Instance& I) { return I.running && !I.call_feasibility_restoration; })) bd.commit();

    // ---- feasibility restoration on the batch-1 system (:721-771), one instance at a time ----
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running || !I.call_feasibility_restoration) continue;
      const auto t_fr = clk::now();
      Vec x, s, y, z, V;
      bd.get_instance(b, x, s, y, z, V);
      VView cur{st, V};
      const Vec c_e(cur.c_e(), cur.c_e() + m_e), c_i(cur.c_i(), cur.c_i() + m_i), g = cur.g_dense();
      const FilterEntry initial_entry = I.current_entry;
      auto outer_accepts = [&](const FilterEntry& trial_entry, double D_phi_restoration) {
        return I.filter->try_add(initial_entry, trial_entry, D_phi_restoration, I.alpha);
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
      I.E_0 = error_unscaled(I.err, m_e, m_i);
      if (I.E_0 > options.tolerance) {
        double E_mu = error_mu(I.err, m_e, m_i, I.mu);
        while (I.mu > I.mu_min && E_mu <= 10.0 * I.mu) {
          update_barrier(I);
          E_mu = error_mu(I.err, m_e, m_i, I.mu);
        }
      }
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
    out.cost[b] = I.f / I.scales[0];
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
