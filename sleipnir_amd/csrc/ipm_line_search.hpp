// The decisions every solver driver shares, host only, on scalars: the filter line search of
// interior_point.hpp:512-716 as ONE resumable state machine, and around it the barrier update (:308-333), the
// infeasibility / divergence exits (:387-408) and the diagnostics line.  The error measures are ipm_E_mu / ipm_E_0
// of ipm_decide.h — the ones the device decides the common iteration with.
//
// The machine says which device work it waits for (`want`, at `t_alpha`, `t_alpha_z`, along the Newton direction or
// the correction's) and is resumed with a handful of scalars.  A sequential driver (host: ipm.cpp; device-resident:
// ipm_resident.cpp; restoration: ipm_restoration.cpp; SQP: sqp_newton.cpp) runs it with
// `while (ls.want != Done) switch (ls.want)`; the batched loop (batch_lockstep.cpp)
// keeps one per instance and answers all instances that want the same work with one masked launch.  What a driver
// keeps for itself is plumbing: where the four numbers of a trial point come from, and what to commit.
#pragma once

#include <cstdio>

#include "ipm.hpp"
#include "ipm_host.hpp"

namespace slpx::ipm_host {

constexpr double kAlphaReduction = 0.5;  // alpha_reduction_factor
constexpr double kAlphaMin = 1e-7;       // the step floor of the filter line search
constexpr double kNewtonAlphaMin = 1e-20;  // the step floor of Newton's search (newton.hpp:138-139)
constexpr double kTauMin = 0.99;         // fraction to the boundary
constexpr double kKappaSoc = 0.99;       // a correction round must take 1 % off the violation to be followed by another
constexpr int kMaxCorrections = 5;
constexpr double kFallbackDecrease = 0.999;  // the KKT-error fallback's test on the full step

class LineSearch {
 public:
  enum class Want { Eval, SocSolve, SocEval, KktEval, Done };
  // how the search ended: at `alpha` along the Newton direction, by a correction (alpha, alpha_z are the corrected
  // direction's), by the fallback (the full step alpha_max; alpha stays the halved one), or with nothing accepted
  enum class End { None, Newton, Correction, Fallback };

  Want want = Want::Done;
  End end = End::None;
  // restoration wanted.  Set from the start where alpha_max is below the floor (:489-491): the search still runs,
  // as the reference's does, and whatever it accepts is not committed.
  bool call_feasibility_restoration = false;
  static constexpr bool failed = false;  // (a search that accepts nothing asks for restoration; NewtonSearch can fail)
  double alpha_max = 1.0, alpha = 1.0, alpha_z = 1.0;

  // the request: Eval / SocEval = f, violation, sum ln s at (t_alpha, t_alpha_z) along the Newton direction or
  // the correction's; SocSolve = a correction solve (the first of its rounds or not) accumulating with alpha_soc,
  // answered with the corrected direction's step sizes; KktEval = the one-norm KKT error here and at the full step
  bool on_correction = false;
  double t_alpha = 0.0, t_alpha_z = 0.0;
  bool soc_first = false;
  double alpha_soc = 0.0, alpha_z_soc = 0.0;

  // `filter` and `full_step_rejected_counter` are the driver's: they live across iterations.  A driver that moves
  // y with the primal step (SQP) reads `alpha` alone, and answers a correction solve with the full step.
  void start(Filter& filter, int& full_step_rejected_counter, double mu, const FilterEntry& current_entry, double alpha_max_,
             double alpha_z_, double D_phi) {
    m_filter = &filter;
    m_counter = &full_step_rejected_counter;
    m_mu = mu;
    m_current = current_entry;
    m_D_phi = D_phi;
    alpha_max = alpha = alpha_max_;
    alpha_z = alpha_z_;
    end = End::None;
    call_feasibility_restoration = alpha < kAlphaMin;
    request_eval();
  }

  void on_trial(const IpmTrialOut& tr) {  // answers Eval and SocEval
    const FilterEntry trial_entry{tr.f - m_mu * tr.logsum, tr.viol};
    if (want == Want::SocEval) {  // :636-657
      if (m_filter->try_add(m_current, trial_entry, m_D_phi, alpha)) {
        alpha = alpha_soc;
        alpha_z = alpha_z_soc;
        return finish(End::Correction);
      }
      if (tr.viol > kKappaSoc * m_soc_violation || ++m_soc_round >= kMaxCorrections) return after_rejection();
      m_soc_violation = tr.viol;
      soc_first = false;
      want = Want::SocSolve;
      return;
    }
    if (tr.finite == 0.0) {  // :532-542
      alpha *= kAlphaReduction;
      if (alpha < kAlphaMin) {
        call_feasibility_restoration = true;
        want = Want::Done;
        return;
      }
      return request_eval();
    }
    if (m_filter->try_add(m_current, trial_entry, m_D_phi, alpha)) return finish(End::Newton);
    if (alpha == alpha_max && tr.viol >= m_current.constraint_violation) {  // :561-571
      alpha_soc = alpha;
      m_soc_violation = tr.viol;
      m_soc_round = 0;
      soc_first = true;
      want = Want::SocSolve;
      return;
    }
    after_rejection();
  }

  void on_soc_solve(double alpha_soc_, double alpha_z_soc_) {  // :623-624
    alpha_soc = alpha_soc_;
    alpha_z_soc = alpha_z_soc_;
    on_correction = true;
    t_alpha = alpha_soc;
    t_alpha_z = alpha_z_soc;
    want = Want::SocEval;
  }

  void on_kkt_errors(double current_kkt_error, double next_kkt_error) {  // :709-715
    if (next_kkt_error <= kFallbackDecrease * current_kkt_error) return finish(End::Fallback);
    call_feasibility_restoration = true;
    want = Want::Done;
  }

 private:
  Filter* m_filter = nullptr;
  int* m_counter = nullptr;
  double m_mu = 0.0, m_D_phi = 0.0, m_soc_violation = 0.0;
  FilterEntry m_current;
  int m_soc_round = 0;

  void request_eval() {
    on_correction = false;
    t_alpha = alpha;
    t_alpha_z = alpha_z;
    want = Want::Eval;
  }
  // the step is taken unless restoration was wanted from the start; a full step ends the run of rejected ones (:773)
  void finish(End how) {
    end = how;
    want = Want::Done;
    if (!call_feasibility_restoration && alpha == alpha_max) *m_counter = 0;
  }
  // what follows a rejected trial point once the corrections (if any) failed (:666-716)
  void after_rejection() {
    if (alpha == alpha_max) ++*m_counter;
    if (*m_counter >= 4 && m_filter->max_constraint_violation > m_current.constraint_violation / 10.0 &&
        m_filter->last_rejection_due_to_filter()) {  // :677-684
      m_filter->max_constraint_violation *= 0.1;
      m_filter->reset();
      return request_eval();
    }
    alpha *= kAlphaReduction;
    if (alpha < kAlphaMin) {  // :691-706: the full step's KKT error against the current one
      on_correction = false;
      t_alpha = alpha_max;
      t_alpha_z = alpha_z;
      want = Want::KktEval;
      return;
    }
    request_eval();
  }
};

// Newton's own search (newton.hpp:201-243) as the same kind of machine: no corrections, no restoration to fall back
// on, a floor of 1e-20, entries without a constraint violation.  Eval asks for the cost at `t_alpha` along the
// Newton direction and whether it is finite; past the floor KktEval asks for ||g||_1 here and at the full step
// `alpha_max`, and for the cost there.  It ends (Done) accepted — `t_alpha` is the step to commit, `f` the cost the
// filter compares the next search's trial points with — or `failed`: LINE_SEARCH_FAILED.
class NewtonSearch {
 public:
  using Want = LineSearch::Want;
  static constexpr double alpha_max = 1.0;
  static constexpr bool call_feasibility_restoration = false;

  Want want = Want::Done;
  bool failed = false;
  double f = 0.0;
  double alpha = alpha_max;  // halved with every rejection; stays the halved one where the fallback accepts
  double t_alpha = alpha_max;

  void start(Filter& filter, double D_phi) {  // (`f` is the caller's to set before the first search)
    m_filter = &filter;
    m_D_phi = D_phi;
    alpha = t_alpha = alpha_max;
    failed = false;
    want = Want::Eval;
  }

  void on_trial(double trial_f, bool finite) {
    if (finite && m_filter->try_add(FilterEntry{f, 0.0}, FilterEntry{trial_f, 0.0}, m_D_phi, alpha)) {
      f = trial_f;
      want = Want::Done;
      return;
    }
    alpha *= kAlphaReduction;
    t_alpha = alpha;
    if (alpha < kNewtonAlphaMin) {
      if (finite) want = Want::KktEval;  // :225-236: the full step's ||g||_1 against the current one
      else fail();                       // (a non-finite cost has no fallback, :208-214)
    }
  }

  void on_kkt_errors(double current_kkt_error, double next_kkt_error, double f_at_full_step) {
    if (!(next_kkt_error <= kFallbackDecrease * current_kkt_error)) return fail();
    t_alpha = alpha_max;  // (the full step is what is committed)
    f = f_at_full_step;
    want = Want::Done;
  }

 private:
  Filter* m_filter = nullptr;
  double m_D_phi = 0.0;
  void fail() {
    failed = true;
    want = Want::Done;
  }
};

// ---- the scalar decisions around the line search ----

inline double barrier_floor(double cost_scale, double tolerance) { return cost_scale * tolerance / 10.0; }  // mu_min (:294)

// :819-832 with :308-333: the barrier parameter goes down while the barrier problem is solved to within 10 mu.
// E_mu_at(mu): the scaled error measure at the current iterate.
template <class ErrorAt>
void update_barrier_parameter(double& mu, double mu_min, double& tau, Filter& filter, ErrorAt&& E_mu_at) {
  double E_mu = E_mu_at(mu);
  while (mu > mu_min && E_mu <= 10.0 * mu) {
    mu = std::max(mu_min, std::min(0.2 * mu, std::pow(mu, 1.5)));
    tau = std::max(kTauMin, 1.0 - mu);
    filter.reset();
    E_mu = E_mu_at(mu);
  }
}

// :387-408 on the reduced scalars: the exit the iterate calls for, or SUCCESS for none.  (The device's copy of
// these tests, ipm_next_iteration_is_plain in ipm_decide.h, stays as it is: it answers "nothing rare", not which.)
inline ExitStatus infeasible_or_diverging(const IpmErrOut& e, int m_e, int m_i) {
  if (m_e > 0 && std::sqrt(e.aetce_sq) < 1e-6 && std::sqrt(e.ce_sq) > 1e-2) return ExitStatus::LOCALLY_INFEASIBLE;
  if (m_i > 0 && std::sqrt(e.aitcp_sq) < 1e-6 && std::sqrt(e.cp_sq) > 1e-6) return ExitStatus::LOCALLY_INFEASIBLE;
  if (e.x_inf > 1e10 || e.s_inf > 1e10 || e.finite == 0.0) return ExitStatus::DIVERGING_ITERATES;
  return ExitStatus::SUCCESS;
}

// one line per iteration (print_iteration_diagnostics.hpp, condensed); tag: "", "  (restoration)", "  (sqp)", ...
inline void print_iteration(int iteration, double E_0, double f, double violation, double mu, const SolveReport& rep,
                            double alpha, double alpha_z, int factorizations, const char* tag = "") {
  std::fprintf(stderr,
               "%4d  err %.3e  f %.6e  |c| %.3e  mu %.1e  delta %.3e  gamma %.3e  alpha %.2e  alpha_z %.2e  nfact %d%s\n",
               iteration, E_0, f, violation, mu, rep.delta, rep.gamma, alpha, alpha_z, factorizations, tag);
}

}  // namespace slpx::ipm_host
