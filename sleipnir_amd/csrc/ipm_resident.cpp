// The interior-point iteration (interior_point.hpp:129-878) with the iterate, the step and every O(n) vector RESIDENT
// ON THE DEVICE (ipm_kernels.h): per iteration the host reads the
// inertia counters plus ~30 scalars (step sizes, directional derivative, filter entry of
// the trial point, error norms) and decides; it never sees a vector.  The kernels for the
// step sizes, the first trial point and its merit quantities are enqueued speculatively
// behind the Newton step, so the common iteration has two synchronizations: one after
// [step + first trial], one after [iterate update + AD refresh + error norms].
// Rare branches (the KKT-error fallback of the line search, feasibility restoration, user
// callbacks) pull the iterate to the host and reuse the host code of ipm.cpp and ipm_restoration.cpp.
#include "ipm_drivers.hpp"

#include <cstdio>
#include <cstdlib>

namespace slpx {

namespace {

using namespace ipm_host;
using Want = LineSearch::Want;
using End = LineSearch::End;

// One solve: ipm_core_resident's arguments, the state that lives across its iterations, and the iteration as a sequence
// of phases (run()).  An aggregate, local to this file: the arguments come first, everything else starts as written here.
struct ResidentIpm {
  NewtonSystem& sys;
  const Vec& scales;
  const std::vector<IterationCallback>& callbacks;
  const Options& options;
  const bool in_feasibility_restoration;
  Vec &x, &s, &y, &z;
  double& mu;
  int& iterations;
  SolveReport& rep;
  const clk::time_point solve_start;

  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int n = st.n, m_e = st.m_e, m_i = st.m_i;

  // ---- the solve (mu, iterations: the caller's) ----
  double tau = kTauMin;
  const double mu_min = barrier_floor(scales[0], options.tolerance);
  Filter filter{0.0};  // (begin(): from the initial guess's violation)
  int full_step_rejected_counter = 0;
  LineSearch ls;
  IpmErrOut cur{};  // scalars of the current iterate
  double E_0 = 0.0;
  const bool identity = scaling_is_identity(st, scales);
  const bool lookahead = sys.switches().ipm_lookahead;
  bool pipeline_on = false, ride_on = false;  // (begin())

  // ---- where the truth is ----
  bool host_current = true;       // x, s, y, z on the host mirror the device iterate
  bool ctl_current = false;       // the device's copy of (filter, current iterate's entry, mu) is the host's
  bool filter_on_device = false;  // ... and newer than the host's: the device took decisions since
  double mu_on_device = 0.0;

  // ---- the speculation ----
  // (two sets of the scalar outputs, taken in turn by the iterations: the pipelined common iteration enqueues
  // iteration k+1's launches before the host has read iteration k's)
  int slot = 0;
  bool spec_in_flight = false;  // the NEXT iteration's step and chain are enqueued already (and will run)
  bool spec_rides = false;      // the step enqueued ahead last carries its own verdict (it runs whatever that is)
  long pipelined = 0, passed = 0, twin_launches = 0, twin_taken = 0;
  IpmCtl ctl;  // upload_ctl's scratch

  Vec V;  // host copy for the rare branches

  // What one iteration's Newton step was enqueued as (enqueue_step); const afterwards.
  struct Step {
    clk::time_point started;
    bool s_from_ci;     // the feasible-IPM option takes the trial s from the trial c_i
    bool ahead;         // the chain behind the step computes the whole look-ahead iterate
    bool resumed;       // this iteration's first launch (and chain) were enqueued by the one before
    bool deciding;      // this iteration's chain decides on the device
    bool errors_later;  // ... by an error launch that rides in the next step's launch, or runs on its own
    bool spec = false;  // the next iteration's step is enqueued ahead of this one's verdict
    bool rode = false;  // ... and carries the error launch that decides about it
    FactorInfo info = FactorInfo::Success;
    unsigned long long seq = 0;  // a chain that holds its error launch ends with this publication
  };

  ~ResidentIpm() { release(); }

  const IpmHost& out() const { return dev.ipm_host_slot(slot); }  // where the launches enqueued last leave their scalars

  ExitStatus run();
  ExitStatus begin();
  bool callbacks_stop();
  Step enqueue_step();
  bool await_verdict(const Step& step);
  const IpmDirOut& follow_device(const Step& step);
  void let_pass(const Step& step);
  ExitStatus take_over(const Step& step);
  bool line_search(const Step& step);
  void kkt_error_fallback();
  ExitStatus commit_or_restore(const Step& step, bool took_lookahead);
  ExitStatus restore();
  void refresh_errors(bool took_lookahead);
  ExitStatus end_iteration(double alpha, double alpha_z);
  ExitStatus finish(ExitStatus status);
  void release() noexcept;

  void pull_state() {
    if (host_current) return;
    dev.download(dev.d_x(), x.data(), n);
    if (m_i) {
      dev.download(dev.d_s(), s.data(), m_i);
      dev.download(dev.d_z(), z.data(), m_i);
    }
    if (m_e) dev.download(dev.d_y(), y.data(), m_e);
    host_current = true;
  }
  void push_state() {
    dev.upload_x(x.data());
    dev.upload_duals(s.data(), y.data(), z.data());
    host_current = true;
  }
  void pull_V() {
    V.resize(st.nV);
    dev.download_V(V.data());
  }
  void sync_filter_from_device() {
    if (!filter_on_device) return;
    filter.from_state(dev.ipm_pipeline_fetch().filter);
    filter_on_device = false;
  }
  bool upload_ctl() {
    if (!filter.to_state(ctl.filter)) return false;
    ctl.mu = mu;
    ctl.mu_min = mu_min;
    ctl.tolerance = options.tolerance;
    ctl.cur_f = cur.f;
    ctl.cur_logsum = cur.logsum;
    ctl.cur_viol = cur.viol;
    ctl.m_e = m_e;
    ctl.m_i = m_i;
    ctl.identity_scaling = identity ? 1 : 0;
    dev.ipm_pipeline_upload(ctl);
    ctl_current = true;
    return true;
  }
};

ExitStatus ResidentIpm::run() {
  if (const ExitStatus exit = begin(); exit != ExitStatus::SUCCESS) return finish(exit);
  while (E_0 > options.tolerance) {
    if (const ExitStatus exit = infeasible_or_diverging(cur, m_e, m_i); exit != ExitStatus::SUCCESS) return finish(exit);  // :387-408
    if (!callbacks.empty() && callbacks_stop()) return finish(ExitStatus::CALLBACK_REQUESTED_STOP);

    const Step step = enqueue_step();
    if (await_verdict(step)) {
      const IpmDirOut& taken = follow_device(step);
      if (const ExitStatus exit = end_iteration(taken.alpha_max, taken.alpha_z); exit != ExitStatus::SUCCESS) return finish(exit);
      continue;
    }
    if (step.spec) let_pass(step);
    if (const ExitStatus exit = take_over(step); exit != ExitStatus::SUCCESS) return finish(exit);

    const bool took_lookahead = line_search(step);

    const auto t0 = clk::now();
    if (const ExitStatus exit = commit_or_restore(step, took_lookahead); exit != ExitStatus::SUCCESS) return finish(exit);
    refresh_errors(took_lookahead);
    rep.t_ad_refresh += since(t0);

    if (const ExitStatus exit = end_iteration(ls.alpha, ls.alpha_z); exit != ExitStatus::SUCCESS) return finish(exit);
  }
  rep.final_error = E_0;
  return finish(ExitStatus::SUCCESS);
}

// The initial guess on the device, its sweep and error norms (:245-362); an exit the guess calls for, or SUCCESS.
ExitStatus ResidentIpm::begin() {
  dev.ipm_enable();
  dev.ipm_set_error_scaling(scales);
  release();  // (a system an earlier solve left while unwinding is put right here)

  sys.reset_regularization();
  sys.set_gamma_min(in_feasibility_restoration ? 0.0 : 1e-10);  // :350-352

  auto t_setup = clk::now();
  push_state();
  dev.upload_mu(&mu);
  mu_on_device = mu;
  dev.sweep_full(/*with_reduce=*/false);  // :245-251 (the separable sums ride in the error launch)
  dev.ipm_errors(/*check_all_V=*/true, /*sums_ride=*/true);
  dev.wait_published();
  cur = out().err;

  if (m_e > n) return ExitStatus::TOO_FEW_DOFS;                        // :274
  if (cur.finite == 0.0) return ExitStatus::NONFINITE_INITIAL_GUESS;  // :283-286

  filter = Filter{cur.viol};               // :303
  E_0 = ipm_E_0(cur, m_e, m_i, identity);  // :361-362
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
  pipeline_on = lookahead && callbacks.empty() && !options.feasible_ipm && sys.switches().ipm_pipeline;
  ride_on = pipeline_on && dev.ipm_ride_possible();  // (SLPX_IPM_RIDE=0: the error launch in front of the gated step)
  return ExitStatus::SUCCESS;
}

// The user's callbacks, on the iterate pulled over; true: one of them asked to stop.
bool ResidentIpm::callbacks_stop() {
  pull_state();
  pull_V();
  for (const auto& cb : callbacks)
    if (cb({iterations, x, s, y, z, V, &st, in_feasibility_restoration})) return true;
  push_state();  // a callback may have used this system's device buffers (restoration does)
  return false;
}

// ---- Newton step (:426-482), then speculatively: step sizes, first trial point ---- and, where this iteration's chain
// decides on the device, the next iteration's step ahead of this one's verdict.
ResidentIpm::Step ResidentIpm::enqueue_step() {
  Step k;
  k.started = clk::now();
  k.s_from_ci = options.feasible_ipm && cur.ci_all_pos != 0.0;
  k.ahead = lookahead && !k.s_from_ci;
  if (mu != mu_on_device) {
    dev.upload_mu(&mu);
    mu_on_device = mu;
  }
  k.resumed = spec_in_flight;  // this iteration's first launch (and chain) were enqueued by the one before
  spec_in_flight = false;
  // will THIS iteration's chain decide?  (its state on the device must be the host's, or the device's own)
  k.deciding = pipeline_on && k.ahead && (k.resumed || ctl_current || upload_ctl());
  if (!k.deciding) ctl_current = false;
  if (!k.resumed) dev.build_kkt_for_step(/*with_reduce=*/false);
  // Look-ahead (DeviceNlp::ipm_lookahead): instead of only f, c_e, c_i at the first trial point, the
  // WHOLE next iterate the full step would give — updated s, y, z, the full tape at it, the error norms
  // of :809-832 — is computed speculatively behind the step kernel, in a second set of buffers.  Most
  // iterations take the first trial point: the iteration is then complete when these numbers arrive
  // (one host round trip, four launches), and nothing is computed twice.  The feasible-IPM option
  // derives the trial s from the trial c_i (:520-526): it keeps the trial-values chain below.
  // (the error launch of a deciding chain comes LATER: riding in the next step's launch — it decides whether that
  // step counts while the step factors — or on its own where no step is enqueued ahead)
  k.errors_later = k.deciding && ride_on;
  sys.set_after_attempt([this, &k] {
    if (k.ahead) {
      dev.ipm_lookahead(tau);
      dev.sweep_full_lookahead();
      if (k.errors_later) {
      } else if (k.deciding) dev.ipm_errors_deciding(/*sums_ride=*/true);
      else dev.ipm_errors(false, /*sums_ride=*/true, /*ahead=*/true);
    } else {
      dev.ipm_direction(tau);
      dev.sweep_values_trial();
      dev.ipm_trial_metrics(-1.0, k.s_from_ci);
    }
  });
  // (twin attempts, NewtonSystem::compute_twin: the look-ahead launch takes the direction of whichever of a
  // launch's two attempts the regularization policy takes — the other after_attempt chain does not)
  sys.set_twin_attempts(k.ahead);
  k.info = sys.compute(/*solve_speculatively=*/true)[0];
  twin_launches += sys.last_twin_launches();
  twin_taken += sys.last_twin_taken();
  // ---- the next iteration's step, ahead of this one's verdict ----
  if (k.deciding && k.info == FactorInfo::Success && iterations + 2 < options.max_iterations) {
    dev.ipm_accept_lookahead();  // (the roles the buffers have if the device takes the step; put back in let_pass if not)
    dev.ipm_set_slot(slot ^ 1);
    // (the chain of the step enqueued ahead decides too: the device's state is its own by then)
    if (k.errors_later) k.rode = dev.ipm_ride_errors_in_next_step(slot);
    k.spec = sys.begin_speculative_compute(/*gated=*/!k.rode);
    if (!k.spec) {
      k.rode = false;
      dev.ipm_accept_lookahead();
      dev.ipm_set_slot(slot);
    }
    spec_rides = k.rode;
  }
  if (k.errors_later && !k.rode) {
    if (k.spec) throw std::logic_error("slpx: a step enqueued ahead of its own verdict");
    dev.ipm_errors_deciding(/*sums_ride=*/true);  // (nothing was enqueued ahead: the error launch on its own)
  }
  k.seq = dev.seq_expected();
  sys.set_twin_attempts(false);
  sys.set_after_attempt(nullptr);
  return k;
}

// The wait for this iteration's scalars, by the riding launch's verdict or by sequence number; true: the device took
// the iteration's decisions, and the step enqueued ahead counts.
bool ResidentIpm::await_verdict(const Step& step) {
  if (step.rode) return dev.ipm_ride_wait(slot);  // (the riding launch's scalars are in when its verdict is)
  dev.wait_published_until(step.seq);  // compute() returns when the inertia counters are in; the trial chain may still run
  return step.spec && out().go != 0.0;
}

// the device took this iteration's decisions (ipm_decide.h): the filter accepted the full step, the
// error is above the tolerance, mu stays; the next step is on its way.  The host follows.  Returns the step sizes taken.
const IpmDirOut& ResidentIpm::follow_device(const Step& step) {
  ++pipelined;
  rep.factorizations += sys.last_factorizations();
  rep.solves += sys.last_factorizations();
  rep.value_sweeps += sys.last_factorizations();
  rep.t_kkt_decomp += since(step.started);
  rep.delta = sys.hessian_regularization()[0];
  rep.gamma = sys.constraint_jacobian_regularization()[0];
  full_step_rejected_counter = 0;
  host_current = false;
  filter_on_device = true;
  const IpmHost& decided = out();
  cur = decided.err_ahead;
  slot ^= 1;
  spec_in_flight = true;
  return decided.dir;
}

// the host has to look: what was enqueued ahead passes (a gated step at once; a step that carried its own verdict
// runs and holds its results back, the chain behind it passes) — as if it had never been launched.  No waiting for
// any of it: what the host enqueues next runs behind it in the stream's order, and it writes nothing the host or a
// later launch reads but its sequence numbers.
void ResidentIpm::let_pass(const Step& step) {
  ++passed;
  sys.cancel_speculative_compute(/*launch_ran=*/step.rode);  // (a step that carried its own verdict ran, and held its results back)
  dev.ipm_accept_lookahead();
  dev.ipm_set_slot(slot);
}

// The host decides this iteration: the filter back from the device, the step booked; FACTORIZATION_FAILED, or SUCCESS.
ExitStatus ResidentIpm::take_over(const Step& step) {
  ctl_current = false;  // (whatever happens below changes the filter, the iterate or mu on the host's side)
  sync_filter_from_device();
  rep.factorizations += sys.last_factorizations();
  rep.solves += sys.last_factorizations();
  rep.value_sweeps += sys.last_factorizations();
  rep.t_kkt_decomp += since(step.started);
  if (step.info != FactorInfo::Success) return ExitStatus::FACTORIZATION_FAILED;  // :463-465
  rep.delta = sys.hessian_regularization()[0];
  rep.gamma = sys.constraint_jacobian_regularization()[0];
  return ExitStatus::SUCCESS;
}

// The filter line search (:488-716) on the scalars the chains leave; true: the filter took the complete look-ahead iterate.
bool ResidentIpm::line_search(const Step& step) {
  const auto t0 = clk::now();
  const IpmHost& H = out();
  const FilterEntry current_entry{cur.f - mu * cur.logsum, cur.viol};
  ls.start(filter, full_step_rejected_counter, mu, current_entry, H.dir.alpha_max, H.dir.alpha_z, H.dir.D_phi);  // :488-509
  bool have_trial = true;       // the speculative chain already evaluated alpha_max
  bool took_lookahead = false;  // ... as the complete look-ahead iterate, and the filter took it

  while (ls.want != Want::Done) switch (ls.want) {
    case Want::Eval: {
      const bool from_ahead = have_trial && step.ahead;
      if (!have_trial) {
        dev.ipm_trial_point(ls.t_alpha);
        dev.sweep_values_trial();
        dev.ipm_trial_metrics(ls.t_alpha, step.s_from_ci);
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
      dev.ipm_soc_accumulate(ls.alpha_soc, ls.soc_first, ls.soc_first && step.s_from_ci);
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
    case Want::KktEval: kkt_error_fallback(); break;
    default: break;
  }
  rep.t_line_search += since(t0);
  return took_lookahead;
}

// :691-716 — rare: on the host, with the iterate pulled over
void ResidentIpm::kkt_error_fallback() {
  pull_state();
  pull_V();
  VView cv{st, V};
  const Vec g = cv.g_dense();
  const double current_kkt = kkt_error_impl<ErrType::ONE_NORM>(st, g, cv.Ae(), cv.c_e(), cv.Ai(), cv.c_i(), s, y, z, mu, nullptr);
  Vec p_x, p_y, p_s, p_z;
  download_direction(dev, n, m_e, m_i, p_x, p_y, p_s, p_z);
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
}

// The iterate update (:775-801) on the device — or, where the line search asked for it, feasibility restoration
// (:721-771); an exit restoration ends in, or SUCCESS.
ExitStatus ResidentIpm::commit_or_restore(const Step& step, bool took_lookahead) {
  if (ls.call_feasibility_restoration) return restore();
  if (took_lookahead) {
    dev.ipm_accept_lookahead();  // :775-801 happened in ipm_lookahead_kernel; the buffers change roles
  } else {  // :775-801; the feasible-IPM choice of s holds for a trial point along the Newton direction only
    dev.ipm_commit(ls.end == End::Fallback ? ls.alpha_max : ls.alpha, ls.alpha_z, step.s_from_ci && ls.end == End::Newton);
  }
  host_current = false;
  return ExitStatus::SUCCESS;
}

// :721-771 — rare: host vectors, as in ipm_core_host
ExitStatus ResidentIpm::restore() {
  if (in_feasibility_restoration) return ExitStatus::FEASIBILITY_RESTORATION_FAILED;
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
    return filter.try_add(initial_entry, trial_entry, D_phi_restoration, ls.alpha);
  };
  const ExitStatus fr_status = feasibility_restoration(sys, scales, callbacks, outer_accepts, options, x, s, y, z, mu, iterations,
                                                       rep, solve_start, c_e, c_i, g, initial_entry.constraint_violation);
  if (fr_status != ExitStatus::SUCCESS) return fr_status;
  push_state();
  return ExitStatus::SUCCESS;
}

// AD refresh (:809-812) and every norm the next decisions need
void ResidentIpm::refresh_errors(bool took_lookahead) {
  if (took_lookahead && !ls.call_feasibility_restoration) {
    cur = out().err_ahead;  // already there: the look-ahead chain swept and reduced this iterate
  } else {
    dev.sweep_full(/*with_reduce=*/false);
    dev.ipm_errors(false, /*sums_ride=*/true);
    dev.wait_published();
    cur = out().err;
  }
}

// The tail of every iteration, followed or decided here: the error of the new iterate, the barrier update (:819-832),
// the diagnostics line, the count and the exit tests; MAX_ITERATIONS_EXCEEDED, TIMEOUT, or SUCCESS to go on.
ExitStatus ResidentIpm::end_iteration(double alpha, double alpha_z) {
  const bool followed = spec_in_flight;  // (a step is enqueued ahead exactly where the device took this iteration)
  E_0 = ipm_E_0(cur, m_e, m_i, identity);
  // A followed iteration makes no barrier update: the device only takes the step when none is due (ipm_decide.h:
  // ipm_next_iteration_is_plain), and mu, tau and the filter's table are the device's to keep until the host looks.
  if (!followed && E_0 > options.tolerance)  // :819-832
    update_barrier_parameter(mu, mu_min, tau, filter, [&](double m) { return ipm_E_mu(cur, m, m_e, m_i); });
  if (options.diagnostics) print_iteration(iterations, E_0, cur.f, cur.viol, mu, rep, alpha, alpha_z, sys.last_factorizations());
  ++iterations;
  rep.final_error = E_0;
  // A followed iteration tests the timeout alone: its step was enqueued ahead under iterations + 2 < max_iterations
  // (enqueue_step), so the count cannot have reached the cap here.
  if (!followed && iterations >= options.max_iterations) return ExitStatus::MAX_ITERATIONS_EXCEEDED;
  if (since(solve_start) > options.timeout) return ExitStatus::TIMEOUT;
  return ExitStatus::SUCCESS;
}

// Every exit of run(): what can fail first — the wait for a step enqueued ahead (it runs for nothing), the iterate to
// the host, the SLPX_TWIN_VERBOSE lines —, with the machinery put back (release) as soon as that step is through.
ExitStatus ResidentIpm::finish(ExitStatus status) {
  if (spec_in_flight) dev.wait_published();  // (the step enqueued ahead runs for nothing: wait for it, forget it)
  release();
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
  return status;
}

// The speculative machinery of the NewtonSystem and its device, back as a solve finds it: no step enqueued ahead, no
// riding or gated launch armed, output slot 0, no chain behind an attempt, one attempt per launch.  Host state only,
// so it cannot fail: at entry, on every exit, and — from the destructor — when an exception unwinds the solve.
void ResidentIpm::release() noexcept {
  if (sys.speculative_compute_pending()) sys.cancel_speculative_compute(/*launch_ran=*/spec_rides);
  spec_in_flight = false;
  dev.ipm_ride_disarm();
  dev.ipm_gate_next_step(false);
  dev.ipm_set_slot(slot = 0);
  sys.set_after_attempt(nullptr);
  sys.set_twin_attempts(false);
}

}  // namespace

ExitStatus ipm_core_resident(NewtonSystem& sys, const Vec& scales, const std::vector<IterationCallback>& callbacks,
                             const Options& options, bool in_feasibility_restoration, Vec& x, Vec& s, Vec& y, Vec& z, double& mu,
                             int& iterations, SolveReport& rep, clk::time_point solve_start) {
  return ResidentIpm{sys, scales, callbacks, options, in_feasibility_restoration, x, s, y, z, mu, iterations, rep, solve_start}.run();
}

}  // namespace slpx
