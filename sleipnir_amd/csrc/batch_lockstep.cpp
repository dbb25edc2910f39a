// The batched lockstep loop (batch_lockstep.hpp) and its three drivers.  Each instance's decisions are taken by the
// code the single-problem drivers run (ipm_line_search.hpp: the line search machines, the barrier update, the exits;
// ipm_decide.h: the error measures), from a few scalars per instance; the vectors stay on the device and every piece
// of work runs in one masked launch with the other instances that need it at the same point of their iteration.
// The loop is written once; a driver says what its iteration does differently from the others, and nothing more.
#include <memory>
#include <optional>

#include "eq_batch.hpp"
#include "fr_batch.hpp"
#include "ipm_batch.hpp"
#include "ipm_line_search.hpp"
#include "warm_start.h"

namespace slpx {

using namespace ipm_host;

namespace {

using Want = LineSearch::Want;

struct Instance {
  bool running = false;
  ExitStatus status = ExitStatus::SUCCESS;
  Vec scales;
  bool identity = false;                            // SQP, Newton: problem_scaling.hpp:111-113
  double mu = 0.0, mu_min = 0.0, tau = kTauMin;     // interior point
  int iterations = 0;
  SolveReport rep;
  std::optional<Filter> filter;
  int full_step_rejected_counter = 0;
  IpmErrOut cur{};  // the last refresh's reductions
  double E_0 = 0.0;
  bool s_from_ci = false;  // interior point
  FilterEntry current_entry;
  LineSearch ls;        // where the instance stands in its line search: the device work it waits for
  NewtonSearch newton;  // the same for Newton's own search
};

// ---- interior point (interior_point.hpp:129-878; a problem with inequality rows is always scaled) ----
struct IpmDriver {
  static constexpr const char* kName = "interior_point_batch";
  static constexpr const char* kModels = "a problem with inequality constraints only";
  static constexpr int kId = 1;
  static bool takes(const NlpStructure& st) { return st.m_i > 0; }
  using Device = BatchIpmDevice;

  const NlpStructure& st;
  const Options& options;
  Vec dir, sd;

  template <class I>
  static auto& search(I& inst) { return inst.ls; }
  static constexpr bool kWarmStarts = true;
  void set_initial_iterate(Device& bd, const Vec& x0) const {
    const size_t B = bd.B;
    bd.set_iterate(x0, Vec(B * st.m_i, 1.0), Vec(B * st.m_e, 0.0), Vec(B * st.m_i, 1.0));
  }
  void init(Instance& I) const { I.mu = 0.1 * I.scales[0]; }  // interior_point.hpp:74-79
  void init_warm(Instance& I, double mu) const { I.mu = mu; }
  void setup(Instance& I) const { I.mu_min = barrier_floor(I.scales[0], options.tolerance); }
  void launch_parameters(Device& bd, int b, const Instance& I) const {
    bd.mu[b] = I.mu;
    bd.tau[b] = I.tau;
    bd.alpha[b] = I.ls.t_alpha;
    bd.alpha_z[b] = I.ls.t_alpha_z;
    bd.s_from_ci[b] = I.s_from_ci ? 1 : 0;
  }
  // the refreshed point's choice of s (feasible_ipm) and its error
  void after_refresh(Instance& I) const {
    I.s_from_ci = options.feasible_ipm && I.cur.ci_all_pos != 0.0;
    I.E_0 = ipm_E_0(I.cur, st.m_e, st.m_i, /*identity_scaling=*/false);
  }
  void update_barrier(Instance& I) const {  // :814-832
    if (I.E_0 > options.tolerance)
      update_barrier_parameter(I.mu, I.mu_min, I.tau, *I.filter, [&](double mu) { return ipm_E_mu(I.cur, mu, st.m_e, st.m_i); });
  }
  const double* step_mu(const Device& bd) const { return bd.mu.data(); }
  void direction(Device& bd) { bd.newton_direction(dir); }  // alpha_max, alpha_z, D_phi (:488-509)
  void start_search(Instance& I, int b) const {
    I.current_entry = FilterEntry{I.cur.f - I.mu * I.cur.logsum, I.cur.viol};
    I.ls.start(*I.filter, I.full_step_rejected_counter, I.mu, I.current_entry, dir[3 * b], dir[3 * b + 1], dir[3 * b + 2]);
  }
  void soc_step(Device& bd) { bd.soc_step(sd); }
  void on_soc_solve(Instance& I, int b) const { I.ls.on_soc_solve(sd[2 * b], sd[2 * b + 1]); }
  void on_trial(Instance& I, int b, const Vec& met) const {
    const double* m = met.data() + 4 * b;  // f, violation, sum ln s, non-finite count
    I.ls.on_trial(IpmTrialOut{m[0], m[1], m[2], m[3] == 0.0 ? 1.0 : 0.0});
  }
  void on_kkt_errors(Instance& I, const double* ec, const double* et) const {
    I.ls.on_kkt_errors(error_one_norm(ec), error_one_norm(et));
  }
  double restoration_mu(const Instance& I) const { return I.mu; }
  void after_restoration(NewtonSystem&) const {}
};

// ---- what SQP and Newton share: no inequality rows, no barrier ----
struct EqDriver {
  using Device = BatchEqDevice;
  const NlpStructure& st;
  const Options& options;
  Vec dphi, mu0;

  void init(Instance& I) const { I.identity = scaling_is_identity(st, I.scales); }
  void init_warm(Instance&, double) const {}  // (no barrier)
  void after_refresh(Instance& I) const {
    // (m_i = 0, and for Newton m_e = 0 too: the divisors of the scale factors are 0, the quotients NaN, and fmax
    // drops a NaN as std::max does one in its second argument: both factors are 1, as on the host)
    I.E_0 = ipm_E_0(I.cur, st.m_e, 0, I.identity);
  }
  void update_barrier(Instance&) const {}
  const double* step_mu(const Device& bd) {
    mu0.assign(bd.B, 0.0);
    return mu0.data();
  }
  void direction(Device& bd) { bd.direction(dphi); }  // D_phi; alpha_max = alpha_z = 1
};

// ---- SQP (sqp.hpp:98-604, as sqp_core of sqp_newton.cpp restates it) ----
struct SqpDriver : EqDriver {
  static constexpr const char* kName = "sqp_batch";
  static constexpr const char* kModels = "a problem with equality constraints and no inequality constraints only";
  static constexpr int kId = 2;
  static bool takes(const NlpStructure& st) { return st.m_i == 0 && st.m_e > 0; }

  template <class I>
  static auto& search(I& inst) { return inst.ls; }
  static constexpr bool kWarmStarts = true;  // x and y
  void set_initial_iterate(Device& bd, const Vec& x0) const {
    bd.set_iterate(x0, Vec(static_cast<size_t>(bd.B) * st.m_e, 0.0));  // problem.hpp:503-504: y = 0
  }
  void setup(Instance&) const {}
  void launch_parameters(Device& bd, int b, const Instance& I) const { bd.alpha[b] = I.ls.t_alpha; }
  // the interior-point line search with alpha_max = 1 and no barrier term; y moves with the primal step
  void start_search(Instance& I, int b) const {
    I.current_entry = FilterEntry{I.cur.f, I.cur.viol};
    I.ls.start(*I.filter, I.full_step_rejected_counter, 0.0, I.current_entry, 1.0, 1.0, dphi[b]);
  }
  void soc_step(Device& bd) const { bd.soc_step(); }
  void on_soc_solve(Instance& I, int) const { I.ls.on_soc_solve(I.ls.alpha_max, I.ls.alpha_max); }  // a correction keeps the full step
  void on_trial(Instance& I, int b, const Vec& met) const {
    const double* m = met.data() + 3 * b;  // f, ||c_e||_1, non-finite count
    I.ls.on_trial(IpmTrialOut{m[0], m[1], 0.0, m[2] == 0.0 ? 1.0 : 0.0});
  }
  void on_kkt_errors(Instance& I, const double* ec, const double* et) const {
    I.ls.on_kkt_errors(error_one_norm(ec), error_one_norm(et));
  }
  double restoration_mu(const Instance&) const { return options.tolerance / 10.0; }  // sqp.hpp:521-556
  void after_restoration(NewtonSystem& single) const { single.set_gamma_min(1e-10); }
};

// ---- Newton (newton.hpp:51-292, as newton_core of sqp_newton.cpp restates it): its own search, never a correction or a restoration ----
struct NewtonDriver : EqDriver {
  static constexpr const char* kName = "newton_batch";
  static constexpr const char* kModels = "a problem without constraints only";
  static constexpr int kId = 3;
  static bool takes(const NlpStructure& st) { return st.m_e == 0 && st.m_i == 0; }

  template <class I>
  static auto& search(I& inst) { return inst.newton; }
  static constexpr bool kWarmStarts = false;  // x only: the other blocks are accepted and ignored
  void set_initial_iterate(Device& bd, const Vec& x0) const { bd.set_iterate(x0, Vec{}); }
  void setup(Instance& I) const { I.newton.f = I.cur.f; }
  // the fallback looks at the full step (newton.hpp:226); every other trial point is at t_alpha
  void launch_parameters(Device& bd, int b, const Instance& I) const {
    bd.alpha[b] = I.newton.want == Want::KktEval ? NewtonSearch::alpha_max : I.newton.t_alpha;
  }
  // the cost the filter compares is the accepted trial point's (newton.hpp:246-247), not the refresh's
  void start_search(Instance& I, int b) const { I.newton.start(*I.filter, dphi[b]); }
  void soc_step(Device&) const {}
  void on_soc_solve(Instance&, int) const {}
  void on_trial(Instance& I, int b, const Vec& met) const {
    const double* m = met.data() + 3 * b;  // f, -, non-finite count
    I.newton.on_trial(m[0], m[2] == 0.0);
  }
  void on_kkt_errors(Instance& I, const double* ec, const double* et) const {  // ||g||_1 (newton.hpp:225-236)
    I.newton.on_kkt_errors(error_one_norm(ec), error_one_norm(et), et[BE_F]);
  }
  double restoration_mu(const Instance&) const { return 0.0; }
  void after_restoration(NewtonSystem&) const {}
};

template <class Driver>
void lockstep(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
              const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out, int restoration_mode,
              const std::vector<double>* instance_params, const BatchWarmStart* warm) {
  const auto solve_start = clk::now();
  const NlpStructure& st = sys.structure();
  DeviceNlp& dev = sys.device();
  const int B = sys.batch(), n = st.n, m_e = st.m_e, m_i = st.m_i, ns = st.n_scales();
  const std::string name = Driver::kName;
  if (static_cast<int>(x0.size()) != B * n || static_cast<int>(scales.size()) != B * ns || static_cast<int>(run.size()) != B)
    throw std::runtime_error(name + ": wrong lengths");
  if (!Driver::takes(st)) throw std::runtime_error(name + ": " + Driver::kModels);
  // per-instance parameters: row b of instance_params
  const size_t n_p = instance_params ? st.parameter_nodes().size() : 0;
  if (instance_params && (n_p == 0 || instance_params->size() != static_cast<size_t>(B) * n_p))
    throw std::runtime_error(name + ": wrong length of the per-instance parameters");
  auto params_of = [&](int b) {
    return n_p ? Vec(instance_params->begin() + static_cast<size_t>(b) * n_p, instance_params->begin() + static_cast<size_t>(b + 1) * n_p) : Vec{};
  };
  SolveReport& rep = out.report;
  out.driver = Driver::kId;
  out.rounds = out.handoffs = 0;
  std::fill(out.restoration_lockstep, out.restoration_lockstep + 4, int64_t{0});
  if (restoration_mode != 0 && restoration_mode != 1) throw std::runtime_error(name + ": restoration mode must be 0 (hand-off) or 1 (lockstep)");

  Driver drv{st, options};
  typename Driver::Device bd(sys);
  std::unique_ptr<BatchFrDevice> frd;  // restoration in lockstep: made when a phase is first entered
  bd.set_scales(scales);
  sys.reset_regularization();
  sys.set_gamma_min(1e-10);  // interior_point.hpp:350-352, sparse_regularized_ldlt.hpp:197

  std::vector<Instance> inst(B);
  for (int b = 0; b < B; ++b) {
    Instance& I = inst[b];
    I.scales.assign(scales.begin() + static_cast<size_t>(b) * ns, scales.begin() + static_cast<size_t>(b + 1) * ns);
    drv.init(I);
    I.running = run[b] != 0;
  }
  drv.set_initial_iterate(bd, x0);
  // A warm start (warm_start.h) in place of the constants, for the instances that run and whose input is finite — the
  // others keep the cold start: s, y, z converted and safeguarded on the device, the first barrier parameter from it
  if (warm) out.repaired.assign(B, 0);
  // (nothing given beside x0 — no block, and no barrier parameter above 0 — is the cold start, as in a single solve)
  bool warm_given = warm && (warm->s || warm->y || warm->z);
  for (int b = 0; warm && warm->mu && !warm_given && b < B; ++b) warm_given = !(warm->mu[b] <= 0.0);
  if (Driver::kWarmStarts && warm_given) {
    BatchWarmStart ws = *warm;
    if (m_i == 0) ws.s = ws.z = ws.mu = nullptr;  // SQP: x and y
    Vec mu_min(B), first;
    for (int b = 0; b < B; ++b) mu_min[b] = barrier_floor(inst[b].scales[0], options.tolerance);
    bd.warm_start(ws, run, mu_min, first);
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running) continue;
      const double* w = first.data() + static_cast<size_t>(b) * 3;
      if (w[2] != 0.0) {
        I.status = ExitStatus::NONFINITE_INITIAL_GUESS;
        I.running = false;
        Driver::search(I).want = Want::Done;
        continue;
      }
      drv.init_warm(I, w[0]);
      out.repaired[b] = static_cast<int>(w[1]);
    }
  }

  // the per-instance parameters of the next launches, for the instances `pred` selects
  auto launch_for = [&](auto pred) {
    bool any = false;
    for (int b = 0; b < B; ++b) {
      const Instance& I = inst[b];
      bd.active[b] = pred(I) ? 1 : 0;
      any = any || bd.active[b];
      bd.alpha_soc[b] = I.ls.alpha_soc;
      bd.mode[b] = I.ls.on_correction ? 1 : 0;
      bd.first[b] = I.ls.soc_first ? 1 : 0;
      drv.launch_parameters(bd, b, I);
    }
    if (any) bd.upload();
    return any;
  };
  auto running = [](const Instance& I) { return I.running; };
  auto wants = [](const Instance& I, Want w) { return I.running && Driver::search(I).want == w; };
  auto restores = [](const Instance& I) { return Driver::search(I).call_feasibility_restoration; };
  auto finish = [&](Instance& I, ExitStatus s_) {
    I.status = s_;
    I.running = false;
    Driver::search(I).want = Want::Done;
  };
  // (only Newton's search can end with nothing to do next; the filter line search hands over to restoration)
  auto answered = [&](Instance& I) {
    if (Driver::search(I).failed) finish(I, ExitStatus::LINE_SEARCH_FAILED);
  };
  Vec err, met, err_cur, err_trial;
  // the refreshed point's scalars of instance b
  auto take_refresh = [&](Instance& I, int b) {
    I.cur = err_of(err.data() + static_cast<size_t>(b) * kBatchErrN);
    drv.after_refresh(I);
  };

  // ---- setup (interior_point.hpp:245-362, sqp.hpp:182-254, newton.hpp:108-150) ----
  auto t0 = clk::now();
  if (launch_for(running)) bd.refresh(err);
  for (int b = 0; b < B; ++b) {
    Instance& I = inst[b];
    if (!I.running) continue;
    take_refresh(I, b);
    if (m_e > n) {  // interior_point.hpp:274, sqp.hpp:205-210
      finish(I, ExitStatus::TOO_FEW_DOFS);
      continue;
    }
    if (err[static_cast<size_t>(b) * kBatchErrN + BE_V_BAD] != 0.0) {  // :283-286, sqp.hpp:213-216, newton.hpp:125-127
      finish(I, ExitStatus::NONFINITE_INITIAL_GUESS);
      continue;
    }
    drv.setup(I);
    I.filter.emplace(I.cur.viol);  // :303, sqp.hpp:220 (||c_e||_1), newton.hpp:131 (0)
    if (!(I.E_0 > options.tolerance)) finish(I, ExitStatus::SUCCESS);
  }
  rep.t_setup = since(t0);

  while (true) {
    // infeasibility (where there are rows) / divergence, from the last refresh (:387-408, sqp.hpp:277-292, newton.hpp:164)
    for (auto& I : inst) {
      if (!I.running) continue;
      const ExitStatus exit = infeasible_or_diverging(I.cur, m_e, m_i);
      if (exit != ExitStatus::SUCCESS) finish(I, exit);
    }
    if (!launch_for(running)) break;

    // ---- Newton step of every running instance (:426-482, sqp.hpp:305-346, newton.hpp:182-190): the system's
    // s, y, z, V are the last refresh's ----
    t0 = clk::now();
    dev.upload_mu(drv.step_mu(bd));
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
    drv.direction(bd);
    rep.t_kkt_solve += since(t0);

    t0 = clk::now();
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running) continue;
      if (info[b] != FactorInfo::Success) {  // :463-465, sqp.hpp:336-338
        finish(I, ExitStatus::FACTORIZATION_FAILED);
        continue;
      }
      drv.start_search(I, b);
    }

    // ---- the line search in rounds: one masked launch per kind of work still wanted ----
    while (true) {
      if (launch_for([&](const Instance& I) { return wants(I, Want::SocSolve); })) {
        drv.soc_step(bd);
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          ++rep.solves;
          drv.on_soc_solve(inst[b], b);
        }
      }
      if (launch_for([&](const Instance& I) { return wants(I, Want::Eval) || wants(I, Want::SocEval); })) {
        bd.trial_values(met);
        ++rep.value_sweeps;
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          drv.on_trial(inst[b], b, met);
          answered(inst[b]);
        }
      }
      if (launch_for([&](const Instance& I) { return wants(I, Want::KktEval); })) {
        bd.kkt_fallback(err_cur, err_trial);
        for (int b = 0; b < B; ++b) {
          if (!bd.active[b]) continue;
          drv.on_kkt_errors(inst[b], err_cur.data() + static_cast<size_t>(b) * kBatchErrN,
                            err_trial.data() + static_cast<size_t>(b) * kBatchErrN);
          answered(inst[b]);
        }
      }
      bool searching = false;
      for (const auto& I : inst) searching = searching || (I.running && Driver::search(I).want != Want::Done);
      if (!searching) break;
    }
    rep.t_line_search += since(t0);

    // ---- commit (:773-801) ----
    if (launch_for([&](const Instance& I) { return I.running && !restores(I); })) bd.commit();

    // ---- feasibility restoration in lockstep (restoration_mode 1): everybody who asked in this round enters ONE
    // restoration phase on the batch system (fr_batch.hpp); the others wait ----
    if (restoration_mode == 1) {
      std::vector<BatchRestorationRequest> requests;
      for (int b = 0; b < B; ++b) {
        Instance& I = inst[b];
        if (!I.running || !restores(I)) continue;
        BatchRestorationRequest r;
        r.b = b;
        r.scales = I.scales;
        r.params = params_of(b);
        r.mu = drv.restoration_mu(I);
        Vec V;
        bd.get_instance(b, r.x, r.s, r.y, r.z, V);
        VView cur{st, V};
        r.c_e.assign(cur.c_e(), cur.c_e() + m_e);
        r.c_i.assign(cur.c_i(), cur.c_i() + m_i);
        r.g = cur.g_dense();
        const FilterEntry initial_entry = I.current_entry;
        r.initial_violation = initial_entry.constraint_violation;
        Instance* ip = &I;
        r.outer_accepts = [ip, initial_entry](const FilterEntry& trial_entry, double D_phi_restoration) {
          return ip->filter->try_add(initial_entry, trial_entry, D_phi_restoration, Driver::search(*ip).alpha);
        };
        r.iterations = &I.iterations;
        r.rep = &I.rep;
        requests.push_back(std::move(r));
      }
      if (!requests.empty()) {
        const auto t_fr = clk::now();
        if (!frd) frd = std::make_unique<BatchFrDevice>(sys);
        BatchRestorationStats fs;
        restoration_phase(sys, single, *frd, options, requests, /*stop_after=*/-1, solve_start, fs);
        out.restoration_lockstep[0] += fs.instances;
        out.restoration_lockstep[1] += fs.phases;
        out.restoration_lockstep[2] += fs.rounds;
        out.restoration_lockstep[3] += fs.fallbacks;
        drv.after_restoration(single);
        rep.t_restoration += since(t_fr);
        for (BatchRestorationRequest& r : requests) {
          if (r.status != ExitStatus::SUCCESS) finish(inst[r.b], r.status);
          bd.put_instance(r.b, r.x, r.s, r.y, r.z);
        }
      }
    }

    // ---- feasibility restoration on the batch-1 system (:721-771, sqp.hpp:521-556), one instance at a time ----
    for (int b = 0; b < B && restoration_mode == 0; ++b) {
      Instance& I = inst[b];
      if (!I.running || !restores(I)) continue;
      const auto t_fr = clk::now();
      ++out.handoffs;
      Vec x, s, y, z, V;
      bd.get_instance(b, x, s, y, z, V);
      VView cur{st, V};
      const Vec c_e(cur.c_e(), cur.c_e() + m_e), c_i(cur.c_i(), cur.c_i() + m_i), g = cur.g_dense();
      const FilterEntry initial_entry = I.current_entry;
      auto outer_accepts = [&](const FilterEntry& trial_entry, double D_phi_restoration) {
        return I.filter->try_add(initial_entry, trial_entry, D_phi_restoration, Driver::search(I).alpha);
      };
      single.device().set_scaling(I.scales);
      if (n_p) single.device().set_parameters(params_of(b).data(), /*per_instance=*/false);
      const auto reg = sys.regularization_state();
      single.set_regularization_state({{reg.first[b]}, {reg.second[b]}});
      const ExitStatus fr_status = feasibility_restoration_handoff(single, I.scales, outer_accepts, options, x, s, y, z,
                                                                   drv.restoration_mu(I), I.iterations, I.rep, solve_start, c_e,
                                                                   c_i, g, initial_entry.constraint_violation);
      drv.after_restoration(single);
      rep.t_restoration += since(t_fr);
      if (fr_status != ExitStatus::SUCCESS) finish(I, fr_status);
      bd.put_instance(b, x, s, y, z);
    }

    // ---- AD refresh (:809-812, sqp.hpp:574-577, newton.hpp:254-255), errors and barrier update, exits (:834-878) ----
    t0 = clk::now();
    if (launch_for(running)) bd.refresh(err);
    rep.t_ad_refresh += since(t0);
    for (int b = 0; b < B; ++b) {
      Instance& I = inst[b];
      if (!I.running) continue;
      take_refresh(I, b);
      drv.update_barrier(I);
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
  if (warm) {  // the end iterate in the user's units (warm_start.h): what the next warm start takes
    bd.unscaled_iterate(run, out.s_u, out.y_u, out.z_u);
    out.mu_u.assign(B, 0.0);
    for (int b = 0; b < B; ++b)
      if (run[b]) out.mu_u[b] = warm_unscale_mu(inst[b].mu, inst[b].scales[0]);
  }
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

}  // namespace

void interior_point_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales,
                          const Options& options, const std::vector<double>& x0, const std::vector<uint8_t>& run,
                          BatchSolveResult& out, int restoration_mode, const std::vector<double>* instance_params,
                          const BatchWarmStart* warm) {
  lockstep<IpmDriver>(sys, single, scales, options, x0, run, out, restoration_mode, instance_params, warm);
}

void sqp_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
               const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out, int restoration_mode,
               const std::vector<double>* instance_params, const BatchWarmStart* warm) {
  lockstep<SqpDriver>(sys, single, scales, options, x0, run, out, restoration_mode, instance_params, warm);
}

void newton_batch(NewtonSystem& sys, NewtonSystem& single, const std::vector<double>& scales, const Options& options,
                  const std::vector<double>& x0, const std::vector<uint8_t>& run, BatchSolveResult& out,
                  const std::vector<double>* instance_params, const BatchWarmStart* warm) {
  lockstep<NewtonDriver>(sys, single, scales, options, x0, run, out, /*restoration_mode=*/0, instance_params, warm);
}

}  // namespace slpx
