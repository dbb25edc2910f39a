// The restoration phase of the batched lockstep loop (fr_batch.hpp): restoration_core() and feasibility_restoration()
// of ipm_restoration.cpp for every instance that asked for restoration in one round of the outer loop, in lockstep.  Each
// instance's decisions are the single path's — LineSearch, Filter, the barrier update and the exits of
// ipm_line_search.hpp, the error measures of ipm_decide.h, LdltPolicy — on its own scalars; the vectors stay on the
// device (BatchFrDevice) and every piece of work is one masked launch for the instances that want it.  What differs
// from the single path is what it does to save round trips and nothing else: no twin attempts and no look-ahead chain
// (the first trial point of a step is a trial point like the others).  Two rare pieces stay per instance on the batch-1
// system: the KKT-error fallback of a line search and the multiplier estimate at exit.
#include <cstring>
#include <optional>

#include "fr_batch.hpp"
#include "ipm_line_search.hpp"

namespace slpx {

using namespace ipm_host;

namespace {

using Want = LineSearch::Want;
using End = LineSearch::End;

struct FrInstance {
  BatchRestorationRequest* req = nullptr;
  bool running = false;
  ExitStatus core = ExitStatus::SUCCESS;  // what restoration_core() returns
  RestorationEntry entry;
  double mu = 0.0, mu_min = 0.0, tau = kTauMin, delta = 0.0, E_0 = 0.0;
  std::optional<Filter> filter;
  int full_step_rejected_counter = 0, it_before = 0;
  LineSearch ls;
  FrErrOut cur{};
};

}  // namespace

void restoration_phase(NewtonSystem& sys, NewtonSystem& single, BatchFrDevice& frd, const Options& options,
                       std::vector<BatchRestorationRequest>& requests, int stop_after, clk::time_point solve_start,
                       BatchRestorationStats& stats) {
  if (requests.empty()) return;
  const NlpStructure& st = sys.structure();
  const int B = sys.batch(), n = st.n, m_e = st.m_e, m_i = st.m_i, M = 2 * m_e + 2 * m_i, dim = n + m_e, mi_ext = m_i + M;
  const int ns = st.n_scales();
  ++stats.phases;
  stats.instances += static_cast<int64_t>(requests.size());

  // ---- entry (feasibility_restoration.hpp:391-432), per instance on the host ----
  std::vector<FrInstance> inst(B);
  std::vector<double> scales(static_cast<size_t>(B) * ns, 1.0);
  const NewtonSystem::RegularizationState saved_regularization = sys.regularization_state();
  NewtonSystem::RegularizationState reg = saved_regularization;
  for (BatchRestorationRequest& r : requests) {
    if (r.b < 0 || r.b >= B || inst[r.b].req) throw std::runtime_error("restoration_phase: bad instance");
    FrInstance& I = inst[r.b];
    I.req = &r;
    I.running = true;
    ++r.rep->restorations;
    I.it_before = *r.iterations;
    I.entry = restoration_entry(st, r.scales, r.x, r.s, r.mu, r.c_e, r.c_i);
    I.mu = I.entry.fr_mu;
    std::copy(r.scales.begin(), r.scales.end(), scales.begin() + static_cast<size_t>(r.b) * ns);
    const RestorationEntry& e = I.entry;
    frd.begin(r.b, e.X.data(), e.S.data(), e.y.data(), e.Z.data(), e.x_r.data(), e.w.data(), r.g.data(), r.s.data(), e.X.data() + n,
              e.S.data() + m_i, e.Z.data() + m_i);
    frd.mu_outer[r.b] = r.mu;
    reg.first[r.b] = reg.second[r.b] = 0.0;  // (restoration_core: reset_regularization)
  }
  frd.set_scales(scales);
  sys.set_regularization_state(reg);
  sys.set_gamma_min(0.0);  // :350-352

  // the launch parameters every kernel reads, for the instances `pred` selects
  auto select = [&](auto pred) {
    bool any = false;
    for (int b = 0; b < B; ++b) {
      const FrInstance& I = inst[b];
      frd.active[b] = I.req && pred(I) ? 1 : 0;
      any = any || frd.active[b];
      frd.mu[b] = I.mu;
      frd.tau[b] = I.tau;
      frd.delta[b] = I.delta;
      frd.soc[b] = frd.rhs_only[b] = frd.first[b] = 0;
    }
    return any;
  };
  auto running = [](const FrInstance& I) { return I.running; };
  auto finish = [](FrInstance& I, ExitStatus s) {
    I.core = s;
    I.running = false;
    I.ls.want = Want::Done;
  };
  Vec err, dir, met;
  auto take_errors = [&](FrInstance& I, int b) {
    std::memcpy(&I.cur, err.data() + static_cast<size_t>(b) * kFrBatchErrN, sizeof(FrErrOut));
    I.E_0 = ipm_E_0(I.cur.e, m_e, mi_ext, /*identity_scaling=*/false);
  };
  auto trial_of = [&](int b) { return IpmTrialOut{met[4 * b], met[4 * b + 1], met[4 * b + 2], met[4 * b + 3]}; };

  // ---- setup (restoration_core: :245-362 on the restoration problem) ----
  select(running);
  frd.upload();
  frd.sweep();
  frd.errors(/*check_all_V=*/true, err);
  for (int b = 0; b < B; ++b) {
    FrInstance& I = inst[b];
    if (!I.running) continue;
    take_errors(I, b);
    if (I.cur.e.finite == 0.0) {  // :283-286
      finish(I, ExitStatus::NONFINITE_INITIAL_GUESS);
      continue;
    }
    I.mu_min = barrier_floor(1.0, options.tolerance);  // (the restoration cost is not scaled)
    I.filter.emplace(I.cur.e.viol);                    // :303
  }

  while (true) {
    // ---- the loop's condition and the exits in front of a step ----
    for (int b = 0; b < B; ++b) {
      FrInstance& I = inst[b];
      if (!I.running) continue;
      const BatchRestorationRequest& r = *I.req;
      if (!(I.E_0 > options.tolerance)) {
        finish(I, ExitStatus::SUCCESS);
        continue;
      }
      if (const ExitStatus exit = infeasible_or_diverging(I.cur.e, m_e, mi_ext); exit != ExitStatus::SUCCESS) {  // :387-408
        finish(I, exit);
        continue;
      }
      if (stop_after >= 0 && *r.iterations - I.it_before >= stop_after) {
        finish(I, ExitStatus::CALLBACK_REQUESTED_STOP);
        continue;
      }
      // the callback the reference appends (interior_point.hpp:729-752): leave once the OUTER filter accepts the
      // restoration iterate and the violation dropped by 10 %
      const FilterEntry trial_entry{I.cur.f_outer - r.mu * I.cur.logsum_outer, I.cur.viol_outer};
      if (trial_entry.constraint_violation < 0.9 * r.initial_violation && r.outer_accepts(trial_entry, I.cur.dphi_outer))
        finish(I, ExitStatus::CALLBACK_REQUESTED_STOP);
    }
    std::vector<uint8_t> mask(B, 0);
    std::vector<double> eliminated(B, std::numeric_limits<double>::infinity());
    bool any = false;
    for (int b = 0; b < B; ++b)
      if (inst[b].running) {
        mask[b] = 1;
        eliminated[b] = inst[b].cur.eliminated_min_pivot;
        any = true;
      }
    if (!any) break;

    // ---- Newton step (:426-482) on the reduced systems: the regularization policy per instance, the build in front of
    // every attempt ----
    const std::vector<FactorInfo> info = sys.compute_hooked_batch(
        [&](const std::vector<double>& d, const std::vector<double>&, const std::vector<uint8_t>& a) {
          select([](const FrInstance&) { return true; });
          for (int b = 0; b < B; ++b) {
            frd.active[b] = a[b];
            frd.delta[b] = d[b];
          }
          frd.upload();
          frd.build();
        },
        mask, eliminated);
    ++stats.rounds;
    for (int b = 0; b < B; ++b) {
      FrInstance& I = inst[b];
      if (!I.running) continue;
      I.req->rep->factorizations += sys.last_factorizations();
      I.req->rep->solves += 1;
      if (info[b] != FactorInfo::Success) {  // :463-465
        finish(I, ExitStatus::FACTORIZATION_FAILED);
        continue;
      }
      I.delta = sys.hessian_regularization()[b];
    }
    if (select(running)) {
      frd.upload();
      frd.expand(dir);
    }
    for (int b = 0; b < B; ++b) {
      FrInstance& I = inst[b];
      if (!I.running) continue;
      const FilterEntry current_entry{I.cur.e.f - I.mu * I.cur.e.logsum, I.cur.e.viol};
      I.ls.start(*I.filter, I.full_step_rejected_counter, I.mu, current_entry, dir[4 * b], dir[4 * b + 1], dir[4 * b + 2]);  // :488-509
    }

    // ---- the line search in rounds (a step below the floor fails the phase at once: there is no restoration to call
    // from here) ----
    auto wants = [](const FrInstance& I, Want w) { return I.running && !I.ls.call_feasibility_restoration && I.ls.want == w; };
    while (true) {
      // second-order corrections (:601-633): new right-hand side, SAME factorization
      if (select([&](const FrInstance& I) { return wants(I, Want::SocSolve) && I.ls.soc_first; })) {
        frd.upload();
        frd.save_direction();
      }
      if (select([&](const FrInstance& I) { return wants(I, Want::SocSolve); })) {
        const std::vector<uint8_t> group = frd.active;
        for (int b = 0; b < B; ++b) {
          frd.alpha_soc[b] = inst[b].ls.alpha_soc;
          frd.first[b] = inst[b].ls.soc_first ? 1 : 0;
          frd.soc[b] = frd.rhs_only[b] = 1;
        }
        frd.upload();
        frd.soc_accumulate();
        frd.build();
        sys.device().solve();  // (every instance's factors; the slices of the others are not read)
        frd.expand(dir);
        for (int b = 0; b < B; ++b) frd.alpha[b] = dir[4 * b];
        frd.upload();
        frd.trial_values(met, /*after_expand=*/true);
        for (int b = 0; b < B; ++b) {
          if (!group[b]) continue;
          FrInstance& I = inst[b];
          ++I.req->rep->solves;
          ++I.req->rep->value_sweeps;
          I.ls.on_soc_solve(dir[4 * b], dir[4 * b + 1]);
          I.ls.on_trial(trial_of(b));
        }
        // the corrections failed: back to the Newton direction
        bool back = false;
        for (int b = 0; b < B; ++b) {
          frd.active[b] = group[b] && !inst[b].ls.on_correction ? 1 : 0;
          back = back || frd.active[b];
        }
        if (back) {
          frd.upload();
          frd.restore_direction();
        }
      }
      if (select([&](const FrInstance& I) { return wants(I, Want::Eval); })) {
        const std::vector<uint8_t> group = frd.active;
        for (int b = 0; b < B; ++b) frd.alpha[b] = inst[b].ls.t_alpha;
        frd.upload();
        frd.trial_values(met);
        for (int b = 0; b < B; ++b) {
          if (!group[b]) continue;
          ++inst[b].req->rep->value_sweeps;
          inst[b].ls.on_trial(trial_of(b));
        }
      }
      // the KKT-error fallback (:691-716) — rare: on the host and the batch-1 system, one instance at a time
      for (int b = 0; b < B; ++b) {
        FrInstance& I = inst[b];
        if (!wants(I, Want::KktEval)) continue;
        ++stats.fallbacks;
        const double alpha_max = I.ls.t_alpha, alpha_z = I.ls.t_alpha_z;
        Vec X(n + M), S(mi_ext), y(m_e), Z(mi_ext), Vo(st.nV), Vt(st.nV);
        frd.download_instance(b, X.data(), S.data(), y.data(), Z.data(), X.data() + n, S.data() + m_i, Z.data() + m_i);
        frd.download_V(b, Vo.data());
        const double current_kkt = restoration_kkt_error(st, Vo, X, S, y, Z, I.entry.x_r, I.entry.w, I.mu);
        Vec p(dim), ps0(m_i), pz0(m_i), dpn(M), psx(M), pzx(M);
        frd.download_direction(b, p.data(), ps0.data(), pz0.data(), dpn.data(), psx.data(), pzx.data());
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
        // A_e, A_i at the trial point: a full sweep there
        DeviceNlp& one = single.device();
        one.set_scaling(I.req->scales);
        if (!I.req->params.empty()) one.set_parameters(I.req->params.data(), /*per_instance=*/false);
        one.upload_x(Xt.data());
        one.upload_duals(St.data(), yt.data(), Zt.data());
        one.sweep_full();
        one.download_V(Vt.data());
        I.ls.on_kkt_errors(current_kkt, restoration_kkt_error(st, Vt, Xt, St, yt, Zt, I.entry.x_r, I.entry.w, I.mu));
      }
      bool searching = false;
      for (const FrInstance& I : inst)
        searching = searching || (I.running && !I.ls.call_feasibility_restoration && I.ls.want != Want::Done);
      if (!searching) break;
    }
    for (FrInstance& I : inst)
      if (I.running && I.ls.call_feasibility_restoration) finish(I, ExitStatus::FEASIBILITY_RESTORATION_FAILED);  // :721-723

    // ---- commit (:775-801), AD refresh (:809-812) and every norm the next decisions need ----
    if (!select(running)) continue;
    for (int b = 0; b < B; ++b) {
      const LineSearch& ls = inst[b].ls;
      frd.alpha[b] = ls.end == End::Fallback ? ls.alpha_max : ls.alpha;
      frd.alpha_z[b] = ls.alpha_z;
    }
    frd.upload();
    frd.commit();
    frd.sweep();
    frd.errors(/*check_all_V=*/false, err);
    const bool timed_out = since(solve_start) > options.timeout;
    for (int b = 0; b < B; ++b) {
      FrInstance& I = inst[b];
      if (!I.running) continue;
      take_errors(I, b);
      if (I.E_0 > options.tolerance)  // :819-832
        update_barrier_parameter(I.mu, I.mu_min, I.tau, *I.filter, [&](double m) { return ipm_E_mu(I.cur.e, m, m_e, mi_ext); });
      I.req->rep->delta = I.delta;
      ++*I.req->iterations;
      if (*I.req->iterations >= options.max_iterations) finish(I, ExitStatus::MAX_ITERATIONS_EXCEEDED);
      else if (timed_out) finish(I, ExitStatus::TIMEOUT);
    }
  }

  // ---- exit (feasibility_restoration.hpp:602-628): the regularization as it was, the outer iterate, the status ----
  sys.set_regularization_state(saved_regularization);
  sys.set_gamma_min(1e-10);
  for (BatchRestorationRequest& r : requests) {
    FrInstance& I = inst[r.b];
    Vec y(m_e), Z(mi_ext), pn(M), sx(M);
    frd.download_instance(r.b, r.x.data(), r.s.data(), y.data(), Z.data(), pn.data(), sx.data(), Z.data() + m_i);
    r.rep->restoration_iterations += *r.iterations - I.it_before;
    if (I.core == ExitStatus::CALLBACK_REQUESTED_STOP) {
      // back to the original problem: least-squares multipliers at the new point (:606-617), on the batch-1 system
      single.device().set_scaling(r.scales);
      if (!r.params.empty()) single.device().set_parameters(r.params.data(), /*per_instance=*/false);
      r.status = restoration_multiplier_estimate(single, r.x, r.s, r.y, r.z, r.mu, *r.rep) ? ExitStatus::SUCCESS : ExitStatus::FACTORIZATION_FAILED;
    } else if (I.core == ExitStatus::SUCCESS) {
      r.status = ExitStatus::LOCALLY_INFEASIBLE;
    } else {
      r.status = ExitStatus::FEASIBILITY_RESTORATION_FAILED;
    }
  }
}

}  // namespace slpx
