// The regularization policy of SparseRegularizedLDLT::compute (util/sparse_regularized_ldlt.hpp:64-152) for ONE
// problem, on scalars: what is tried, how an attempt's inertia counters are judged, the answer to a failed attempt,
// the give-up and what the memory (prev_delta, prev_gamma) holds afterwards.  No device calls: the drivers of
// newton.cpp are launchers around the loops at the end of this file, tests/test_reg_policy_cpu.py scripts the same
// loops without a GPU, and ipm_lookahead_body (ipm_kernels.h) takes a twin launch's choice from the predicates.
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <vector>

#include "ipm_decide.h"  // SLPX_DECIDE; device.hpp: LdltStats

namespace slpx {

// Eigen::ComputationInfo stand-in
enum class FactorInfo : int { Success = 0, NumericalIssue = 1 };

constexpr double kLdltMinPivot = 1e-4;          // :83   |D| of an accepted unregularized attempt
constexpr double kLdltFirstDelta = 1e-4;        // :96
constexpr double kLdltFirstGamma = 1e-10;       // :120, :134, :140
constexpr double kLdltDefaultGammaMin = 1e-10;  // :197
constexpr double kLdltGrowth = 10.0;            // :124-125, :130, :134, :139-140
constexpr double kLdltGiveUp = 1e20;            // :145

// What an attempt showed.  1 and 3 are also the modes of the twin launches whose second attempt is the answer to
// them (IpmTwin::mode; mode 2: the unregularized attempt beside the loop's first guess).
enum LdltVerdict : int {
  kLdltAccepted = 0,
  kLdltTooManyNegative = 1,  // :127
  kLdltSmallPivot = 2,       // :83, the unregularized attempt only
  kLdltTooManyPositive = 3,  // :131
  kLdltZeroPivots = 4,       // :116
  kLdltFailed = 5,           // :136 (info != Success: an exactly-zero or non-finite pivot)
  kLdltOtherInertia = 6,     // (none of :116-135: the reference tries the same again)
};

SLPX_DECIDE bool ldlt_ideal(const LdltStats& st, int n, int m_e) {  // :82, :111, no bad pivot
  return st.n_bad == 0 && st.n_pos == n && st.n_neg == m_e && st.n_zero == 0;
}
SLPX_DECIDE double ldlt_min_abs(const LdltStats& st) { return __builtin_bit_cast(double, st.min_abs_bits); }
SLPX_DECIDE LdltVerdict ldlt_judge(const LdltStats& st, int n, int m_e, bool unregularized) {
  if (st.n_bad != 0) return kLdltFailed;
  if (ldlt_ideal(st, n, m_e)) return unregularized && !(ldlt_min_abs(st) >= kLdltMinPivot) ? kLdltSmallPivot : kLdltAccepted;
  if (st.n_zero > 0) return kLdltZeroPivots;
  if (st.n_neg > m_e) return kLdltTooManyNegative;
  return st.n_pos > n ? kLdltTooManyPositive : kLdltOtherInertia;
}
// A launch held two attempts: is the second the one the policy makes next, given what the first showed?
SLPX_DECIDE bool ldlt_second_stands(int mode, LdltVerdict first) {
  return first != kLdltAccepted && (mode == 2 || mode == first);
}

// :114-141: the next (delta, gamma) after an attempt that showed `v`
inline void ldlt_answer(LdltVerdict v, double& delta, double& gamma) {
  const double more_gamma = gamma == 0.0 ? kLdltFirstGamma : gamma * kLdltGrowth;
  switch (v) {
    case kLdltZeroPivots:  // :116-126
      if (gamma != 0.0) delta *= kLdltGrowth;
      gamma = more_gamma;
      break;
    case kLdltTooManyNegative: delta *= kLdltGrowth; break;  // :127-130
    case kLdltTooManyPositive: gamma = more_gamma; break;    // :131-135
    case kLdltFailed:                                        // :136-141
      delta *= kLdltGrowth;
      gamma = more_gamma;
      break;
    default: break;
  }
}

struct LdltLaunch {  // a twin launch: the attempt (d0, g0) and, beside it, (d1, g1) — IpmTwin::mode
  double d0, g0, d1, g1;
  int mode;
  bool operator==(const LdltLaunch&) const = default;
};

// One compute() of one problem.  `delta`, `gamma`: the regularized attempt the loop is at (or starts with, while the
// unregularized one is still to be judged); `prev_delta`, `prev_gamma`: the memory, in at start() and final once done().
class LdltPolicy {
 public:
  double delta = 0.0, gamma = 0.0, prev_delta = 0.0, prev_gamma = 0.0;
  FactorInfo info = FactorInfo::Success;
  int factorizations = 0;  // attempts judged

  void start(int n, int m_e, double prev_delta_, double prev_gamma_, double gamma_min, bool skip_first) {
    m_n = n;
    m_m_e = m_e;
    prev_delta = prev_delta_;
    prev_gamma = prev_gamma_;
    delta = prev_delta == 0.0 ? kLdltFirstDelta : std::max(prev_delta / 2.0, std::numeric_limits<double>::epsilon());  // :95-98
    gamma = gamma_min;                                                                                                 // :102
    m_unregularized = !skip_first;  // :74-87
    m_done = false;
    info = FactorInfo::Success;
    factorizations = 0;
  }
  bool done() const { return m_done; }
  bool unregularized() const { return m_unregularized; }  // the attempt at hand is the one without regularization
  double try_delta() const { return m_unregularized ? 0.0 : delta; }
  double try_gamma() const { return m_unregularized ? 0.0 : gamma; }
  // the attempt at hand and the one that follows it if it shows `expect` (too many negative or positive pivots)
  LdltLaunch launch(int expect) const {
    if (m_unregularized) return {0.0, 0.0, delta, gamma, 2};
    LdltLaunch l{delta, gamma, delta, gamma, expect};
    ldlt_answer(static_cast<LdltVerdict>(expect), l.d1, l.g1);
    return l;
  }

  // the counters of the attempt at hand; `extra_min_pivot`: of rows eliminated outside the factorization (:83)
  LdltVerdict judge(const LdltStats& st, double extra_min_pivot = std::numeric_limits<double>::infinity()) {
    ++factorizations;
    LdltVerdict v = ldlt_judge(st, m_n, m_m_e, m_unregularized);
    if (m_unregularized) {
      if (v == kLdltAccepted && !(extra_min_pivot >= kLdltMinPivot)) v = kLdltSmallPivot;
      m_unregularized = false;
      if (v == kLdltAccepted) finish(0.0, 0.0);  // :84-86
      return v;
    }
    if (v == kLdltAccepted) {  // :111-115
      finish(delta, gamma);
      return v;
    }
    ldlt_answer(v, delta, gamma);
    if (delta > kLdltGiveUp || gamma > kLdltGiveUp) {  // :145-150
      info = FactorInfo::NumericalIssue;
      finish(delta, gamma);
    }
    return v;
  }

 private:
  int m_n = 0, m_m_e = 0;
  bool m_unregularized = false, m_done = true;
  void finish(double d, double g) {
    prev_delta = d;
    prev_gamma = g;
    m_done = true;
  }
};

// The loop for a batch, one attempt per launch: launch(delta, gamma, active) factors the problems with active[b] != 0
// and returns every problem's counters.  Returns the number of launches.  (`launch_for_nobody`: the unregularized
// launch is made even where `active` leaves nobody.)  `extra_min_pivot` (or none): per problem, the smallest pivot of
// rows the caller eliminated outside the factorization — it joins the test of the unregularized attempt, as in
// ldlt_run_twin (restoration.hpp: the closed-form rows of a batch of restoration problems).
template <class Launch>
int ldlt_run_batch(std::vector<LdltPolicy>& pol, std::vector<uint8_t>& active, bool launch_for_nobody, Launch&& launch,
                   const std::vector<double>* extra_min_pivot = nullptr) {
  const size_t B = pol.size();
  std::vector<double> delta(B, 0.0), gamma(B, 0.0);
  int launches = 0;
  for (bool any = launch_for_nobody || std::any_of(active.begin(), active.end(), [](uint8_t a) { return a != 0; }); any; ++launches) {
    for (size_t b = 0; b < B; ++b)
      if (active[b]) {
        delta[b] = pol[b].try_delta();
        gamma[b] = pol[b].try_gamma();
      }
    const LdltStats* stats = launch(delta, gamma, active);
    any = false;
    for (size_t b = 0; b < B; ++b)
      if (active[b]) {
        if (extra_min_pivot) pol[b].judge(stats[b], (*extra_min_pivot)[b]);
        else pol[b].judge(stats[b]);
        active[b] = !pol[b].done();
        any = any || active[b];
      }
  }
  return launches;
}

// The loop for one problem, two attempts per launch: L.launch(LdltLaunch) says whether the launch held the second,
// L.first() / L.second() are their counters, L.adopt_second() makes the second's factors and solve the current ones.
// The attempts are judged in the policy's order from their own counters, so the (delta, gamma) tried, the one
// accepted and the count of factorizations are ldlt_run_batch's; a second attempt that does not stand is ignored.
// `expect_memory` (or none: too many negative pivots, always): which answer the second attempt of the loop's first
// launch stands for — the one that launch's first attempt drew in the LAST compute (a phase of a solve that needs a
// larger gamma needs it iteration after iteration, and the loop starts from gamma_min every time, :102).
struct LdltTwinRun {
  int launches = 0, taken = 0;  // launches that held two attempts; second attempts the policy accepted
};
template <class Launcher>
LdltTwinRun ldlt_run_twin(LdltPolicy& P, Launcher& L, int* expect_memory,
                          double extra_min_pivot = std::numeric_limits<double>::infinity()) {
  LdltTwinRun run;
  int expect = expect_memory ? *expect_memory : kLdltTooManyNegative;
  bool second_is_current = false;  // the launch's second attempt was made with what the policy tries now
  while (!P.done()) {
    if (second_is_current) {
      second_is_current = false;
      if (P.judge(L.second()) == kLdltAccepted) {
        L.adopt_second();
        ++run.taken;
      }
      continue;
    }
    const LdltLaunch tl = P.launch(expect);
    const bool have_second = L.launch(tl);
    run.launches += have_second;
    const LdltVerdict v = P.judge(L.first(), extra_min_pivot);
    if (tl.mode != 2) {  // (only the loop's first launch is remembered, and expected of)
      if (expect_memory && (v == kLdltAccepted || v == kLdltTooManyNegative)) *expect_memory = kLdltTooManyNegative;
      if (expect_memory && v == kLdltTooManyPositive) *expect_memory = kLdltTooManyPositive;
      expect_memory = nullptr;
      expect = kLdltTooManyNegative;
    }
    second_is_current = have_second && !P.done() && ldlt_second_stands(tl.mode, v);
  }
  return run;
}

}  // namespace slpx
