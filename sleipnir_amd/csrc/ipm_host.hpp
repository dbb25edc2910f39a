// Host-side pieces of the interior-point iteration shared by the single-problem drivers (ipm_drivers.hpp) and
// the batched lockstep loop (batch_lockstep.cpp): norms over downloaded vectors, the KKT error measures, the
// filter (its rules: ipm_decide.h), the fraction-to-the-boundary rule.  (The line search and the scalar decisions
// around it: ipm_line_search.hpp.)
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "ipm_decide.h"
#include "nlp.hpp"

namespace slpx::ipm_host {

using Vec = std::vector<double>;
using clk = std::chrono::steady_clock;

inline double since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }

inline double norm_inf(const double* v, int n) {
  double m = 0.0;
  for (int i = 0; i < n; ++i) m = std::max(m, std::abs(v[i]));
  return m;
}
inline double norm_1(const double* v, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += std::abs(v[i]);
  return s;
}
inline bool all_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// out += scale_rows(A)ᵀ v  with A in CSC over `vals`; row_scale may be null
inline void add_At_v(const CscPattern& A, const double* vals, const double* row_scale, const double* v,
              double sign, Vec& out) {
  for (int c = 0; c < A.cols; ++c) {
    double acc = 0.0;
    for (int p = A.colptr[c]; p < A.colptr[c + 1]; ++p) {
      const int r = A.rowidx[p];
      acc += (row_scale ? row_scale[r] * vals[p] : vals[p]) * v[r];
    }
    out[c] += sign * acc;
  }
}

// is_locally_infeasible.hpp:17-60, the equality rows, on host vectors: ‖A_eᵀc_e‖ < 1e-6 and ‖c_e‖ > 1e-2
// (interior_point.hpp:387-395, sqp.hpp:277-285)
inline bool equality_rows_locally_infeasible(const NlpStructure& st, const double* Ae, const Vec& c_e) {
  if (st.m_e == 0) return false;
  Vec t(st.n, 0.0);
  add_At_v(st.Ae, Ae, nullptr, c_e.data(), 1.0, t);
  double nt = 0.0, nc = 0.0;
  for (double v : t) nt += v * v;
  for (double v : c_e) nc += v * v;
  return std::sqrt(nt) < 1e-6 && std::sqrt(nc) > 1e-2;
}

enum class ErrType { INF_NORM_SCALED, ONE_NORM };

// Views into one downloaded V (see nlp.hpp for the layout)
struct VView {
  const NlpStructure& s;
  const Vec& V;
  double f() const { return V[s.off_f]; }
  const double* c_e() const { return V.data() + s.off_ce; }
  const double* c_i() const { return V.data() + s.off_ci; }
  const double* Ae() const { return V.data() + s.off_Ae; }
  const double* Ai() const { return V.data() + s.off_Ai; }
  Vec g_dense() const {
    Vec g(s.n, 0.0);
    for (int c = 0; c < s.n; ++c)
      for (int p = s.g_pat.colptr[c]; p < s.g_pat.colptr[c + 1]; ++p) g[c] += V[s.off_g + p];
    return g;
  }
};

// util/kkt_error.hpp:92-146.  `inv` = optional un-scaling (kkt_error.hpp:216-251):
// inv_f multiplies g, inv_ce/inv_ci multiply the rows of A_e/A_i and c_e/c_i/s,
// and y, z are replaced by d_c∘y·inv_f, d_c∘z·inv_f, μ by inv_f·μ.
template <ErrType T>
double kkt_error_impl(const NlpStructure& st, const Vec& g, const double* Ae, const double* c_e,
                      const double* Ai, const double* c_i, const Vec& s, const Vec& y, const Vec& z,
                      double mu, const Vec* scales) {
  const int n = st.n, m_e = st.m_e, m_i = st.m_i;
  const bool unscale = scales != nullptr;
  const double inv_f = unscale ? 1.0 / (*scales)[0] : 1.0;
  Vec inv_ce, inv_ci, yu(y), zu(z), su(s), ceu(m_e), ciu(m_i);
  if (unscale) {
    inv_ce.resize(m_e);
    inv_ci.resize(m_i);
    for (int j = 0; j < m_e; ++j) inv_ce[j] = 1.0 / (*scales)[1 + j];
    for (int j = 0; j < m_i; ++j) inv_ci[j] = 1.0 / (*scales)[1 + m_e + j];
    for (int j = 0; j < m_e; ++j) yu[j] = (*scales)[1 + j] * y[j] * inv_f;
    for (int j = 0; j < m_i; ++j) zu[j] = (*scales)[1 + m_e + j] * z[j] * inv_f;
    for (int j = 0; j < m_i; ++j) su[j] = inv_ci[j] * s[j];
  }
  for (int j = 0; j < m_e; ++j) ceu[j] = unscale ? inv_ce[j] * c_e[j] : c_e[j];
  for (int j = 0; j < m_i; ++j) ciu[j] = unscale ? inv_ci[j] * c_i[j] : c_i[j];
  const double muu = inv_f * mu;
  Vec dual(n);
  for (int i = 0; i < n; ++i) dual[i] = inv_f * g[i];
  add_At_v(st.Ae, Ae, unscale ? inv_ce.data() : nullptr, yu.data(), -1.0, dual);
  add_At_v(st.Ai, Ai, unscale ? inv_ci.data() : nullptr, zu.data(), -1.0, dual);
  Vec comp(m_i), cis(m_i);
  for (int j = 0; j < m_i; ++j) {
    comp[j] = su[j] * zu[j] - muu;
    cis[j] = ciu[j] - su[j];
  }
  if constexpr (T == ErrType::INF_NORM_SCALED) {
    constexpr double s_max = 100.0;
    const double s_d =
        std::max(s_max, (norm_1(yu.data(), m_e) + norm_1(zu.data(), m_i)) / double(m_e + m_i)) / s_max;
    const double s_c = std::max(s_max, norm_1(zu.data(), m_i) / double(m_i)) / s_max;
    return std::max({norm_inf(dual.data(), n) / s_d, norm_inf(comp.data(), m_i) / s_c,
                     norm_inf(ceu.data(), m_e), norm_inf(cis.data(), m_i)});
  } else {
    return norm_1(dual.data(), n) + norm_1(comp.data(), m_i) + norm_1(ceu.data(), m_e) +
           norm_1(cis.data(), m_i);
  }
}

inline bool scaling_is_identity(const NlpStructure& st, const Vec& scales) {
  // problem_scaling.hpp:111-113
  return scales[0] == 1.0 && st.m_e == 0 && st.m_i == 0;
}

// filter.hpp:17-212 (the entry type and the device's copy of the table: ipm_decide.h)
inline FilterEntry make_entry(double c, double v) { return FilterEntry{c, v}; }
inline FilterEntry make_entry(double f, const Vec& s, const double* c_e, int m_e, const double* c_i, double mu) {
  double logsum = 0.0, viol = norm_1(c_e, m_e);
  for (size_t j = 0; j < s.size(); ++j) {
    logsum += std::log(s[j]);
    viol += std::abs(c_i[j] - s[j]);
  }
  return FilterEntry{f - mu * logsum, viol};
}
inline bool dominated_by(const FilterEntry& a, const FilterEntry& e) { return filter_dominated_by(a, e); }

class Filter {
 public:
  double min_constraint_violation, max_constraint_violation;
  explicit Filter(double initial) {
    min_constraint_violation = 1e-4 * std::max(1.0, initial);
    max_constraint_violation = 1e4 * std::max(1.0, initial);
  }
  void reset() {
    m_filter.clear();
    m_last_rejection_due_to_filter = false;
  }
  bool try_add(const FilterEntry& cur, const FilterEntry& trial, double D_phi, double alpha) {
    // the rules: ipm_decide.h (one source for this driver and for the launch that decides the common iteration)
    FilterEntry add;
    bool insert = false;
    int last = m_last_rejection_due_to_filter ? 1 : 0;
    const int through = filter_rules(min_constraint_violation, max_constraint_violation, &last, cur, trial, D_phi, alpha,
                                     filter_powers(cur, D_phi, alpha), &add, &insert);
    m_last_rejection_due_to_filter = last != 0;
    if (!through) return false;
    for (auto& e : m_filter)
      if (dominated_by(trial, e)) {
        m_last_rejection_due_to_filter = true;
        return false;
      }
    if (insert) {
      m_filter.erase(std::remove_if(m_filter.begin(), m_filter.end(),
                                    [&](const FilterEntry& e) { return dominated_by(e, add); }),
                     m_filter.end());
      m_filter.push_back(add);
    }
    return true;
  }
  bool last_rejection_due_to_filter() const { return m_last_rejection_due_to_filter; }
  // the table as the device keeps it (ipm_decide.h); false: more entries than it holds
  bool to_state(FilterState& F) const {
    if (m_filter.size() > static_cast<size_t>(kFilterCapacity)) return false;
    F.min_constraint_violation = min_constraint_violation;
    F.max_constraint_violation = max_constraint_violation;
    F.n = static_cast<int>(m_filter.size());
    F.last_rejection_due_to_filter = m_last_rejection_due_to_filter ? 1 : 0;
    for (int k = 0; k < F.n; ++k) {
      F.ent[2 * k] = m_filter[k].cost;
      F.ent[2 * k + 1] = m_filter[k].constraint_violation;
    }
    return true;
  }
  void from_state(const FilterState& F) {
    min_constraint_violation = F.min_constraint_violation;
    max_constraint_violation = F.max_constraint_violation;
    m_last_rejection_due_to_filter = F.last_rejection_due_to_filter != 0;
    m_filter.clear();
    for (int k = 0; k < F.n; ++k) m_filter.push_back(FilterEntry{F.ent[2 * k], F.ent[2 * k + 1]});
  }

 private:
  std::vector<FilterEntry> m_filter;
  bool m_last_rejection_due_to_filter = false;
};

// fraction_to_the_boundary_rule.hpp:19-43
inline double ftb(const Vec& x, const Vec& p, double tau) {
  double alpha = 1.0;
  for (size_t i = 0; i < x.size(); ++i)
    if (alpha * p[i] < -tau * x[i]) alpha = -tau / p[i] * x[i];
  return alpha;
}

inline Vec axpy(const Vec& a, double alpha, const Vec& b) {
  Vec r(a.size());
  for (size_t i = 0; i < a.size(); ++i) r[i] = a[i] + alpha * b[i];
  return r;
}
}  // namespace slpx::ipm_host
