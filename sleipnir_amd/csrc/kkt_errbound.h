// Error bounds of a solve, p of Kreg p = b on the factors in memory, as plain functions shared by the kernels
// (kkt_errbound.hip) and by the host (the CPU tests run the same bodies): one source for both sides, like
// kkt_residual.h and ipm_decide.h.  Kreg, the row map and the order of a row's terms are those of row_residual().
//
//   w_i   = |b_i| + sum_j |Kreg_ij| |p_j|     the regularization a term of its own behind the diagonal entry
//   t_i   = |r_i| / w_i  (0 where w_i == 0)   berr = max_i t_i: the componentwise backward error (Oettli-Prager)
//   rho_i = a bound on |computed r_i - exact r_i| of row_residual() as written (DESIGN section 4 derives it)
//   f_i   = |r_i| + rho_i                     ferr ~ || |Kreg^-1| f ||_inf / ||p||_inf   (the xSYRFS construction)
//   sum_j |Kreg_ij|                           norm1 = its maximum (Kreg is symmetric: the row sums serve)
//
// and the state machine of Hager's 1-norm estimator in Higham's form (the algorithm of LAPACK's dlacn2), NormEstState:
// host only, fed four scalars per round, so that the device reduces and the host decides.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <limits>

#include "kkt_residual.h"

namespace slpx {

struct RowAbs {
  double w = 0.0;     // |b_i| + sum |Kreg_ij| |p_j|
  double sum = 0.0;   // sum_j |Kreg_ij|
  int32_t terms = 0;  // m_i: the products row_residual() subtracts, the regularization included
  // every operation of row_residual() on this row was exact: each product representable (and none so small that the
  // error term of two_prod could itself have been rounded away), each addition without a rounding error — the
  // computed r_i IS r_i
  bool exact = true;
};

// the step acc -= a x of row_residual() on its leading word, watched: false where it rounded
SLPX_RESIDUAL bool exact_sub_prod(double& hi, double a, double x) {
#pragma clang fp contract(off) reassociate(off)
  double p, pe, s, se;
  two_prod(a, x, p, pe);
  two_sum(hi, -p, s, se);
  hi = s;
  const bool product_safe = p == 0.0 ? (a == 0.0 || x == 0.0) : __builtin_fabs(p) >= 0x1p-960;
  return pe == 0.0 && se == 0.0 && product_safe;
}

// Plain double: every term is >= 0, so the sums carry a relative error of at most (terms + 1) u and no cancellation.
// w takes the terms in the order row_residual() takes them; the row sum takes the diagonal entry as the one number
// the factorization saw, lhs_ii + reg.
SLPX_RESIDUAL RowAbs row_abs_sum(int row, const int32_t* rowptr, const int32_t* ent, const int32_t* col, const double* lhs, const double* p,
                                 double b_i, int n_dec, double delta, double gamma) {
#pragma clang fp contract(off) reassociate(off)
  RowAbs out;
  out.w = __builtin_fabs(b_i);
  double hi = b_i;
  const double reg = row < n_dec ? delta : -gamma;
  for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
    const int32_t j = col[q];
    const double a = lhs[ent[q]], pj = __builtin_fabs(p[j]);
    out.w = out.w + __builtin_fabs(a) * pj;
    ++out.terms;
    if (!exact_sub_prod(hi, a, p[j])) out.exact = false;
    if (j == row) {
      out.w = out.w + __builtin_fabs(reg) * pj;
      ++out.terms;
      if (!exact_sub_prod(hi, reg, p[j])) out.exact = false;
      out.sum = out.sum + __builtin_fabs(a + reg);
    } else {
      out.sum = out.sum + __builtin_fabs(a);
    }
  }
  return out;
}

// t_i.  w == 0 means b_i and every product are zero, and so is r_i; a w that is neither (NaN) must not hide behind
// the zero: it is passed on.
SLPX_RESIDUAL double berr_term(double r, double w) {
#pragma clang fp contract(off) reassociate(off)
  if (w > 0.0) return __builtin_fabs(r) / w;
  if (w == 0.0) return 0.0;
  return w + r;  // NaN
}

// rho_i: |computed r_i - r_i| <= u |computed r_i| + m (m + 1) u^2 W (1 + u)^(2 m + 1) + underflow, W the exact
// |b_i| + sum |Kreg_ij p_j| <= w (1 - u)^-(m + 1) + underflow.  The form below dominates it for
// every m < 2^24 with its own roundings counted (it has 5 / m to spare in the second term, u |r| in the first), and
// stays within twice of it.
// A row computed without a single rounding (RowAbs::exact) has rho_i = 0: an exact solve reports ferr = 0.
SLPX_RESIDUAL double residual_rounding_bound(double r, double w, int32_t terms, bool exact) {
#pragma clang fp contract(off) reassociate(off)
  if (exact && r == r && __builtin_fabs(r) <= DBL_MAX) return 0.0;
  constexpr double u = 0x1p-53, uu = 0x1p-106;
  const double m = static_cast<double>(terms);
  return 2.0 * u * __builtin_fabs(r) + ((m + 3.0) * (m + 3.0)) * uu * w * (1.0 + m * u) + m * DBL_MIN;
}

// ---- the estimator -------------------------------------------------------------------------------------------------
// ||A||_1 from products with A and A^T (here A = Kreg^-1, or diag(f) Kreg^-1 with the transpose Kreg^-1 diag(f)):
//   round 1        x = e / dim                         v = A x; est = ||v||_1; xi = sign(v)      (dim == 1: est = |v|, done)
//   then, at most kNormEstIterations - 1 times:
//                  x = xi                              z = A^T x; j = the first index of max |z_i|
//                                                      (from the second time on: j equal to the last one ends it)
//                  x = e_j                             v = A x; est = ||v||_1
//                                                      ends if sign(v) == xi everywhere, or est did not grow
//   last           x_i = (-1)^i (1 + i / (dim - 1))    v = A x; est = max(est, 2 ||v||_1 / (3 dim))
// sign(v_i) = v_i >= 0 ? +1 : -1.  A non-finite v anywhere makes the estimate NaN and ends it.  1 + 2 * 5 + 1 = 11
// products at the most.
//
// dlacn2 ends the unit-vector iterations on z(jlast) == |z(j)|, reading the vector; here the device hands the host
// the first index of the maximum only, and the test is j == jlast.  The two differ where z(jlast) is negative or
// ties with an earlier entry; dlacn2 then spends one more pair of products on the same e_j (the signs repeat) and
// ends with the same estimate.
constexpr int kNormEstIterations = 5;

enum NormEstProbe : int32_t {
  kProbeNone = 0,         // done (the device fills zeros: the shared solve stays finite for this problem)
  kProbeUniform = 1,      // e / dim                        product with A
  kProbeUnit = 2,         // e_j                            product with A
  kProbeSigns = 3,        // the kept sign vector           product with A^T
  kProbeAlternating = 4,  // (-1)^i (1 + i / (dim - 1))     product with A
};

class NormEstState {
 public:
  explicit NormEstState(int dim = 1) : m_dim(dim) {}
  // a problem that has nothing to estimate
  void finish(double estimate) {
    m_est = estimate;
    m_probe = kProbeNone;
  }
  NormEstProbe probe() const { return m_probe; }
  int unit_index() const { return m_j; }  // of kProbeUnit
  bool done() const { return m_probe == kProbeNone; }
  // the product of this round is with A^T (kProbeSigns), else with A
  bool transposed() const { return m_probe == kProbeSigns; }
  double estimate() const { return m_est; }
  int solves() const { return m_solves; }
  // The scalars of the product v of the current probe: ||v||_1, the first index of max |v_i|, "sign(v) equals the
  // kept sign vector everywhere", "every v_i is finite".  Returns true where sign(v) becomes the kept sign vector
  // (the next probe is kProbeSigns).
  bool advance(double norm1, int argmax, bool signs_repeated, bool finite) {
    if (done()) return false;
    ++m_solves;
    if (!finite) {
      finish(std::numeric_limits<double>::quiet_NaN());
      return false;
    }
    switch (m_probe) {
      case kProbeUniform:
        m_est = norm1;  // (dim == 1: |v|)
        if (m_dim == 1) {
          m_probe = kProbeNone;
          return false;
        }
        m_iter = 1;
        m_probe = kProbeSigns;
        return true;
      case kProbeSigns:
        if (m_iter >= 2 && argmax == m_j) {
          m_probe = kProbeAlternating;
          return false;
        }
        if (m_iter >= kNormEstIterations) {
          m_probe = kProbeAlternating;
          return false;
        }
        ++m_iter;
        m_j = argmax;
        m_probe = kProbeUnit;
        return false;
      case kProbeUnit: {
        const double old = m_est;
        m_est = norm1;
        if (signs_repeated || m_est <= old) {
          m_probe = kProbeAlternating;
          return false;
        }
        m_probe = kProbeSigns;
        return true;
      }
      case kProbeAlternating: {
        const double alt = 2.0 * (norm1 / static_cast<double>(3 * static_cast<long long>(m_dim)));
        if (alt > m_est) m_est = alt;
        m_probe = kProbeNone;
        return false;
      }
      default: return false;
    }
  }

 private:
  int m_dim;
  NormEstProbe m_probe = kProbeUniform;
  int m_j = -1, m_iter = 0, m_solves = 0;
  double m_est = 0.0;
};

}  // namespace slpx
