// The rows of the sensitivity right-hand sides and of their expansion as plain functions shared by the kernels
// (sensitivity.hip) and by the host executor (sens_plan.cpp; the CPU tests run it): one source for both sides, like
// kkt_residual.h.  The index maps are those of SensPlan (sens_plan.hpp), which also states the mathematics.
//
// Every function computes ONE output entry from its inputs alone, its terms in the plan's order: the bits of an
// entry do not depend on who computes it or with what launch geometry.  Products join their sum through an explicit
// fma and nothing else is contracted, so the host and the device round alike.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SLPX_SENS __host__ __device__ inline
#else
#define SLPX_SENS inline
#endif

namespace slpx {

constexpr int kSensVjpThreads = 256;  // lanes of one dot product of the vjp (sens_vjp_partial / sens_vjp_fold)

// M[q][row]: the sum of the entries of V' the plan names (k = q * dimM + row)
SLPX_SENS double sens_m_entry(const int32_t* m_ptr, const int32_t* m_src, const double* Vx, int64_t k) {
#pragma clang fp contract(off) reassociate(off)
  double acc = 0.0;
  for (int32_t t = m_ptr[k]; t < m_ptr[k + 1]; ++t) acc += Vx[m_src[t]];
  return acc;
}

// R[q][row], row < n + m_e:  −r_x[row] − sum_j A_i[j, row] (z_j / s_j) r_i[j]  above,  −r_e below.
// r_i[j] is summed here from V' again (not read back from M): the launch that writes M needs no second pass.
SLPX_SENS double sens_reduced_entry(int n, int m_e, int dimM, const int32_t* m_ptr, const int32_t* m_src, const int32_t* red_ptr,
                                    const int32_t* red_src, const int32_t* red_row, const double* Vx, const double* V,
                                    const double* s, const double* z, int q, int row, double m_own) {
#pragma clang fp contract(off) reassociate(off)
  if (row >= n) return -m_own;
  double acc = 0.0;
  const int64_t ri0 = static_cast<int64_t>(q) * dimM + n + m_e;
  for (int32_t t = red_ptr[row]; t < red_ptr[row + 1]; ++t) {
    const int32_t j = red_row[t];
    const double a_sigma = V[red_src[t]] * (z[j] / s[j]);
    acc = __builtin_fma(a_sigma, sens_m_entry(m_ptr, m_src, Vx, ri0 + j), acc);
  }
  return -m_own - acc;
}

// entry `row` of R dp (row < dim, stride = dim, first = 0) or of (∂c_i/∂p) dp (stride = dimM, first = n + m_e): q ascending
SLPX_SENS double sens_combine_entry(int n_p, const double* A, int64_t stride, int64_t first, int row, const double* dp) {
#pragma clang fp contract(off) reassociate(off)
  double acc = 0.0;
  for (int q = 0; q < n_p; ++q) acc = __builtin_fma(A[q * stride + first + row], dp[q], acc);
  return acc;
}

// ds[j] = (A_i dx)[j] + r_i[j], the row's entries in column order
SLPX_SENS double sens_ds_entry(const int32_t* ai_rowptr, const int32_t* ai_col, const int32_t* ai_src, const double* V,
                               const double* dx, const double* r_i, int j) {
#pragma clang fp contract(off) reassociate(off)
  double acc = 0.0;
  for (int32_t t = ai_rowptr[j]; t < ai_rowptr[j + 1]; ++t) acc = __builtin_fma(V[ai_src[t]], dx[ai_col[t]], acc);
  return acc + r_i[j];
}
// dz[j] = −(z_j / s_j) ds[j]
SLPX_SENS double sens_dz_entry(double s, double z, double ds) {
#pragma clang fp contract(off) reassociate(off)
  return -((z / s) * ds);
}

// wᵀ R[:, q] in a fixed order: lane t of kSensVjpThreads sums the rows t, t + kSensVjpThreads, ... ascending, and the
// lanes' sums are folded pairwise, lane t with lane t + width for width = kSensVjpThreads / 2, ..., 1.
SLPX_SENS double sens_vjp_partial(int dim, const double* Rq, const double* w, int lane) {
#pragma clang fp contract(off) reassociate(off)
  double acc = 0.0;
  for (int row = lane; row < dim; row += kSensVjpThreads) acc = __builtin_fma(w[row], Rq[row], acc);
  return acc;
}

// ---- the adjoint: cotangents on x, s, y, z and on the cost (sens_plan.hpp: the adjoint) ----
// A null cotangent is absent and its term is skipped; one on rows the model does not have is absent too.

// whether t = vs − Σ ∘ vz has any term
SLPX_SENS bool sens_adjoint_has_t(int m_i, const double* vs, const double* vz) { return m_i > 0 && (vs != nullptr || vz != nullptr); }

// t[j] = vs[j] − (z_j / s_j) vz[j] (sens_adjoint_has_t holds)
SLPX_SENS double sens_adjoint_t_entry(const double* s, const double* z, const double* vs, const double* vz, int j) {
#pragma clang fp contract(off) reassociate(off)
  if (vz == nullptr) return vs[j];
  const double sigma = z[j] / s[j];
  if (vs == nullptr) return -(sigma * vz[j]);
  return __builtin_fma(-sigma, vz[j], vs[j]);
}

// entry `row` < n + m_e of the adjoint's right-hand side [u; −vy]: above the equality rows
//   vx[row] + sum_j A_i[j, row] t_j + vcost g_row
// with the entries of column `row` of A_i in pattern order and t_j recomputed in place (as sens_reduced_entry
// recomputes r_i), below them −vy.  With vx alone: [vx; 0], the bits of vx.
SLPX_SENS double sens_adjoint_rhs_entry(int n, const int32_t* red_ptr, const int32_t* red_src, const int32_t* red_row, const int32_t* g_src,
                                        const double* V, const double* s, const double* z, const double* vx, const double* vs,
                                        const double* vy, const double* vz, const double* vcost, int row) {
#pragma clang fp contract(off) reassociate(off)
  if (row >= n) return vy != nullptr ? -vy[row - n] : 0.0;
  double acc = vx != nullptr ? vx[row] : 0.0;
  if (vs != nullptr || vz != nullptr)
    for (int32_t t = red_ptr[row]; t < red_ptr[row + 1]; ++t)
      acc = __builtin_fma(V[red_src[t]], sens_adjoint_t_entry(s, z, vs, vz, red_row[t]), acc);
  if (vcost != nullptr && g_src[row] >= 0) acc = __builtin_fma(vcost[0], V[g_src[row]], acc);
  return acc;
}

// t · r_i[:, q] in the order of sens_vjp_partial: lane t of kSensVjpThreads sums the rows t, t + kSensVjpThreads, ...
// ascending, the lanes' sums folded pairwise like those of wᵀR.  r_i: M[q] + n + m_e.
SLPX_SENS double sens_adjoint_direct_partial(int m_i, const double* r_i, const double* s, const double* z, const double* vs,
                                             const double* vz, int lane) {
#pragma clang fp contract(off) reassociate(off)
  double acc = 0.0;
  for (int j = lane; j < m_i; j += kSensVjpThreads) acc = __builtin_fma(sens_adjoint_t_entry(s, z, vs, vz, j), r_i[j], acc);
  return acc;
}

// grad[q] = (wᵀR) + (t·r_i) + vcost f_p[q], in that order; a term that is absent is skipped
SLPX_SENS double sens_vjp_full_sum(double wR, bool direct, double tr, const double* vcost, int32_t fp_src, const double* Vx) {
#pragma clang fp contract(off) reassociate(off)
  double acc = wR;
  if (direct) acc = acc + tr;
  if (vcost != nullptr && fp_src >= 0) acc = __builtin_fma(vcost[0], Vx[fp_src], acc);
  return acc;
}

}  // namespace slpx
