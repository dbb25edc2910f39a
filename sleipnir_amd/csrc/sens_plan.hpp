// Sensitivity plan: the static index maps that turn the derivatives of the EXTENDED structure — the model
// differentiated with respect to x' = [x ; p], the parameters behind the decision variables (nlp.hpp:
// build_nlp_structure with the parameter nodes appended) — into the right-hand sides of
//
//   [H + AᵢᵀΣAᵢ  Aₑᵀ] [ dx ]   [ −r_x − AᵢᵀΣ r_i ]
//   [    Aₑ       0 ] [−dy ] = [      −r_e        ]        ds = Aᵢ dx + r_i      dz = −Σ ds         Σ = S⁻¹Z
//
// for every parameter q, with r_x = (∇²ₓₚL)[:, q], r_e = ∂c_e/∂p_q, r_i = ∂c_i/∂p_q at the iterate held fixed: the
// KKT conditions of interior_point.hpp:426-481 differentiated, ds and dz eliminated the way p_s and p_z are there.  The
// matrix is the one kkt_plan.hpp assembles and the unknown [dx; −dy] the one it solves for.
//
//   M = [∇²ₓₚL; ∂c_e/∂p; ∂c_i/∂p]   (n + m_e + m_i) x n_p, "unreduced": column q is [r_x; r_e; r_i]
//   R                               (n + m_e) x n_p, "reduced": column q is the right-hand side above
//
// Both are held dense and parameter-major: M[q * dimM + row], R[q * dim + row].  V' is the value vector of the extended
// structure, V the model's own; both swept at unit scales with the multipliers in the user's units (warm_start.h), so
// that everything here is in the user's units.
//
// A pure function of the two structures' patterns: no device, no values.  sens_rows.h holds the row formulas — the
// bodies the kernels of sensitivity.hip and the host executor below both run, so a row has one summation order.
#pragma once

#include <cstdint>
#include <vector>

#include "nlp.hpp"

namespace slpx {

struct SensPlan {
  int n = 0, n_p = 0, m_e = 0, m_i = 0;
  int dim = 0;   // n + m_e: the order of the KKT system
  int dimM = 0;  // n + m_e + m_i: the rows of M
  int nV = 0, nVx = 0;  // lengths of V and V'

  // M[q * dimM + row] = sum_{t in [m_ptr[q * dimM + row], m_ptr[q * dimM + row + 1])} V'[m_src[t]]
  // rows < n: the entries (n + q, row) of the lower triangles of H_f' and H_c', in that order; rows of c_e, c_i: the
  // entry (row, n + q) of A_e', A_i'.  Every structural non-zero of those blocks appears exactly once; no entry of
  // the p-p block of the Hessians (rows and columns >= n) appears at all.
  std::vector<int32_t> m_ptr, m_src;

  // reduction: R[q * dim + i] for i < n adds, over the entries of column i of A_i in pattern order,
  //   V[red_src[t]] * (z[red_row[t]] / s[red_row[t]]) * M[q * dimM + n + m_e + red_row[t]],  t in [red_ptr[i], red_ptr[i + 1])
  std::vector<int32_t> red_ptr, red_src, red_row;

  // expansion: A_i by rows, columns ascending: (A_i dx)[j] = sum_t V[ai_src[t]] * dx[ai_col[t]], t in [ai_rowptr[j], ai_rowptr[j + 1])
  std::vector<int32_t> ai_rowptr, ai_col, ai_src;

  // the cost's derivatives, for the cotangent on the optimal cost (the adjoint below): g_i = V[g_src[i]], i < n, and
  // f_p[q] = ∂f/∂p_q = V'[fp_src[q]] (column n + q of the extended structure's g_pat); −1 where the pattern has no entry
  std::vector<int32_t> g_src, fp_src;
};

// `model`: the structure of the model over x; `extended`: the same model over [x ; p] (n + n_p variables, the same
// constraints).  Throws std::runtime_error where the two do not belong together.
SensPlan build_sens_plan(const NlpStructure& model, const NlpStructure& extended);

// ---- the plan executed on host arrays (tests, and the reference the kernels are compared with) ----
// Vx = V' [nVx], V [nV], s, z [m_i]: M [n_p * dimM] and R [n_p * dim]
void sens_host_rhs(const SensPlan& p, const double* Vx, const double* V, const double* s, const double* z, double* M, double* R);
// rhs [dim] = R dp and r_i [m_i] = (∂c_i/∂p) dp, summed over q ascending
void sens_host_combine(const SensPlan& p, const double* M, const double* R, const double* dp, double* rhs, double* r_i);
// sol = [dx; −dy] [dim], r_i [m_i] (of that right-hand side) -> dx [n], ds [m_i], dy [m_e], dz [m_i]
void sens_host_expand(const SensPlan& p, const double* V, const double* s, const double* z, const double* sol, const double* r_i,
                      double* dx, double* ds, double* dy, double* dz);
// grad [n_p]: grad[q] = wᵀ R[:, q], w [dim]
void sens_host_vjp(const SensPlan& p, const double* R, const double* w, double* grad);

// ---- the adjoint of the whole map p -> (x, s, y, z, cost), cost = f at the iterate (include/slpx.h: "the full vjp") ----
// Forward, per parameter q:  K [dx; −dy] = R[:, q]   ds = A_i dx + r_i   dz = −Σ ds   dcost = g·dx + f_p[q].
// Reverse, for cotangents vx [n], vs [m_i], vy [m_e], vz [m_i], vcost [1], any of them absent (null):
//   t = vs − Σ ∘ vz      u = vx + A_iᵀ t + vcost g      K w = [u; −vy]      grad_q = wᵀR[:, q] + t·r_i[:, q] + vcost f_p[q]
// A term whose cotangent is absent is skipped, not added as zero: with vx alone the right-hand side is [vx; 0] and
// the gradient wᵀR, bit for bit sens_host_vjp's.
struct SensCotangent {
  const double *vx = nullptr, *vs = nullptr, *vy = nullptr, *vz = nullptr, *vcost = nullptr;
};
// V [nV], s, z [m_i] -> rhs [dim] = [u; −vy]
void sens_host_adjoint_rhs(const SensPlan& p, const double* V, const double* s, const double* z, const SensCotangent& v, double* rhs);
// Vx = V' [nVx], M [n_p * dimM], R [n_p * dim], s, z [m_i], w [dim] -> grad [n_p]
void sens_host_vjp_full(const SensPlan& p, const double* Vx, const double* M, const double* R, const double* s, const double* z,
                        const double* w, const SensCotangent& v, double* grad);

// ---- batched calls: which instances are differentiated at all (include/slpx.h: batched sensitivities) ----
// The per-instance outcome of a batched sensitivity call (slpx.h: status[B]).
constexpr int32_t kSensComputed = 0;     // differentiated
constexpr int32_t kSensSkipped = 1;      // a NaN or an Inf among its inputs, or an s_j <= 0 (Sigma = z / s would not be finite)
constexpr int32_t kSensNotFactored = 2;  // the KKT system at its iterate could not be factored (set by the driver)
// status[b] = kSensSkipped where a row of instance b — x [B][n], s [B][m_i], y [B][m_e], z [B][m_i], mu [B],
// params [B][n_p], extra [B][n_extra] (dp or vx; null: none) — holds a value that is not finite, or s an entry <= 0;
// kSensComputed otherwise.  An array whose row has no entries may be null.  A pure function: no device, no model.
void sens_classify_instances(int B, int n, int m_e, int m_i, int n_p, const double* x, const double* s, const double* y,
                             const double* z, const double* mu, const double* params, const double* extra, int n_extra,
                             int32_t* status);
// The same for several arrays beside the iterate — the cotangents of the full vjp: status[b] = kSensSkipped where row b of
// ANY given array (rows [B][width]; a null one, or one without entries, is not looked at) holds a value that is not
// finite, kSensComputed otherwise.  A pure function.
struct SensExtraRows {
  const double* rows = nullptr;
  int width = 0;
};
void sens_classify_extras(int B, const SensExtraRows* extras, int count, int32_t* status);

}  // namespace slpx
