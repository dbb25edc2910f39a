// The row bodies of feasibility restoration's closed-form reduction (restoration.hpp's header comment): the kernels'
// view of a restoration iterate, and what one equality row / one inequality row of the restoration problem contributes
// to the reduced system, to the expansion of its solution and to the step sizes.  ONE source: the single-problem
// kernels (restoration.hip) and the batched ones (fr_batch_kernels.h) call these bodies, so a row of an instance of a
// batch goes through the expression trees a single solve's row goes through.
// Index conventions: `e` in [0, M), M = 2 m_e + 2 m_i, walks the extra variables [p_e | n_e | p_i | n_i] — and the
// inequality rows "variable >= 0" that belong to them, with their slacks sx[e] and duals zx[e]; block 0 of the
// inequality rows (c_i(x) - p_i + n_i >= 0) has its slack and dual in s0, z0.
#pragma once

#include <hip/hip_runtime.h>

#include "restoration.hpp"

namespace slpx {

struct FrDevice::Args {
  int n, m_e, m_i;
  int off_Hf, off_Hc;
  double rho;
  KktDev K;
  // the outer system's buffers
  const double* V;
  double* Vt;        // the trial V (values at the trial x)
  double* in;        // [x | y | z_0] as the tape reads it
  double* trial_in;  // the trial x (and whatever else of the tape's input)
  double *s0, *y, *z0, *p, *ps0, *pz0;
  // fixed for the phase
  const double *xr, *w, *g_outer, *s_outer, *scales;
  // the rest of the restoration iterate and of its direction
  double *pn, *sx, *zx, *dpn, *psx, *pzx;
  double *soc_ce, *soc_c0, *soc_x;
  // the look-ahead iterate (expand with ahead): s_0, y, z_0 beside the trial input, the rest of it
  double *s0_t, *y_t, *z0_t, *pn_t, *sx_t, *zx_t;
};

namespace {

constexpr double kFrRho = 1e3;  // feasibility_restoration.hpp:391

// One equality row j of the restoration problem, c_e(x)_j - p_e_j + n_e_j = 0, with its two bound rows p_e_j >= 0,
// n_e_j >= 0: Sigma of the bound rows, the right-hand sides of the p_e and n_e rows of the Newton-KKT system
// (interior_point.hpp:441-448 on the restoration callbacks), the constraint value (or its second-order-correction
// accumulator) and the (c_i' - s') terms of the two bound rows.
struct FrEq {
  double S1, S2, rpe, rne, ce, c1, c2, s1, z1, s2, z2, i1, i2;
};
__device__ __forceinline__ FrEq fr_eq_row(const FrDevice::Args& A, int j, double mu, bool soc) {
  FrEq r;
  const int me = A.m_e;
  r.s1 = A.sx[j];
  r.z1 = A.zx[j];
  r.s2 = A.sx[me + j];
  r.z2 = A.zx[me + j];
  const double pe = A.pn[j], ne = A.pn[me + j], yj = A.y[j];
  r.i1 = 1.0 / r.s1;
  r.i2 = 1.0 / r.s2;
  r.S1 = r.i1 * r.z1;
  r.S2 = r.i2 * r.z2;
  double t1, t2;
  if (soc) {  // :611-616: mu S^-1 e - Sigma (c_i - s)^soc
    r.c1 = A.soc_x[j];
    r.c2 = A.soc_x[me + j];
    r.ce = A.soc_ce[j];
    t1 = mu * r.i1 - r.S1 * r.c1;
    t2 = mu * r.i2 - r.S2 * r.c2;
  } else {  // :444-447: -Sigma c_i + mu S^-1 e + z
    r.c1 = pe - r.s1;
    r.c2 = ne - r.s2;
    r.ce = (A.V[A.K.off_ce + j] - pe) + ne;
    t1 = (-(r.S1 * pe) + mu * r.i1) + r.z1;
    t2 = (-(r.S2 * ne) + mu * r.i2) + r.z2;
  }
  // -g' + A_e'^T y + A_i'^T t: the cost's gradient is rho, the column of p_e has -1 in row j of A_e' and 1 in its bound row
  r.rpe = (-A.rho - yj) + t1;
  r.rne = (-A.rho + yj) + t2;
  return r;
}

// One inequality row r of the outer problem inside the restoration problem, c_i(x)_r - p_i_r + n_i_r >= 0 (block 0),
// with the bound rows of p_i_r and n_i_r (blocks 3, 4).
// (u3 = -rho + t3, u4 = -rho + t4: the right-hand sides of the p_i and n_i rows are r_pi = u3 - t0, r_ni = u4 + t0.
// Sigma_0 = z_0 / s_0 of a row whose slack a run of short steps has driven to 1e-10 is 1e21, and t0 with it: every
// formula below is arranged so that no two terms of that size are subtracted from each other — eliminating the rows
// in closed form is then BETTER conditioned than factoring them)
struct FrIn {
  double sig, S3, S4, a3, a4, det, u3, u4, t0, c0, c3, c4, s0, z0, s3, z3, s4, z4, i0, i3, i4;
};
__device__ __forceinline__ FrIn fr_in_row(const FrDevice::Args& A, int r, double delta, double mu, bool soc) {
  FrIn q;
  const int e3 = 2 * A.m_e + r, e4 = 2 * A.m_e + A.m_i + r;
  q.s0 = A.s0[r];
  q.z0 = A.z0[r];
  q.s3 = A.sx[e3];
  q.z3 = A.zx[e3];
  q.s4 = A.sx[e4];
  q.z4 = A.zx[e4];
  const double pi = A.pn[e3], ni = A.pn[e4];
  q.i0 = 1.0 / q.s0;
  q.i3 = 1.0 / q.s3;
  q.i4 = 1.0 / q.s4;
  q.sig = q.i0 * q.z0;
  q.S3 = q.i3 * q.z3;
  q.S4 = q.i4 * q.z4;
  double t3, t4;
  if (soc) {
    q.c0 = A.soc_c0[r];
    q.c3 = A.soc_x[e3];
    q.c4 = A.soc_x[e4];
    q.t0 = mu * q.i0 - q.sig * q.c0;
    t3 = mu * q.i3 - q.S3 * q.c3;
    t4 = mu * q.i4 - q.S4 * q.c4;
  } else {
    const double ci = (A.V[A.K.off_ci + r] - pi) + ni;
    q.c0 = ci - q.s0;
    q.c3 = pi - q.s3;
    q.c4 = ni - q.s4;
    q.t0 = (-(q.sig * ci) + mu * q.i0) + q.z0;
    t3 = (-(q.S3 * pi) + mu * q.i3) + q.z3;
    t4 = (-(q.S4 * ni) + mu * q.i4) + q.z4;
  }
  // the column of p_i has -1 in row r of block 0 and 1 in its bound row; n_i: 1 and 1
  q.u3 = -A.rho + t3;
  q.u4 = -A.rho + t4;
  q.a3 = q.S3 + delta;
  q.a4 = q.S4 + delta;
  q.det = q.sig * (q.a3 + q.a4) + q.a3 * q.a4;
  return q;
}
__device__ __forceinline__ double fr_sigma_eff(const FrIn& q) { return q.sig * q.a3 * q.a4 / q.det; }
// what row r contributes to the x rows of the reduced right-hand side, per unit of A_i(r, :)
// (t0 + Sigma_0 (a4 r_pi - a3 r_ni) / det with the two t0 terms combined: 1 - Sigma_0 (a3 + a4) / det = a3 a4 / det)
__device__ __forceinline__ double fr_rhs_mult(const FrIn& q) {
  return (q.a3 * q.a4 * q.t0 + q.sig * (q.a4 * q.u3 - q.a3 * q.u4)) / q.det;
}

}  // namespace

}  // namespace slpx
