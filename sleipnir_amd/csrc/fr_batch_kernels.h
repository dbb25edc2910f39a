// Kernels of feasibility restoration for a batch (fr_batch.hpp has the contract): B instances of one compiled model,
// each with its restoration iterate in its own slice of batch-major buffers, its own delta, mu, tau, step sizes and
// flags read from device arrays.  The reduced system is built on a (chunks, B) grid — row-local, nothing reduced —
// with the per-entry loops of fr_build_kernel (restoration.hip) in the same order; every kernel that reduces is one
// 256-thread workgroup per instance: strided per-thread partials, then block_reduce.  No kernel waits for another
// workgroup (the single problem's expand spreads its rows over a grid and joins it by a barrier; a workgroup per
// instance has nothing to join).  An instance whose active flag is 0 is skipped by whole workgroups.
// The row arithmetic is fr_rows.h's (fr_eq_row, fr_in_row, fr_sigma_eff, fr_rhs_mult) and ipm_formulas.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "fr_batch.hpp"
#include "fr_rows.h"
#include "ipm_formulas.h"
#include "ipm_reduce.h"

namespace slpx {

constexpr int kFrBatchThreads = 256;

// A: the pointers of instance 0 (FrDevice::Args of fr_rows.h; the look-ahead pointers are not used).  V = the current
// point's V kept by the device struct, Vt = the batch system's V (a value sweep's), in = the iterate's x, trial_in =
// the batch system's tape input, p = the direction's (dx, w) kept by the device struct.
struct FrBatchArgs {
  FrDevice::Args A;
  int nV, nin;
  const int32_t* diag_of;
  const double *delta, *mu, *tau, *alpha, *alpha_soc, *alpha_z, *mu_outer;
  const uint8_t *soc, *first, *rhs_only, *active;
  double *lhs, *rhs;    // the batch system's, batch-major
  const double* p_sys;  // the batch system's solution [B][dim]
  double *keep_p, *keep_ps0, *keep_pz0, *keep_dpn, *keep_psx, *keep_pzx;
  double* vt_keep;  // [B][nhead]: f, c_e, c_i of an instance's last trial point (a later sweep for others overwrites Vt)
  int nhead;
  double* out;
};

namespace {

// instance b's view: every pointer moved to its slice
__device__ __forceinline__ FrDevice::Args fr_instance(const FrBatchArgs& G, int b) {
  FrDevice::Args A = G.A;
  const size_t sb = static_cast<size_t>(b);
  const size_t n = A.n, me = A.m_e, mi = A.m_i, M = 2 * me + 2 * mi, dim = n + me;
  A.V += sb * G.nV;
  A.Vt += sb * G.nV;
  A.in += sb * n;
  A.trial_in += sb * G.nin;
  A.s0 += sb * mi;
  A.y += sb * me;
  A.z0 += sb * mi;
  A.p += sb * dim;
  A.ps0 += sb * mi;
  A.pz0 += sb * mi;
  A.xr += sb * n;
  A.w += sb * n;
  A.g_outer += sb * n;
  A.s_outer += sb * mi;
  A.scales += sb * (1 + me + mi);
  A.pn += sb * M;
  A.sx += sb * M;
  A.zx += sb * M;
  A.dpn += sb * M;
  A.psx += sb * M;
  A.pzx += sb * M;
  A.soc_ce += sb * me;
  A.soc_c0 += sb * mi;
  A.soc_x += sb * M;
  return A;
}

}  // namespace

// V[b][k] -> Vcur[b][k], k < count, of the active instances.  grid (chunks, B).
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_keep_V_kernel(const double* __restrict__ V, double* __restrict__ Vcur, int count,
                                                                          const uint8_t* __restrict__ active) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int k = blockIdx.x * kFrBatchThreads + threadIdx.x;
  if (k < count) Vcur[static_cast<size_t>(b) * count + k] = V[static_cast<size_t>(b) * count + k];
}

// The reduced system of instance b (restoration.hpp's header comment) for delta[b], mu[b] into lhs[b][nnz], rhs[b][dim];
// soc[b]: the second-order correction's right-hand side; rhs_only[b]: the lhs is in place.  grid (chunks, B), grid-stride
// in x.
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_build_kernel(FrBatchArgs G) {
  const int b = blockIdx.y;
  if (!G.active[b]) return;
  const FrDevice::Args A = fr_instance(G, b);
  const KktDev& K = A.K;
  const double* V = A.V;
  const double delta = G.delta[b], mu = G.mu[b];
  const int soc = G.soc[b], rhs_only = G.rhs_only[b];
  const int32_t* diag_of = G.diag_of;
  double* lhs = G.lhs + static_cast<size_t>(b) * K.nnz_lhs;
  double* rhs = G.rhs + static_cast<size_t>(b) * K.dim;
  const int stride = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
  auto not_Hf = [&](int src) { return src < A.off_Hf || src >= A.off_Hc; };  // the restoration cost has its own Hessian
  if (!rhs_only)
    for (int k = t0; k < K.nnz_lhs; k += stride) {
      const int f = K.fast_src[k];
      double v = 0.0;
      if (f >= 0) {
        v = not_Hf(f) ? V[f] : 0.0;
      } else if (f == -2) {
        double direct = 0.0, prod = 0.0;
        for (int d = K.dptr[k]; d < K.dptr[k + 1]; ++d) {
          const int src = K.dsrc[d];
          if (not_Hf(src)) direct += V[src];
        }
        for (int q = K.pptr[k]; q < K.pptr[k + 1]; ++q) {
          const FrIn row = fr_in_row(A, K.pr[q], delta, mu, false);
          prod += (V[K.pa[q]] * fr_sigma_eff(row)) * V[K.pb[q]];
        }
        v = direct + prod;
      }
      const int d = diag_of[k];
      if (d >= 0) {
        if (d < A.n) {
          v += A.w[d];  // zeta D_R
        } else {
          const FrEq e = fr_eq_row(A, d - A.n, mu, false);
          v = -(1.0 / (e.S1 + delta) + 1.0 / (e.S2 + delta));
        }
      }
      lhs[k] = v;
    }
  for (int j = t0; j < K.dim; j += stride) {
    if (j >= A.n) {
      const FrEq e = fr_eq_row(A, j - A.n, mu, soc != 0);
      rhs[j] = (-e.ce + e.rpe / (e.S1 + delta)) - e.rne / (e.S2 + delta);
      continue;
    }
    const double* Ae = V + K.off_Ae;
    const double* Ai = V + K.off_Ai;
    double aey = 0.0, ait = 0.0;
    for (int q = K.ae_colptr[j]; q < K.ae_colptr[j + 1]; ++q) aey += Ae[q] * A.y[K.ae_rowidx[q]];
    for (int q = K.ai_colptr[j]; q < K.ai_colptr[j + 1]; ++q)
      ait += Ai[q] * fr_rhs_mult(fr_in_row(A, K.ai_rowidx[q], delta, mu, soc != 0));
    const double g = A.w[j] * (A.in[j] - A.xr[j]);  // zeta D_R (x - x_R)
    rhs[j] = (-g + aey) + ait;
  }
}

// p = (dx, w) of the batch system's solution -> kept; dp_e, dn_e, dp_i, dn_i, p_s, p_z of the five inequality blocks
// (interior_point.hpp:470-481 on the restoration problem); out[b] = {alpha_max, alpha_z
// (fraction_to_the_boundary_rule.hpp:19-43 with tau[b]), D_phi (:508-509), the smallest eliminated pivot}; the first
// trial x = x + alpha_max dx into the tape's input.  The rows' formulas are fr_expand_kernel's.  grid (B).
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_expand_kernel(FrBatchArgs G) {
  __shared__ double scratch[(kFrBatchThreads / 64 + 1) * 4];
  const int b = blockIdx.x;
  if (!G.active[b]) return;  // (uniform across the workgroup: no lane reaches the barriers below)
  const FrDevice::Args A = fr_instance(G, b);
  const KktDev& K = A.K;
  const int me = A.m_e, mi = A.m_i, n = A.n, tid = threadIdx.x;
  const double delta = G.delta[b], mu = G.mu[b], tau = G.tau[b];
  const int soc = G.soc[b];
  const double* ps = G.p_sys + static_cast<size_t>(b) * K.dim;
  for (int j = tid; j < K.dim; j += kFrBatchThreads) A.p[j] = ps[j];
  __syncthreads();
  double acc[4] = {1.0, 1.0, 0.0, 1e300};  // alpha_max, alpha_z, D_phi, smallest eliminated pivot
  auto ftb = [&](double s, double psv, double z, double pz) {
    acc[0] = ftb_candidate(acc[0], tau, psv, s);
    acc[1] = ftb_candidate(acc[1], tau, pz, z);
  };
  for (int j = tid; j < me; j += kFrBatchThreads) {
    const FrEq e = fr_eq_row(A, j, mu, soc != 0);
    const double w = A.p[n + j];
    const double d1 = e.S1 + delta, d2 = e.S2 + delta;
    const double dpe = (e.rpe + w) / d1, dne = (e.rne - w) / d2;
    const double ps1 = e.c1 + dpe, ps2 = e.c2 + dne;
    const double pz1 = (mu * e.i1 - e.z1) - e.S1 * ps1, pz2 = (mu * e.i2 - e.z2) - e.S2 * ps2;
    A.dpn[j] = dpe;
    A.dpn[me + j] = dne;
    A.psx[j] = ps1;
    A.psx[me + j] = ps2;
    A.pzx[j] = pz1;
    A.pzx[me + j] = pz2;
    ftb(e.s1, ps1, e.z1, pz1);
    ftb(e.s2, ps2, e.z2, pz2);
    acc[2] += A.rho * dpe + A.rho * dne;
    acc[2] -= mu * (e.i1 * ps1) + mu * (e.i2 * ps2);
    acc[3] = fmin(acc[3], fmin(d1, d2));
  }
  for (int r = tid; r < mi; r += kFrBatchThreads) {
    double aidx = 0.0;
    for (int q = K.ai_rowptr[r]; q < K.ai_rowptr[r + 1]; ++q) aidx += A.V[K.ai_src[q]] * A.p[K.ai_col[q]];
    const FrIn f = fr_in_row(A, r, delta, mu, soc != 0);
    const double a = f.sig + f.a3;
    const double rsum = f.u3 + f.u4;  // r_pi + r_ni
    const double dpi = (f.a4 * ((f.u3 - f.t0) + f.sig * aidx) + f.sig * rsum) / f.det;
    const double dni = (f.a3 * ((f.u4 + f.t0) - f.sig * aidx) + f.sig * rsum) / f.det;
    const double ps0 = f.c0 + (f.a3 * f.a4 * aidx + (f.a3 + f.a4) * f.t0 - f.a4 * f.u3 + f.a3 * f.u4) / f.det;
    const double ps3 = f.c3 + dpi, ps4 = f.c4 + dni;
    const double pz0 = (mu * f.i0 - f.z0) - f.sig * ps0, pz3 = (mu * f.i3 - f.z3) - f.S3 * ps3,
                 pz4 = (mu * f.i4 - f.z4) - f.S4 * ps4;
    const int e3 = 2 * me + r, e4 = 2 * me + mi + r;
    A.dpn[e3] = dpi;
    A.dpn[e4] = dni;
    A.ps0[r] = ps0;
    A.pz0[r] = pz0;
    A.psx[e3] = ps3;
    A.pzx[e3] = pz3;
    A.psx[e4] = ps4;
    A.pzx[e4] = pz4;
    ftb(f.s0, ps0, f.z0, pz0);
    ftb(f.s3, ps3, f.z3, pz3);
    ftb(f.s4, ps4, f.z4, pz4);
    acc[2] += A.rho * dpi + A.rho * dni;
    acc[2] -= mu * (f.i0 * ps0) + mu * (f.i3 * ps3) + mu * (f.i4 * ps4);
    acc[3] = fmin(acc[3], fmin(a, f.det / a));  // (the second pivot, b - sig^2 / a)
  }
  for (int j = tid; j < n; j += kFrBatchThreads) acc[2] += (A.w[j] * (A.in[j] - A.xr[j])) * A.p[j];
  const int ops[4] = {IPM_MIN, IPM_MIN, IPM_SUM, IPM_MIN};
  block_reduce<4, kFrBatchThreads>(acc, ops, scratch);
  if (tid == 0) {
    double* o = G.out + static_cast<size_t>(b) * kFrBatchErrN;
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
    o[3] = acc[3];
  }
  const double alpha = acc[0];
  for (int j = tid; j < n; j += kFrBatchThreads) A.trial_in[j] = A.in[j] + alpha * A.p[j];
}

// trial x = x + alpha[b] dx into the tape's input.  grid (B).
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_trial_point_kernel(FrBatchArgs G) {
  const int b = blockIdx.x;
  if (!G.active[b]) return;
  const FrDevice::Args A = fr_instance(G, b);
  const double alpha = G.alpha[b];
  for (int j = threadIdx.x; j < A.n; j += kFrBatchThreads) A.trial_in[j] = A.in[j] + alpha * A.p[j];
}

// Filter entry (filter.hpp:30-60) of the trial point X + alpha[b] dX of the restoration problem; c_e, c_i of the outer
// problem at the trial x are in Vt (a value sweep, scaled): out[b] = {f, violation, sum ln s, finite}.  grid (B).
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_trial_metrics_kernel(FrBatchArgs G) {
  __shared__ double scratch[(kFrBatchThreads / 64 + 1) * 4];
  const int b = blockIdx.x;
  if (!G.active[b]) return;
  const FrDevice::Args A = fr_instance(G, b);
  const KktDev& K = A.K;
  const int tid = threadIdx.x, me = A.m_e, mi = A.m_i, n = A.n;
  const double alpha = G.alpha[b];
  double acc[4] = {0.0, 0.0, 0.0, 1.0};  // cost, violation, log sum, finite
  double* keep = G.vt_keep + static_cast<size_t>(b) * G.nhead;  // (a second-order correction that follows reads these)
  for (int k = tid; k < G.nhead; k += kFrBatchThreads) keep[k] = A.Vt[k];
  for (int j = tid; j < n; j += kFrBatchThreads) {
    const double d = A.trial_in[j] - A.xr[j];
    acc[0] += 0.5 * (A.w[j] * (d * d));
  }
  auto bound_row = [&](int e, double v) {  // the row "variable e >= 0" at its trial value v
    const double st = A.sx[e] + alpha * A.psx[e];
    acc[1] += fabs(v - st);
    acc[2] += log(st);
  };
  for (int j = tid; j < me; j += kFrBatchThreads) {
    const double pe = A.pn[j] + alpha * A.dpn[j], ne = A.pn[me + j] + alpha * A.dpn[me + j];
    const double c = A.Vt[K.off_ce + j];
    acc[0] += A.rho * pe + A.rho * ne;
    acc[1] += fabs((c - pe) + ne);
    bound_row(j, pe);
    bound_row(me + j, ne);
    if (!isfinite(c)) acc[3] = 0.0;
  }
  for (int r = tid; r < mi; r += kFrBatchThreads) {
    const int e3 = 2 * me + r, e4 = 2 * me + mi + r;
    const double pi = A.pn[e3] + alpha * A.dpn[e3], ni = A.pn[e4] + alpha * A.dpn[e4];
    const double c = A.Vt[K.off_ci + r];
    const double st = A.s0[r] + alpha * A.ps0[r];
    acc[0] += A.rho * pi + A.rho * ni;
    acc[1] += fabs(((c - pi) + ni) - st);
    acc[2] += log(st);
    bound_row(e3, pi);
    bound_row(e4, ni);
    if (!isfinite(c)) acc[3] = 0.0;
  }
  const int ops[4] = {IPM_SUM, IPM_SUM, IPM_SUM, IPM_MIN};
  block_reduce<4, kFrBatchThreads>(acc, ops, scratch);
  if (tid == 0) {
    double* o = G.out + static_cast<size_t>(b) * kFrBatchErrN;
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
    o[3] = (acc[3] != 0.0 && isfinite(acc[0])) ? 1.0 : 0.0;
  }
}

// interior_point.hpp:775-801 on the whole restoration iterate of instance b: alpha[b], alpha_z[b], the z reset with
// mu[b].  grid (B).
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_commit_kernel(FrBatchArgs G) {
  const int b = blockIdx.x;
  if (!G.active[b]) return;
  const FrDevice::Args A = fr_instance(G, b);
  const double alpha = G.alpha[b], alpha_z = G.alpha_z[b], mu = G.mu[b];
  const int n = A.n, me = A.m_e, mi = A.m_i, M = 2 * me + 2 * mi, tid = threadIdx.x;
  for (int j = tid; j < n; j += kFrBatchThreads) A.in[j] = A.in[j] + alpha * A.p[j];
  for (int r = tid; r < me; r += kFrBatchThreads) A.y[r] = A.y[r] + alpha_z * (-A.p[n + r]);
  for (int r = tid; r < mi; r += kFrBatchThreads) {
    const double sn = A.s0[r] + alpha * A.ps0[r];
    A.s0[r] = sn;
    A.z0[r] = z_reset(A.z0[r] + alpha_z * A.pz0[r], mu, sn);
  }
  for (int e = tid; e < M; e += kFrBatchThreads) {
    A.pn[e] = A.pn[e] + alpha * A.dpn[e];
    const double sn = A.sx[e] + alpha * A.psx[e];
    A.sx[e] = sn;
    A.zx[e] = z_reset(A.zx[e] + alpha_z * A.pzx[e], mu, sn);
  }
}

// interior_point.hpp:590-600 on the restoration problem's rows; the trial values of the outer c_e, c_i are the ones the
// instance's last trial metrics kept, the trial point is X + alpha_soc[b] dX with the direction in place; first[b] starts
// the accumulation.  grid (B).
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_soc_accumulate_kernel(FrBatchArgs G) {
  const int b = blockIdx.x;
  if (!G.active[b]) return;
  const FrDevice::Args A = fr_instance(G, b);
  const KktDev& K = A.K;
  const double alpha = G.alpha_soc[b];
  const int first = G.first[b];
  const double* Vt = G.vt_keep + static_cast<size_t>(b) * G.nhead;
  const int me = A.m_e, mi = A.m_i, tid = threadIdx.x;
  auto bound_row = [&](int e, double v_now, double v_trial) {
    const double prev = first ? v_now - A.sx[e] : A.soc_x[e];
    A.soc_x[e] = alpha * prev + (v_trial - (A.sx[e] + alpha * A.psx[e]));
  };
  for (int j = tid; j < me; j += kFrBatchThreads) {
    const double pe = A.pn[j], ne = A.pn[me + j];
    const double pet = pe + alpha * A.dpn[j], net = ne + alpha * A.dpn[me + j];
    const double prev = first ? (A.V[K.off_ce + j] - pe) + ne : A.soc_ce[j];
    A.soc_ce[j] = alpha * prev + ((Vt[K.off_ce + j] - pet) + net);
    bound_row(j, pe, pet);
    bound_row(me + j, ne, net);
  }
  for (int r = tid; r < mi; r += kFrBatchThreads) {
    const int e3 = 2 * me + r, e4 = 2 * me + mi + r;
    const double pi = A.pn[e3], ni = A.pn[e4];
    const double pit = pi + alpha * A.dpn[e3], nit = ni + alpha * A.dpn[e4];
    const double prev = first ? ((A.V[K.off_ci + r] - pi) + ni) - A.s0[r] : A.soc_c0[r];
    A.soc_c0[r] = alpha * prev + (((Vt[K.off_ci + r] - pit) + nit) - (A.s0[r] + alpha * A.ps0[r]));
    bound_row(e3, pi, pit);
    bound_row(e4, ni, nit);
  }
}

// the direction of instance b into its kept copy, or (restore) back.  grid (B).
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_copy_direction_kernel(FrBatchArgs G, int restore) {
  const int b = blockIdx.x;
  if (!G.active[b]) return;
  const FrDevice::Args A = fr_instance(G, b);
  const size_t sb = static_cast<size_t>(b);
  const int mi = A.m_i, M = 2 * A.m_e + 2 * A.m_i, dim = A.n + A.m_e, tid = threadIdx.x;
  double* kp = G.keep_p + sb * dim;
  double* kps0 = G.keep_ps0 + sb * mi;
  double* kpz0 = G.keep_pz0 + sb * mi;
  double* kdpn = G.keep_dpn + sb * M;
  double* kpsx = G.keep_psx + sb * M;
  double* kpzx = G.keep_pzx + sb * M;
  if (restore) {
    for (int j = tid; j < dim; j += kFrBatchThreads) A.p[j] = kp[j];
    for (int r = tid; r < mi; r += kFrBatchThreads) {
      A.ps0[r] = kps0[r];
      A.pz0[r] = kpz0[r];
    }
    for (int e = tid; e < M; e += kFrBatchThreads) {
      A.dpn[e] = kdpn[e];
      A.psx[e] = kpsx[e];
      A.pzx[e] = kpzx[e];
    }
  } else {
    for (int j = tid; j < dim; j += kFrBatchThreads) kp[j] = A.p[j];
    for (int r = tid; r < mi; r += kFrBatchThreads) {
      kps0[r] = A.ps0[r];
      kpz0[r] = A.pz0[r];
    }
    for (int e = tid; e < M; e += kFrBatchThreads) {
      kdpn[e] = A.dpn[e];
      kpsx[e] = A.psx[e];
      kpzx[e] = A.pzx[e];
    }
  }
}

// Error norms (kkt_error.hpp:92-146, un-scaled :216-251), filter entry, local-infeasibility and divergence quantities
// of the restoration problem at instance b's freshly swept iterate, the OUTER problem's filter quantities at (x, s_0)
// (interior_point.hpp:729-752) and the unregularized eliminated minimum pivot: out[b] = FrErrOut.  The quantities and
// their rows are fr_errors_kernel's (restoration.hip), eight lanes per column of x included; one workgroup reduces all
// of an instance's rows, so there are no partials to fold.  f_outer is the sweep's own V[off_f].  grid (B).
namespace fr_berr {
enum {
  DUAL_U, SZ_MAX_U, CE_U, CIS_U, Y1_U, Z1_U, DUAL, SZ_MIN, SZ_MAX, CE, CIS, Y1, Z1, VIOL, LOGSUM,
  AETCE, CESQ, AITCP, CPSQ, XINF, SINF, FINITE, CIPOS,
  COST, VIOL_O, LOGSUM_O, DPHI_O, EMIN0, NQ
};
}
__global__ __launch_bounds__(kFrBatchThreads) void fr_batch_errors_kernel(FrBatchArgs G, int check_all_V) {
  using namespace fr_berr;
  __shared__ double scratch[(kFrBatchThreads / 64 + 1) * NQ];
  const int b = blockIdx.x;
  if (!G.active[b]) return;
  const FrDevice::Args A = fr_instance(G, b);
  const KktDev& K = A.K;
  const double* V = A.V;
  const double mu_outer = G.mu_outer[b];
  const int me = A.m_e, mi = A.m_i, n = A.n, nV = G.nV;
  const int ops[NQ] = {IPM_MAX, IPM_MAX, IPM_MAX, IPM_MAX, IPM_SUM, IPM_SUM, IPM_MAX, IPM_MIN, IPM_MAX, IPM_MAX, IPM_MAX,
                       IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_MAX, IPM_MAX, IPM_MIN,
                       IPM_MIN, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_MIN};
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = ops[q] == IPM_MIN ? 1.0 : 0.0;
  acc[SZ_MIN] = 1e300;
  acc[EMIN0] = 1e300;
  const int stride = kFrBatchThreads, t0 = threadIdx.x;
  const double* d_ce = A.scales + 1;
  const double* d_ci = A.scales + 1 + me;
  const double* ce = V + K.off_ce;
  const double* ci = V + K.off_ci;
  const double* Ae = V + K.off_Ae;
  const double* Ai = V + K.off_Ai;
  auto dual_entry = [&](double d, double du) {
    acc[DUAL] = fmax(acc[DUAL], fabs(d));
    acc[DUAL_U] = fmax(acc[DUAL_U], fabs(du));
  };
  auto var_entry = [&](double v) {
    acc[XINF] = fmax(acc[XINF], fabs(v));
    if (!isfinite(v)) acc[FINITE] = 0.0;
  };
  // an inequality row with slack sr, dual zr, value c and row scale dr (1 for the bound rows)
  auto ineq_row = [&](double c, double sr, double zr, double dr) {
    const double inv = 1.0 / dr, su = inv * sr, zu = dr * zr;
    acc[CIS] = fmax(acc[CIS], fabs(c - sr));
    acc[CIS_U] = fmax(acc[CIS_U], fabs(inv * c - su));
    acc[SZ_MIN] = fmin(acc[SZ_MIN], sr * zr);
    acc[SZ_MAX] = fmax(acc[SZ_MAX], sr * zr);
    acc[SZ_MAX_U] = fmax(acc[SZ_MAX_U], fabs(su * zu));
    acc[Z1] += fabs(zr);
    acc[Z1_U] += fabs(zu);
    const double cp = fmin(c, 0.0);
    acc[CPSQ] += cp * cp;
    acc[VIOL] += fabs(c - sr);
    acc[LOGSUM] += log(sr);
    acc[SINF] = fmax(acc[SINF], fabs(sr));
    if (!isfinite(sr) || !isfinite(c)) acc[FINITE] = 0.0;
    if (!(c > 0.0)) acc[CIPOS] = 0.0;
  };
  // columns of x: eight lanes per column, an entry of the column each, summed by DPP in lane order
  const int lane8 = t0 & 7;
  for (int j = t0 >> 3; j < n; j += stride >> 3) {
    double a1 = 0.0, a1u = 0.0, aetce = 0.0;
    for (int q = K.ae_colptr[j] + lane8; q < K.ae_colptr[j + 1]; q += 8) {
      const int r = K.ae_rowidx[q];
      const double a = Ae[q], dr = d_ce[r];
      const double cer = (ce[r] - A.pn[r]) + A.pn[me + r];
      a1 += a * A.y[r];
      a1u += ((1.0 / dr) * a) * (dr * A.y[r]);
      aetce += a * cer;
    }
    double a2 = 0.0, a2u = 0.0, aitcp = 0.0;
    for (int q = K.ai_colptr[j] + lane8; q < K.ai_colptr[j + 1]; q += 8) {
      const int r = K.ai_rowidx[q];
      const double a = Ai[q], dr = d_ci[r];
      const double cir = (ci[r] - A.pn[2 * me + r]) + A.pn[2 * me + mi + r];
      a2 += a * A.z0[r];
      a2u += ((1.0 / dr) * a) * (dr * A.z0[r]);
      aitcp += a * fmin(cir, 0.0);
    }
    const double xj = A.in[j], dx = xj - A.xr[j], wj = A.w[j], go = A.g_outer[j];
    a1 = ipm_group8_sum(a1);
    a1u = ipm_group8_sum(a1u);
    aetce = ipm_group8_sum(aetce);
    a2 = ipm_group8_sum(a2);
    a2u = ipm_group8_sum(a2u);
    aitcp = ipm_group8_sum(aitcp);
    if (lane8 == 0) {
      const double g = wj * dx;
      dual_entry((g - a1) - a2, (g - a1u) - a2u);
      acc[AETCE] += aetce * aetce;
      acc[AITCP] += aitcp * aitcp;
      var_entry(xj);
      acc[COST] += 0.5 * (wj * (dx * dx));
      acc[DPHI_O] += go * dx;
    }
  }
  // equality rows, with the columns and bound rows of p_e, n_e
  for (int j = t0; j < me; j += stride) {
    const double pe = A.pn[j], ne = A.pn[me + j], yr = A.y[j], dr = d_ce[j];
    const double c = (ce[j] - pe) + ne;
    acc[CE] = fmax(acc[CE], fabs(c));
    acc[CE_U] = fmax(acc[CE_U], fabs((1.0 / dr) * c));
    acc[Y1] += fabs(yr);
    acc[Y1_U] += fabs(dr * yr);
    acc[CESQ] += c * c;
    acc[VIOL] += fabs(c);
    if (!isfinite(c)) acc[FINITE] = 0.0;
    acc[VIOL_O] += fabs(ce[j]);
    // columns: g' - A_e'^T y - A_i'^T z' = rho + y - z_1 (p_e), rho - y - z_2 (n_e)
    const double z1 = A.zx[j], z2 = A.zx[me + j];
    const double yu = (1.0 / dr) * (dr * yr);
    dual_entry((A.rho + yr) - z1, (A.rho + yu) - z1);
    dual_entry((A.rho - yr) - z2, (A.rho - yu) - z2);
    acc[AETCE] += 2.0 * (c * c);  // (-c)^2 + c^2
    const double cp1 = fmin(pe, 0.0), cp2 = fmin(ne, 0.0);
    acc[AITCP] += cp1 * cp1 + cp2 * cp2;
    var_entry(pe);
    var_entry(ne);
    acc[COST] += A.rho * pe + A.rho * ne;
    ineq_row(pe, A.sx[j], z1, 1.0);
    ineq_row(ne, A.sx[me + j], z2, 1.0);
    acc[EMIN0] = fmin(acc[EMIN0], fmin((1.0 / A.sx[j]) * z1, (1.0 / A.sx[me + j]) * z2));
  }
  // inequality rows of block 0, with the columns and bound rows of p_i, n_i
  for (int r = t0; r < mi; r += stride) {
    const int e3 = 2 * me + r, e4 = 2 * me + mi + r;
    const double pi = A.pn[e3], ni = A.pn[e4], sr = A.s0[r], zr = A.z0[r], dr = d_ci[r];
    const double c = (ci[r] - pi) + ni;
    ineq_row(c, sr, zr, dr);
    const double z3 = A.zx[e3], z4 = A.zx[e4];
    const double zu = (1.0 / dr) * (dr * zr);
    dual_entry((A.rho + zr) - z3, (A.rho + zu) - z3);
    dual_entry((A.rho - zr) - z4, (A.rho - zu) - z4);
    const double cp0 = fmin(c, 0.0), cp3 = fmin(pi, 0.0), cp4 = fmin(ni, 0.0);
    acc[AITCP] += (cp3 - cp0) * (cp3 - cp0) + (cp0 + cp4) * (cp0 + cp4);
    var_entry(pi);
    var_entry(ni);
    acc[COST] += A.rho * pi + A.rho * ni;
    ineq_row(pi, A.sx[e3], z3, 1.0);
    ineq_row(ni, A.sx[e4], z4, 1.0);
    {  // the pivots of the (p_i, n_i) block eliminated in that order: a = Sigma_0 + Sigma_3, then det / a
      const double sig = (1.0 / sr) * zr, a3 = (1.0 / A.sx[e3]) * z3, a4 = (1.0 / A.sx[e4]) * z4;
      const double a = sig + a3;
      acc[EMIN0] = fmin(acc[EMIN0], fmin(a, (sig * (a3 + a4) + a3 * a4) / a));
    }
    // the outer problem's filter quantities at (x, s_0)
    acc[VIOL_O] += fabs(ci[r] - sr);
    acc[LOGSUM_O] += log(sr);
    const double so = A.s_outer[r];
    acc[DPHI_O] -= mu_outer * ((1.0 / so) * (sr - so));
  }
  if (check_all_V)
    for (int k = t0; k < nV; k += stride)
      if (!isfinite(V[k])) acc[FINITE] = 0.0;
  block_reduce<NQ, kFrBatchThreads>(acc, ops, scratch);
  if (threadIdx.x == 0) {
    FrErrOut o;
    IpmErrOut& e = o.e;
    e.dual_inf_u = acc[DUAL_U];
    e.sz_max_u = acc[SZ_MAX_U];
    e.ce_inf_u = acc[CE_U];
    e.cis_inf_u = acc[CIS_U];
    e.y1_u = acc[Y1_U];
    e.z1_u = acc[Z1_U];
    e.dual_inf = acc[DUAL];
    e.sz_min = acc[SZ_MIN];
    e.sz_max = acc[SZ_MAX];
    e.ce_inf = acc[CE];
    e.cis_inf = acc[CIS];
    e.y1 = acc[Y1];
    e.z1 = acc[Z1];
    e.f = acc[COST];
    e.viol = acc[VIOL];
    e.logsum = acc[LOGSUM];
    e.aetce_sq = acc[AETCE];
    e.ce_sq = acc[CESQ];
    e.aitcp_sq = acc[AITCP];
    e.cp_sq = acc[CPSQ];
    e.x_inf = acc[XINF];
    e.s_inf = acc[SINF];
    e.finite = (acc[FINITE] != 0.0 && isfinite(acc[COST])) ? 1.0 : 0.0;
    e.ci_all_pos = acc[CIPOS];
    o.f_outer = V[K.off_f];
    o.viol_outer = acc[VIOL_O];
    o.logsum_outer = acc[LOGSUM_O];
    o.dphi_outer = acc[DPHI_O];
    o.eliminated_min_pivot = acc[EMIN0];
    *reinterpret_cast<FrErrOut*>(G.out + static_cast<size_t>(b) * kFrBatchErrN) = o;
  }
}

}  // namespace slpx
