// Kernels of the batched interior-point driver (batch_lockstep.cpp): B instances of one compiled model, each in its own
// slice of batch-major buffers ([b * stride + i]), one 256-thread workgroup per instance.  An instance whose active
// flag is 0 is skipped: nothing of its slice is read or written.  Every reduction runs in an order fixed by the
// model's sizes alone (strided per-thread partials, then block_reduce: wave64 butterflies and a fixed combination of
// the waves), so an instance's scalars do not depend on B or on which other instances are active.  The iterate, the
// direction and the trial point stay on the device; the host reads a few scalars per instance and decides.
// The per-row formulas are the bodies of ipm_formulas.h — the ones the single solve's kernels and the host run.
//
// Per-instance problem scaling: the batch system's tape runs with unit scales; the dual inputs are multiplied by the
// instance's d_ce, d_ci before a sweep (batch_load_state_kernel), and what the sweep wrote is multiplied by the scale
// the tape would have applied at its output write (batch_scale_V_kernel; tape_kernels.h, tape_jit.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include "device.hpp"
#include "ipm_batch.hpp"
#include "ipm_decide.h"
#include "ipm_formulas.h"
#include "ipm_reduce.h"

namespace slpx {

constexpr int kBatchThreads = 256;

// V[b][k], k < count: the tape's scaling of entry k with instance b's scales.  Entries the tape writes are multiplied
// in place; static entries (never written by the tape) are set from their unscaled value, so the kernel may follow any
// number of sweeps.  grid (chunks, B).
__global__ __launch_bounds__(kBatchThreads) void batch_scale_V_kernel(double* __restrict__ V, int v_stride, int count,
                                                                      const int32_t* __restrict__ scale_idx,
                                                                      const uint8_t* __restrict__ is_static,
                                                                      const double* __restrict__ static_raw,
                                                                      const double* __restrict__ S, int ns,
                                                                      const uint8_t* __restrict__ active) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int k = blockIdx.x * kBatchThreads + threadIdx.x;
  if (k >= count) return;
  const int32_t sc = scale_idx[k];
  double* v = V + static_cast<size_t>(b) * v_stride + k;
  const double f = sc >= 0 ? S[static_cast<size_t>(b) * ns + sc] : 1.0;
  if (is_static[k]) *v = f * static_raw[k];
  else if (sc >= 0) *v = f * *v;
}

// The tape's inputs [x | d_ce y | d_ci z] of instance b from an iterate (problem.hpp:631-634: the duals enter the
// tape scaled), and with_state: s, y, z unscaled into the system's own buffers (what assemble / build_rhs read).
// x only when y == nullptr.  grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_load_state_kernel(KktDev K, double* __restrict__ in, int in_stride,
                                                                         BatchIter it, const double* __restrict__ S,
                                                                         int ns, double* __restrict__ sys_s,
                                                                         double* __restrict__ sys_y,
                                                                         double* __restrict__ sys_z, int with_state,
                                                                         const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e, m_i = K.m_i;
  double* inb = in + static_cast<size_t>(b) * in_stride;
  const double* x = it.x + static_cast<size_t>(b) * n;
  for (int i = threadIdx.x; i < n; i += kBatchThreads) inb[i] = x[i];
  if (it.y == nullptr) return;
  const double* sc = S + static_cast<size_t>(b) * ns;
  const double* y = it.y + static_cast<size_t>(b) * m_e;
  const double* z = it.z + static_cast<size_t>(b) * m_i;
  for (int j = threadIdx.x; j < m_e; j += kBatchThreads) {
    inb[n + j] = sc[1 + j] * y[j];
    if (with_state) sys_y[static_cast<size_t>(b) * m_e + j] = y[j];
  }
  for (int j = threadIdx.x; j < m_i; j += kBatchThreads) {
    inb[n + m_e + j] = sc[1 + m_e + j] * z[j];
    if (with_state) {
      sys_z[static_cast<size_t>(b) * m_i + j] = z[j];
      sys_s[static_cast<size_t>(b) * m_i + j] = it.s[static_cast<size_t>(b) * m_i + j];
    }
  }
}

// The direction's scalars (interior_point.hpp:488-509, the batched ipm_direction_kernel): out[b] = {alpha_max =
// ftb(s, p_s, tau_b), alpha_z = ftb(z, p_z, tau_b), D_phi = g^T p_x - mu_b sum p_s / s}.  (The sequential rule's result
// is the minimum of its candidates, so the step sizes are exact whatever the order.)  grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_direction_kernel(
    KktDev K, const double* __restrict__ V, int v_stride, const double* __restrict__ s, const double* __restrict__ z,
    const double* __restrict__ p, const double* __restrict__ ps, const double* __restrict__ pz,
    const double* __restrict__ mu, const double* __restrict__ tau, const uint8_t* __restrict__ active,
    double* __restrict__ out) {
  __shared__ double scratch[(kBatchThreads / 64 + 1) * 3];
  const int b = blockIdx.x;
  if (!active[b]) return;  // (uniform across the workgroup: no lane reaches the barriers below)
  const int tid = threadIdx.x;
  const int m_i = K.m_i, n = K.n;
  V += static_cast<size_t>(b) * v_stride;
  s += static_cast<size_t>(b) * m_i;
  z += static_cast<size_t>(b) * m_i;
  ps += static_cast<size_t>(b) * m_i;
  pz += static_cast<size_t>(b) * m_i;
  p += static_cast<size_t>(b) * K.dim;
  const double mu_b = mu[b], tau_b = tau[b];
  double acc[3] = {1.0, 1.0, 0.0};
  double logbar = 0.0;
  for (int r = tid; r < m_i; r += kBatchThreads) {
    const double sr = s[r], psr = ps[r], zr = z[r], pzr = pz[r];
    acc[0] = ftb_candidate(acc[0], tau_b, psr, sr);
    acc[1] = ftb_candidate(acc[1], tau_b, pzr, zr);
    logbar += (1.0 / sr) * psr;
  }
  for (int j = tid; j < n; j += kBatchThreads) {
    const int gs = K.g_src[j];
    if (gs >= 0) acc[2] += V[gs] * p[j];
  }
  acc[2] -= mu_b * logbar;
  const int ops[3] = {IPM_MIN, IPM_MIN, IPM_SUM};
  block_reduce<3, kBatchThreads>(acc, ops, scratch);
  if (tid == 0) {
    out[3 * b + 0] = acc[0];
    out[3 * b + 1] = acc[1];
    out[3 * b + 2] = acc[2];
  }
}

// Trial point (interior_point.hpp:512-523, :641, :696-699): T = (x, s, y, z) + (alpha, alpha, alpha_z, alpha_z) * d,
// d = the Newton direction (mode 0; p_y = -p[n..]) or the second-order correction's (mode 1).  s_from_ci[b]: the
// trial s is the trial c_i (feasible_ipm), set by batch_trial_metrics_kernel after the sweep.  The trial x goes to
// the tape's inputs; with_duals: the trial y, z too (scaled by d_c).  grid (B).
struct BatchTrialArgs {
  BatchIter cur, trial, soc;  // soc: x, s, y (already -p[n..]), z of the correction's direction
  const double *p, *ps, *pz;  // the Newton direction
  const int32_t* mode;
  const uint8_t* s_from_ci;
  const double *alpha, *alpha_z;
  double* in;
  int in_stride;
  const double* S;
  int ns, with_duals;
};
__global__ __launch_bounds__(kBatchThreads) void batch_trial_kernel(KktDev K, BatchTrialArgs A,
                                                                    const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e, m_i = K.m_i;
  const size_t bx = static_cast<size_t>(b) * n, be = static_cast<size_t>(b) * m_e, bi = static_cast<size_t>(b) * m_i;
  const bool soc = A.mode[b] == 1;
  const double a = A.alpha[b], az = A.alpha_z[b];
  const double* px = soc ? A.soc.x + bx : A.p + static_cast<size_t>(b) * K.dim;
  double* inb = A.in + static_cast<size_t>(b) * A.in_stride;
  const double* sc = A.S + static_cast<size_t>(b) * A.ns;
  for (int i = threadIdx.x; i < n; i += kBatchThreads) {
    const double t = A.cur.x[bx + i] + a * px[i];
    A.trial.x[bx + i] = t;
    inb[i] = t;
  }
  for (int j = threadIdx.x; j < m_e; j += kBatchThreads) {
    const double py = soc ? A.soc.y[be + j] : -A.p[static_cast<size_t>(b) * K.dim + n + j];
    const double t = A.cur.y[be + j] + az * py;
    A.trial.y[be + j] = t;
    if (A.with_duals) inb[n + j] = sc[1 + j] * t;
  }
  const bool keep_s = !soc && A.s_from_ci[b];
  for (int j = threadIdx.x; j < m_i; j += kBatchThreads) {
    const double ps = soc ? A.soc.s[bi + j] : A.ps[bi + j];
    const double pz = soc ? A.soc.z[bi + j] : A.pz[bi + j];
    if (!keep_s) A.trial.s[bi + j] = A.cur.s[bi + j] + a * ps;
    const double t = A.cur.z[bi + j] + az * pz;
    A.trial.z[bi + j] = t;
    if (A.with_duals) inb[n + m_e + j] = sc[1 + m_e + j] * t;
  }
}

// The trial point's merit quantities after a value sweep (V head scaled): out[b] = {f, ||c_e||_1 + ||c_i - s||_1,
// sum ln s, count of non-finite f, c_e, c_i}; the trial c_e, c_i are kept (tce, tci) for a correction that follows.
// grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_trial_metrics_kernel(KktDev K, const double* __restrict__ V,
                                                                            int v_stride, const uint8_t* __restrict__ s_from_ci,
                                                                            const int32_t* __restrict__ mode,
                                                                            double* __restrict__ ts, double* __restrict__ tce,
                                                                            double* __restrict__ tci,
                                                                            const uint8_t* __restrict__ active,
                                                                            double* __restrict__ out) {
  __shared__ double scratch[(kBatchThreads / 64 + 1) * 3];
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int m_e = K.m_e, m_i = K.m_i, tid = threadIdx.x;
  V += static_cast<size_t>(b) * v_stride;
  ts += static_cast<size_t>(b) * m_i;
  tce += static_cast<size_t>(b) * m_e;
  tci += static_cast<size_t>(b) * m_i;
  const bool take_ci = mode[b] == 0 && s_from_ci[b];
  double acc[3] = {0.0, 0.0, 0.0};  // violation, sum ln s, non-finite count
  for (int j = tid; j < m_e; j += kBatchThreads) {
    const double c = V[K.off_ce + j];
    tce[j] = c;
    acc[0] += fabs(c);
    if (!ipm_isfinite(c)) acc[2] += 1.0;
  }
  for (int j = tid; j < m_i; j += kBatchThreads) {
    const double c = V[K.off_ci + j];
    tci[j] = c;
    if (take_ci) ts[j] = c;
    const double sj = ts[j];
    acc[0] += fabs(c - sj);
    acc[1] += log(sj);
    if (!ipm_isfinite(c)) acc[2] += 1.0;
  }
  const int ops[3] = {IPM_SUM, IPM_SUM, IPM_SUM};
  block_reduce<3, kBatchThreads>(acc, ops, scratch);
  if (tid == 0) {
    const double f = V[K.off_f];
    out[4 * b + 0] = f;
    out[4 * b + 1] = acc[0];
    out[4 * b + 2] = acc[1];
    out[4 * b + 3] = acc[2] + (ipm_isfinite(f) ? 0.0 : 1.0);
  }
}

// The reductions of the error measures and checks at an iterate (util/kkt_error.hpp:92-146 scaled and un-scaled,
// :216-251; interior_point.hpp:283-286, :387-408), out[b][BatchErr].  mu[b] enters the one-norm complementarity only.
// grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_errors_kernel(KktDev K, const double* __restrict__ V, int v_stride,
                                                                     int nV, BatchIter it, const double* __restrict__ mu,
                                                                     const double* __restrict__ S, int ns,
                                                                     const uint8_t* __restrict__ active,
                                                                     double* __restrict__ out) {
  constexpr int NQ = kBatchErrReduced;
  __shared__ double scratch[(kBatchThreads / 64 + 1) * NQ];
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e, m_i = K.m_i, tid = threadIdx.x;
  V += static_cast<size_t>(b) * v_stride;
  const double* x = it.x + static_cast<size_t>(b) * n;
  const double* s = it.s + static_cast<size_t>(b) * m_i;
  const double* y = it.y + static_cast<size_t>(b) * m_e;
  const double* z = it.z + static_cast<size_t>(b) * m_i;
  const double* sc = S + static_cast<size_t>(b) * ns;
  const double mu_b = mu[b], inv_f = 1.0 / sc[0];
  const double* Ae = V + K.off_Ae;
  const double* Ai = V + K.off_Ai;
  double a[NQ];
  const int ops[NQ] = {IPM_MAX, IPM_SUM, IPM_SUM, IPM_SUM, IPM_MAX, IPM_MIN, IPM_SUM, IPM_MAX, IPM_SUM, IPM_MAX, IPM_SUM,
                       IPM_MAX, IPM_SUM, IPM_SUM, IPM_MAX, IPM_MAX, IPM_MAX,
                       IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM, IPM_MAX, IPM_SUM, IPM_MAX, IPM_SUM};
#pragma unroll
  for (int q = 0; q < NQ; ++q) a[q] = ops[q] == IPM_MIN ? INFINITY : 0.0;
  auto A = [&](int k) -> double& { return a[k - 1]; };
  // dual residual per column, scaled (g - A_e^T y - A_i^T z) and un-scaled (the same of the un-scaled quantities),
  // accumulated column by column as add_At_v does; A_e^T c_e and A_i^T min(c_i, 0) for the infeasibility tests
  for (int c = tid; c < n; c += kBatchThreads) {
    const int gs = K.g_src[c];
    const double g = gs >= 0 ? V[gs] : 0.0;
    double d = g, du = inv_f * g;
    double ae = 0.0, aeu = 0.0, aec = 0.0;
    for (int q = K.ae_colptr[c]; q < K.ae_colptr[c + 1]; ++q) {
      const int r = K.ae_rowidx[q];
      ae += Ae[q] * y[r];
      aeu += ((1.0 / sc[1 + r]) * Ae[q]) * (sc[1 + r] * y[r] * inv_f);
      aec += Ae[q] * V[K.off_ce + r];
    }
    d += -ae;
    du += -aeu;
    double ai = 0.0, aiu = 0.0, aic = 0.0;
    for (int q = K.ai_colptr[c]; q < K.ai_colptr[c + 1]; ++q) {
      const int r = K.ai_rowidx[q];
      ai += Ai[q] * z[r];
      aiu += ((1.0 / sc[1 + m_e + r]) * Ai[q]) * (sc[1 + m_e + r] * z[r] * inv_f);
      aic += Ai[q] * fmin(V[K.off_ci + r], 0.0);
    }
    d += -ai;
    du += -aiu;
    A(BE_DUAL_INF) = fmax(A(BE_DUAL_INF), fabs(d));
    A(BE_DUAL_1) += fabs(d);
    A(BE_DUALU_INF) = fmax(A(BE_DUALU_INF), fabs(du));
    A(BE_AETCE2) += aec * aec;
    A(BE_AITCM2) += aic * aic;
    A(BE_X_INF) = fmax(A(BE_X_INF), fabs(x[c]));
    if (!ipm_isfinite(x[c])) A(BE_X_BAD) += 1.0;
  }
  for (int j = tid; j < m_e; j += kBatchThreads) {
    const double ce = V[K.off_ce + j], inv_ce = 1.0 / sc[1 + j];
    A(BE_Y1) += fabs(y[j]);
    A(BE_YU1) += fabs(sc[1 + j] * y[j] * inv_f);
    A(BE_CE_INF) = fmax(A(BE_CE_INF), fabs(ce));
    A(BE_CE_1) += fabs(ce);
    A(BE_CEU_INF) = fmax(A(BE_CEU_INF), fabs(inv_ce * ce));
    A(BE_CE2) += ce * ce;
  }
  for (int j = tid; j < m_i; j += kBatchThreads) {
    const double ci = V[K.off_ci + j], sj = s[j], zj = z[j], dci = sc[1 + m_e + j], inv_ci = 1.0 / dci;
    const double sz = sj * zj, su = inv_ci * sj, zu = dci * zj * inv_f;
    A(BE_Z1) += fabs(zj);
    A(BE_SZ_MAX) = fmax(A(BE_SZ_MAX), sz);
    A(BE_SZ_MIN) = fmin(A(BE_SZ_MIN), sz);
    A(BE_COMP_1) += fabs(sz - mu_b);
    A(BE_CIS_INF) = fmax(A(BE_CIS_INF), fabs(ci - sj));
    A(BE_CIS_1) += fabs(ci - sj);
    A(BE_ZU1) += fabs(zu);
    A(BE_COMPU_INF) = fmax(A(BE_COMPU_INF), fabs(su * zu - 0.0));
    A(BE_CISU_INF) = fmax(A(BE_CISU_INF), fabs(inv_ci * ci - su));
    A(BE_LOGSUM) += log(sj);
    if (!(ci > 0.0)) A(BE_CI_NONPOS) += 1.0;
    const double cm = fmin(ci, 0.0);
    A(BE_CM2) += cm * cm;
    A(BE_S_INF) = fmax(A(BE_S_INF), fabs(sj));
    if (!ipm_isfinite(sj)) A(BE_S_BAD) += 1.0;
  }
  for (int k = tid; k < nV; k += kBatchThreads)
    if (!ipm_isfinite(V[k])) A(BE_V_BAD) += 1.0;
  block_reduce<NQ, kBatchThreads>(a, ops, scratch);
  double* o = out + static_cast<size_t>(b) * kBatchErrN;
  if (tid == 0) {
    o[BE_F] = V[K.off_f];
#pragma unroll
    for (int q = 0; q < NQ; ++q) o[1 + q] = a[q];
  }
}

// Second-order correction, right-hand side (interior_point.hpp:598-616) from the current point's V: first[b] starts
// the accumulation (c_e, c_i - s); then c_e_soc = alpha_soc c_e_soc + trial c_e, (c_i - s)_soc = alpha_soc (..) +
// trial c_i - trial s, and rhs = [-g + A_e^T y + A_i^T (mu/s - z/s (c_i - s)_soc) | -c_e_soc].  t: [B][m_i] scratch.
// grid (B).
struct BatchSocArgs {
  const double* V;  // current point
  int v_stride;
  BatchIter cur;
  const double *ts, *tce, *tci, *alpha_soc, *mu;
  const uint8_t* first;
  double *sce, *scims, *t, *rhs;
};
__global__ __launch_bounds__(kBatchThreads) void batch_soc_rhs_kernel(KktDev K, BatchSocArgs A,
                                                                      const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e, m_i = K.m_i, tid = threadIdx.x;
  const double* V = A.V + static_cast<size_t>(b) * A.v_stride;
  const size_t be = static_cast<size_t>(b) * m_e, bi = static_cast<size_t>(b) * m_i;
  const double as = A.alpha_soc[b], mu_b = A.mu[b];
  const bool first = A.first[b] != 0;
  double* rhs = A.rhs + static_cast<size_t>(b) * K.dim;
  for (int j = tid; j < m_e; j += kBatchThreads) {
    const double prev = first ? V[K.off_ce + j] : A.sce[be + j];
    const double c = soc_accumulate(as, prev, A.tce[be + j]);
    A.sce[be + j] = c;
    rhs[n + j] = -c;
  }
  for (int j = tid; j < m_i; j += kBatchThreads) {
    const double prev = first ? V[K.off_ci + j] - A.cur.s[bi + j] : A.scims[bi + j];
    const double c = soc_accumulate(as, prev, A.tci[bi + j]) - A.ts[bi + j];
    A.scims[bi + j] = c;
    A.t[bi + j] = soc_rhs_multiplier(mu_b, A.cur.s[bi + j], A.cur.z[bi + j], c);
  }
  __syncthreads();  // (t, written above by this workgroup, is read below)
  const double* Ae = V + K.off_Ae;
  const double* Ai = V + K.off_Ai;
  const double* y = A.cur.y + be;
  const double* t = A.t + bi;
  for (int c = tid; c < n; c += kBatchThreads) {
    const int gs = K.g_src[c];
    double r = -(gs >= 0 ? V[gs] : 0.0);
    double acc = 0.0;
    for (int q = K.ae_colptr[c]; q < K.ae_colptr[c + 1]; ++q) acc += Ae[q] * y[K.ae_rowidx[q]];
    r += acc;
    acc = 0.0;
    for (int q = K.ai_colptr[c]; q < K.ai_colptr[c + 1]; ++q) acc += Ai[q] * t[K.ai_rowidx[q]];
    r += acc;
    rhs[c] = r;
  }
}

// Second-order correction, the direction from the solve (interior_point.hpp:617-640): p_x, p_y = -p[n..], p_s =
// (c_i - s)_soc + A_i p_x, p_z = mu/s - z - z/s p_s; out[b] = {ftb(s, p_s, tau), ftb(z, p_z, tau)}.  grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_soc_direction_kernel(
    KktDev K, const double* __restrict__ V, int v_stride, const double* __restrict__ p, BatchIter cur,
    const double* __restrict__ scims, const double* __restrict__ mu, const double* __restrict__ tau, BatchIter soc,
    const uint8_t* __restrict__ active, double* __restrict__ out) {
  __shared__ double scratch[(kBatchThreads / 64 + 1) * 2];
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e, m_i = K.m_i, tid = threadIdx.x;
  V += static_cast<size_t>(b) * v_stride;
  p += static_cast<size_t>(b) * K.dim;
  const size_t bx = static_cast<size_t>(b) * n, be = static_cast<size_t>(b) * m_e, bi = static_cast<size_t>(b) * m_i;
  const double mu_b = mu[b], tau_b = tau[b];
  for (int i = tid; i < n; i += kBatchThreads) soc.x[bx + i] = p[i];
  for (int j = tid; j < m_e; j += kBatchThreads) soc.y[be + j] = -p[n + j];
  double acc[2] = {1.0, 1.0};
  for (int r = tid; r < m_i; r += kBatchThreads) {
    double aipx = 0.0;  // (row r of A_i in column order, as the host's column sweep adds it up)
    for (int q = K.ai_rowptr[r]; q < K.ai_rowptr[r + 1]; ++q) aipx += V[K.ai_src[q]] * p[K.ai_col[q]];
    const double sr = cur.s[bi + r], zr = cur.z[bi + r], sinv = 1.0 / sr;
    const double ps = scims[bi + r] + aipx;
    const double pz = backsub_pz_sinv(mu_b, sinv, zr, ps);
    soc.s[bi + r] = ps;
    soc.z[bi + r] = pz;
    acc[0] = ftb_candidate(acc[0], tau_b, ps, sr);
    acc[1] = ftb_candidate(acc[1], tau_b, pz, zr);
  }
  const int ops[2] = {IPM_MIN, IPM_MIN};
  block_reduce<2, kBatchThreads>(acc, ops, scratch);
  if (tid == 0) {
    out[2 * b + 0] = acc[0];
    out[2 * b + 1] = acc[1];
  }
}

// Commit (interior_point.hpp:773-801): the trial point becomes the iterate, with the z reset (z_reset: a NaN stays).
// grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_commit_kernel(KktDev K, BatchIter trial, BatchIter cur,
                                                                     const double* __restrict__ mu,
                                                                     const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e, m_i = K.m_i;
  const size_t bx = static_cast<size_t>(b) * n, be = static_cast<size_t>(b) * m_e, bi = static_cast<size_t>(b) * m_i;
  const double mu_b = mu[b];
  for (int i = threadIdx.x; i < n; i += kBatchThreads) cur.x[bx + i] = trial.x[bx + i];
  for (int j = threadIdx.x; j < m_e; j += kBatchThreads) cur.y[be + j] = trial.y[be + j];
  for (int j = threadIdx.x; j < m_i; j += kBatchThreads) {
    const double s = trial.s[bi + j];
    cur.s[bi + j] = s;
    cur.z[bi + j] = z_reset(trial.z[bi + j], mu_b, s);
  }
}

}  // namespace slpx
