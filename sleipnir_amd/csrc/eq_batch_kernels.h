// Kernels of the batched SQP and Newton drivers (batch_lockstep.cpp): the conventions of ipm_batch_kernels.h — B instances
// of one compiled model without inequality rows, each in its own slice of batch-major buffers, one 256-thread workgroup
// per instance, grid (B).  An instance whose active flag is 0 is skipped: nothing of its slice is read or written.
// Every reduction runs in an order fixed by the model's sizes alone (strided per-thread partials, then block_reduce),
// so an instance's scalars do not depend on B or on which other instances are active.
//
// The errors at a point, the tape's inputs and the per-instance scaling of what a sweep wrote are the kernels of
// ipm_batch_kernels.h themselves (batch_errors_kernel, batch_load_state_kernel, batch_scale_V_kernel): with m_i = 0
// they compute exactly what these drivers read.
#pragma once

#include <hip/hip_runtime.h>

#include "device.hpp"
#include "ipm_batch_kernels.h"

namespace slpx {

// pointers of one batch's (x, y)-shaped buffers
struct EqIter {
  double *x, *y;
};

// The direction of a solve (sqp.hpp:305-346): d.x = p[0:n], d.y = -p[n:n+m_e] from the system's solution p
// ([b * dim]); out != nullptr: out[b] = D_phi = g . d.x (sqp.hpp:360, newton.hpp:197) with g of the current point's V.
__global__ __launch_bounds__(kBatchThreads) void eq_direction_kernel(KktDev K, const double* __restrict__ V, int v_stride,
                                                                     const double* __restrict__ p, EqIter d,
                                                                     const uint8_t* __restrict__ active,
                                                                     double* __restrict__ out) {
  __shared__ double scratch[kBatchThreads / 64 + 1];
  const int b = blockIdx.x;
  if (!active[b]) return;  // (uniform across the workgroup: no lane reaches the barriers below)
  const int n = K.n, m_e = K.m_e, tid = threadIdx.x;
  V += static_cast<size_t>(b) * v_stride;
  p += static_cast<size_t>(b) * K.dim;
  double* dx = d.x + static_cast<size_t>(b) * n;
  double* dy = d.y + static_cast<size_t>(b) * m_e;
  double acc[1] = {0.0};
  for (int i = tid; i < n; i += kBatchThreads) {
    const double pi = p[i];
    dx[i] = pi;
    const int gs = K.g_src[i];
    if (gs >= 0) acc[0] += V[gs] * pi;
  }
  for (int j = tid; j < m_e; j += kBatchThreads) dy[j] = -p[n + j];
  if (out == nullptr) return;  // (a kernel argument: uniform)
  const int ops[1] = {IPM_SUM};
  block_reduce<1, kBatchThreads>(acc, ops, scratch);
  if (tid == 0) out[b] = acc[0];
}

// Trial point (sqp.hpp:364-384, newton.hpp:201-205): (x, y) + alpha d with d the Newton direction (mode 0) or the
// correction's (mode 1) — y moves with the primal step size.  The trial x goes to the tape's inputs; with_duals: the
// trial y too (scaled by d_ce), for a full sweep.
struct EqTrialArgs {
  EqIter cur, trial, newton, soc;
  const int32_t* mode;
  const double* alpha;
  double* in;
  int in_stride;
  const double* S;
  int ns, with_duals;
};
__global__ __launch_bounds__(kBatchThreads) void eq_trial_kernel(KktDev K, EqTrialArgs A, const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e;
  const size_t bx = static_cast<size_t>(b) * n, be = static_cast<size_t>(b) * m_e;
  const EqIter d = A.mode[b] == 1 ? A.soc : A.newton;
  const double a = A.alpha[b];
  double* inb = A.in + static_cast<size_t>(b) * A.in_stride;
  const double* sc = A.S + static_cast<size_t>(b) * A.ns;
  for (int i = threadIdx.x; i < n; i += kBatchThreads) {
    const double t = A.cur.x[bx + i] + a * d.x[bx + i];
    A.trial.x[bx + i] = t;
    inb[i] = t;
  }
  for (int j = threadIdx.x; j < m_e; j += kBatchThreads) {
    const double t = A.cur.y[be + j] + a * d.y[be + j];
    A.trial.y[be + j] = t;
    if (A.with_duals) inb[n + j] = sc[1 + j] * t;
  }
}

// The trial point's numbers after a value sweep (V head scaled): out[b] = {f, ||c_e||_1, count of non-finite f, c_e};
// the trial c_e is kept (tce) for a correction that follows.
__global__ __launch_bounds__(kBatchThreads) void eq_trial_metrics_kernel(KktDev K, const double* __restrict__ V, int v_stride,
                                                                         double* __restrict__ tce,
                                                                         const uint8_t* __restrict__ active,
                                                                         double* __restrict__ out) {
  __shared__ double scratch[(kBatchThreads / 64 + 1) * 2];
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int m_e = K.m_e, tid = threadIdx.x;
  V += static_cast<size_t>(b) * v_stride;
  tce += static_cast<size_t>(b) * m_e;
  double acc[2] = {0.0, 0.0};  // violation, non-finite count
  for (int j = tid; j < m_e; j += kBatchThreads) {
    const double c = V[K.off_ce + j];
    tce[j] = c;
    acc[0] += fabs(c);
    if (!ipm_isfinite(c)) acc[1] += 1.0;
  }
  const int ops[2] = {IPM_SUM, IPM_SUM};
  block_reduce<2, kBatchThreads>(acc, ops, scratch);
  if (tid == 0) {
    const double f = V[K.off_f];
    out[3 * b + 0] = f;
    out[3 * b + 1] = acc[0];
    out[3 * b + 2] = acc[1] + (ipm_isfinite(f) ? 0.0 : 1.0);
  }
}

// Second-order correction, right-hand side (sqp.hpp:397-468) from the current point's V: first[b] starts the
// accumulation from c_e; then c_e_soc = alpha_soc c_e_soc + trial c_e, and rhs = [-g + A_e^T y | -c_e_soc].
struct EqSocArgs {
  const double* V;  // current point
  int v_stride;
  const double *y, *tce, *alpha_soc;
  const uint8_t* first;
  double *sce, *rhs;
};
__global__ __launch_bounds__(kBatchThreads) void eq_soc_rhs_kernel(KktDev K, EqSocArgs A, const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e, tid = threadIdx.x;
  const double* V = A.V + static_cast<size_t>(b) * A.v_stride;
  const size_t be = static_cast<size_t>(b) * m_e;
  const double as = A.alpha_soc[b];
  const bool first = A.first[b] != 0;
  double* rhs = A.rhs + static_cast<size_t>(b) * K.dim;
  for (int j = tid; j < m_e; j += kBatchThreads) {
    const double prev = first ? V[K.off_ce + j] : A.sce[be + j];
    const double c = as * prev + A.tce[be + j];
    A.sce[be + j] = c;
    rhs[n + j] = -c;
  }
  const double* Ae = V + K.off_Ae;
  const double* y = A.y + be;
  for (int c = tid; c < n; c += kBatchThreads) {
    const int gs = K.g_src[c];
    double acc = 0.0;  // (column c of A_e^T y, accumulated as add_At_v does)
    for (int q = K.ae_colptr[c]; q < K.ae_colptr[c + 1]; ++q) acc += Ae[q] * y[K.ae_rowidx[q]];
    rhs[c] = -(gs >= 0 ? V[gs] : 0.0) + acc;
  }
}

// Commit (sqp.hpp:558-560, newton.hpp:246): the trial point becomes the iterate.
__global__ __launch_bounds__(kBatchThreads) void eq_commit_kernel(KktDev K, EqIter trial, EqIter cur,
                                                                  const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int n = K.n, m_e = K.m_e;
  const size_t bx = static_cast<size_t>(b) * n, be = static_cast<size_t>(b) * m_e;
  for (int i = threadIdx.x; i < n; i += kBatchThreads) cur.x[bx + i] = trial.x[bx + i];
  for (int j = threadIdx.x; j < m_e; j += kBatchThreads) cur.y[be + j] = trial.y[be + j];
}

}  // namespace slpx
