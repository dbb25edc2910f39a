// Kernels of a batched warm start (batch_lockstep.cpp: set_initial_iterate and the results): the first iterate of every
// instance from a caller-given primal-dual iterate in the user's units, and the end iterate back in those units.  The
// formulas are the bodies of warm_start.h — the ones the single solve runs on the host.  As every kernel of this layer
// (ipm_batch_kernels.h): one 256-thread workgroup per instance, batch-major buffers, strided loops over the rows (m_e
// and m_i may each be 0 or larger than the workgroup), reductions in an order fixed by the model's sizes alone (strided
// per-thread partials, then block_reduce), so an instance's outputs do not depend on B, on its slot or on the mask; no
// atomics, and no workgroup waits for another.
#pragma once

#include <hip/hip_runtime.h>

#include "ipm_batch_kernels.h"
#include "warm_start.h"

namespace slpx {

constexpr int kWarmOutN = 3;  // per instance: the first barrier parameter (scaled), entries repaired, non-finite input

struct BatchWarmArgs {
  int n, m_e, m_i;
  const double *s0, *y0, *z0;  // [B][m_i], [B][m_e], [B][m_i], the user's units; null: absent
  const double* mu_in;         // [B][2]: the given barrier parameter (the user's units; <= 0: choose), mu_min
  const double* V;             // the sweep at x0 with unit scales: c_i of instance b at V[b * v_stride + off_ci ..]
  int v_stride, off_ci;
  const double* S;             // [B][ns] = [d_f | d_ce | d_ci]
  int ns;
  BatchIter cur;               // x is read (the non-finite test); s, y, z are written
  const uint8_t* run;          // [B] 0: the instance is skipped, every bit of its slices stays
  double* out;                 // [B][kWarmOutN]
};

// Safeguarded first iterate (warm_start.h, steps 1-5).  A non-finite input: out = {0, 0, 1} and nothing else is written.
// grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_warm_start_kernel(BatchWarmArgs A) {
  __shared__ double scratch[(kBatchThreads / 64 + 1) * 3];
  const int b = blockIdx.x;
  if (!A.run[b]) return;  // (uniform across the workgroup: no lane reaches the barriers below)
  const int tid = threadIdx.x;
  const int n = A.n, m_e = A.m_e, m_i = A.m_i;
  const double* sc = A.S + static_cast<size_t>(b) * A.ns;
  const double d_f = sc[0];
  const double* d_ce = sc + 1;
  const double* d_ci = sc + 1 + m_e;
  const double* x = A.cur.x + static_cast<size_t>(b) * n;
  const double* s0 = A.s0 ? A.s0 + static_cast<size_t>(b) * m_i : nullptr;
  const double* y0 = A.y0 ? A.y0 + static_cast<size_t>(b) * m_e : nullptr;
  const double* z0 = A.z0 ? A.z0 + static_cast<size_t>(b) * m_i : nullptr;
  const double mu_given = A.mu_in[2 * b], mu_min = A.mu_in[2 * b + 1];

  // ---- first pass: non-finite input; sum and count of s_j z_j over the rows where both are given and positive ----
  double acc[3] = {0.0, 0.0, 0.0};  // bad, sum, count
  if (tid == 0 && warm_bad(mu_given)) acc[0] += 1.0;
  for (int i = tid; i < n; i += kBatchThreads)
    if (warm_bad(x[i])) acc[0] += 1.0;
  if (y0)
    for (int j = tid; j < m_e; j += kBatchThreads)
      if (warm_bad(y0[j])) acc[0] += 1.0;
  for (int j = tid; j < m_i; j += kBatchThreads) {
    if (s0 && warm_bad(s0[j])) acc[0] += 1.0;
    if (z0 && warm_bad(z0[j])) acc[0] += 1.0;
    if (s0 && z0) {
      const double s = warm_scale_s(s0[j], d_ci[j]), z = warm_scale_dual(z0[j], d_ci[j], d_f);
      if (warm_counts(s, z)) {
        acc[1] += s * z;
        acc[2] += 1.0;
      }
    }
  }
  const int ops[3] = {IPM_SUM, IPM_SUM, IPM_SUM};
  block_reduce<3, kBatchThreads>(acc, ops, scratch);
  double* out = A.out + static_cast<size_t>(b) * kWarmOutN;
  if (acc[0] != 0.0) {  // (the total is in every lane: the workgroup leaves together)
    if (tid == 0) out[0] = 0.0, out[1] = 0.0, out[2] = 1.0;
    return;
  }
  const double mu = warm_mu(acc[1], acc[2], mu_given, d_f, mu_min);

  // ---- second pass: conversion, repair, clamp ----
  double* s_out = A.cur.s + static_cast<size_t>(b) * m_i;
  double* y_out = A.cur.y + static_cast<size_t>(b) * m_e;
  double* z_out = A.cur.z + static_cast<size_t>(b) * m_i;
  const double* c_i = A.V + static_cast<size_t>(b) * A.v_stride + A.off_ci;
  for (int j = tid; j < m_e; j += kBatchThreads) y_out[j] = y0 ? warm_scale_dual(y0[j], d_ce[j], d_f) : 0.0;
  int repaired = 0;
  for (int j = tid; j < m_i; j += kBatchThreads) {
    const double d = d_ci[j];
    const double s = warm_slack(s0 != nullptr, s0 ? warm_scale_s(s0[j], d) : 0.0, d * c_i[j], mu, &repaired);
    const double z = warm_dual(z0 != nullptr, z0 ? warm_scale_dual(z0[j], d, d_f) : 0.0, mu, s, &repaired);
    s_out[j] = s;
    z_out[j] = z;
  }
  double rep[1] = {static_cast<double>(repaired)};  // (a sum of small integers: exact in any order)
  const int op1[1] = {IPM_SUM};
  block_reduce<1, kBatchThreads>(rep, op1, scratch);
  if (tid == 0) out[0] = mu, out[1] = rep[0], out[2] = 0.0;
}

// The iterate of every instance with run[b] != 0 in the user's units (warm_start.h): su [B][m_i], yu [B][m_e],
// zu [B][m_i].  grid (B).
__global__ __launch_bounds__(kBatchThreads) void batch_unscale_iterate_kernel(int m_e, int m_i, BatchIter cur,
                                                                              const double* __restrict__ S, int ns,
                                                                              const uint8_t* __restrict__ run,
                                                                              double* __restrict__ su,
                                                                              double* __restrict__ yu,
                                                                              double* __restrict__ zu) {
  const int b = blockIdx.x;
  if (!run[b]) return;
  const double* sc = S + static_cast<size_t>(b) * ns;
  const double d_f = sc[0];
  const size_t be = static_cast<size_t>(b) * m_e, bi = static_cast<size_t>(b) * m_i;
  for (int j = threadIdx.x; j < m_e; j += kBatchThreads) yu[be + j] = warm_unscale_dual(cur.y[be + j], sc[1 + j], d_f);
  for (int j = threadIdx.x; j < m_i; j += kBatchThreads) {
    const double d = sc[1 + m_e + j];
    su[bi + j] = warm_unscale_s(cur.s[bi + j], d);
    zu[bi + j] = warm_unscale_dual(cur.z[bi + j], d, d_f);
  }
}

}  // namespace slpx
