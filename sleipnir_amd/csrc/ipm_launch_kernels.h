// The __global__ entry points of the interior-point iteration (their bodies and everything the riding error
// workgroups of the step kernel share with them: ipm_kernels.h).  Non-template kernels: a file that includes this
// header gets a copy of each, so kernels.hip — which launches them — is the only one that does.
#pragma once

#include "ipm_kernels.h"

namespace slpx {

// Step sizes and directional derivative for the direction (p, ps, pz), then the first trial
// point x + alpha_max p_x.  `out` (pinned host) and `alpha_dev` (device copy, read by
// ipm_trial_metrics_kernel of the same speculative chain) may be the only consumers.
__global__ __launch_bounds__(kIpmThreads) void ipm_direction_kernel(
    KktDev K, const double* __restrict__ V, const double* __restrict__ x, const double* __restrict__ s,
    const double* __restrict__ z, const double* __restrict__ p, const double* __restrict__ ps,
    const double* __restrict__ pz, const double* __restrict__ mu_dev, double tau, double* __restrict__ trial_x,
    double* __restrict__ alpha_dev, IpmDirOut* __restrict__ out) {
  __shared__ double scratch[17 * 3];
  const int tid = threadIdx.x;
  const double mu = mu_dev[0];
  double acc[3] = {1.0, 1.0, 0.0};  // alpha_max, alpha_z, D_phi
  for (int r = tid; r < K.m_i; r += kIpmThreads) {
    const double sr = s[r], psr = ps[r], zr = z[r], pzr = pz[r];
    acc[0] = ftb_candidate(acc[0], tau, psr, sr);
    acc[1] = ftb_candidate(acc[1], tau, pzr, zr);
    acc[2] -= mu * ((1.0 / sr) * psr);
  }
  for (int j = tid; j < K.n; j += kIpmThreads) {
    const int gs = K.g_src[j];
    if (gs >= 0) acc[2] += V[gs] * p[j];
  }
  const int ops[3] = {IPM_MIN, IPM_MIN, IPM_SUM};
  block_reduce<3, kIpmThreads>(acc, ops, scratch);
  const double alpha = acc[0];
  for (int j = tid; j < K.n; j += kIpmThreads) trial_x[j] = x[j] + alpha * p[j];
  if (tid == 0) {
    alpha_dev[0] = acc[0];
    alpha_dev[1] = acc[1];
    out->alpha_max = acc[0];
    out->alpha_z = acc[1];
    out->D_phi = acc[2];
  }
}

__global__ __launch_bounds__(kIpmThreads) void ipm_lookahead_kernel(IpmLookaheadArgs A) {
  __shared__ double scratch[17 * 3];
  ipm_lookahead_body<kIpmThreads>(A, scratch);
}

// trial_x = x + alpha p_x (backtracking)
__global__ __launch_bounds__(256) void ipm_trial_point_kernel(int n, const double* __restrict__ x,
                                                              const double* __restrict__ p, double alpha,
                                                              double* __restrict__ trial_x) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    trial_x[j] = x[j] + alpha * p[j];
}

// Filter quantities of the trial point whose f, c_e, c_i a forward sweep left in Vt.
// alpha < 0: take the step size from alpha_dev[0].  s_from_ci: trial_s = trial c_i
// (feasible-IPM option, interior_point.hpp:520-526).
// The separable sums the forward sweep left as partial terms (the cost: one term per stage
// group) are finished here (separable_sum_tree) instead of by a launch of their own between
// the sweep and this kernel.
__global__ __launch_bounds__(kIpmThreads) void ipm_trial_metrics_kernel(
    KktDev K, double* __restrict__ Vt, const double* __restrict__ s, const double* __restrict__ ps,
    double alpha, const double* __restrict__ alpha_dev, int s_from_ci, IpmTrialOut* __restrict__ out,
    unsigned long long* __restrict__ seq_dev, volatile unsigned long long* seq_host,
    const NlpStructure::SumReduce* __restrict__ red, int n_red, const double* __restrict__ scales) {
  __shared__ double scratch[17 * 3];
  __shared__ double part[64];
  const int tid = threadIdx.x;
  for (int q = 0; q < n_red; ++q) {
    const NlpStructure::SumReduce r = red[q];
    separable_sum_tree(Vt, r, part, tid);
    if (tid == 0) Vt[r.dst] = separable_sum_scale(r, scales) * part[0];
    __syncthreads();
  }
  if (alpha < 0.0) alpha = alpha_dev[0];
  double acc[3] = {0.0, 0.0, 1.0};  // violation, log sum, finite
  for (int r = tid; r < K.m_e; r += kIpmThreads) {
    const double c = Vt[K.off_ce + r];
    acc[0] += fabs(c);
    if (!isfinite(c)) acc[2] = 0.0;
  }
  for (int r = tid; r < K.m_i; r += kIpmThreads) {
    const double c = Vt[K.off_ci + r];
    const double st = s_from_ci ? c : s[r] + alpha * ps[r];
    acc[0] += fabs(c - st);
    acc[1] += log(st);
    if (!isfinite(c)) acc[2] = 0.0;
  }
  const int ops[3] = {IPM_SUM, IPM_SUM, IPM_MIN};
  block_reduce<3, kIpmThreads>(acc, ops, scratch);
  if (tid == 0) {
    const double f = Vt[K.off_f];
    out->f = f;
    out->viol = acc[0];
    out->logsum = acc[1];
    out->finite = (acc[2] != 0.0 && isfinite(f)) ? 1.0 : 0.0;
    ipm_publish(seq_dev, seq_host);
  }
}

// Accepts the step: x += alpha p_x, s += alpha p_s (or s = trial c_i), y += alpha_z p_y with
// p_y = −p[n:], z += alpha_z p_z, then the z reset of interior_point.hpp:797-801.  x, y, z
// also live in the tape's input vector `in` = [x | y | z].
__global__ __launch_bounds__(256) void ipm_commit_kernel(KktDev K, const double* __restrict__ Vt,
                                                         const double* __restrict__ p,
                                                         const double* __restrict__ ps,
                                                         const double* __restrict__ pz, double alpha,
                                                         double alpha_z, const double* __restrict__ mu_dev,
                                                         int s_from_ci, double* __restrict__ in,
                                                         double* __restrict__ s, double* __restrict__ y,
                                                         double* __restrict__ z) {
  const double mu = mu_dev[0];
  const int stride = gridDim.x * blockDim.x;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (int j = t0; j < K.n; j += stride) in[j] = in[j] + alpha * p[j];
  for (int r = t0; r < K.m_e; r += stride) {
    const double v = y[r] + alpha_z * (-p[K.n + r]);
    y[r] = v;
    in[K.n + r] = v;
  }
  for (int r = t0; r < K.m_i; r += stride) {
    const double sn = s_from_ci ? Vt[K.off_ci + r] : s[r] + alpha * ps[r];
    const double zn = z_reset(z[r] + alpha_z * pz[r], mu, sn);
    s[r] = sn;
    z[r] = zn;
    in[K.n + K.m_e + r] = zn;
  }
}

// (p, p_s, p_z) -> their keep buffers or back, in ONE launch (three device-to-device copies through the
// runtime cost ~5 us each on the stream)
__global__ __launch_bounds__(256) void ipm_copy_direction_kernel(int dim, int m_i, const double* __restrict__ p,
                                                                 const double* __restrict__ ps, const double* __restrict__ pz,
                                                                 double* __restrict__ p_to, double* __restrict__ ps_to,
                                                                 double* __restrict__ pz_to) {
  const int stride = gridDim.x * blockDim.x;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (int j = t0; j < dim; j += stride) p_to[j] = p[j];
  for (int r = t0; r < m_i; r += stride) {
    ps_to[r] = ps[r];
    pz_to[r] = pz[r];
  }
}

// Second-order correction accumulators (interior_point.hpp:590-600):
//   c_e_soc = alpha c_e_soc + trial c_e,  (c_i − s)_soc = alpha (c_i − s)_soc + trial c_i − trial s
// first != 0: start from the current c_e, c_i − s (in V).
__global__ __launch_bounds__(256) void ipm_soc_accumulate_kernel(KktDev K, const double* __restrict__ V,
                                                                 const double* __restrict__ Vt,
                                                                 const double* __restrict__ s,
                                                                 const double* __restrict__ ps, double alpha,
                                                                 int first, int s_from_ci,
                                                                 double* __restrict__ soc_ce,
                                                                 double* __restrict__ soc_cims) {
  const int stride = gridDim.x * blockDim.x;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (int r = t0; r < K.m_e; r += stride) {
    const double prev = first ? V[K.off_ce + r] : soc_ce[r];
    soc_ce[r] = soc_accumulate(alpha, prev, Vt[K.off_ce + r]);
  }
  for (int r = t0; r < K.m_i; r += stride) {
    const double prev = first ? V[K.off_ci + r] - s[r] : soc_cims[r];
    const double ct = Vt[K.off_ci + r];
    const double st = s_from_ci ? ct : s[r] + alpha * ps[r];
    soc_cims[r] = soc_accumulate(alpha, prev, ct) - st;
  }
}

// Right-hand side of a second-order correction (interior_point.hpp:611-616):
//   [−g + A_eᵀ y + A_iᵀ (μ/s − Σ (c_i − s)_soc);  −c_e_soc]
__global__ __launch_bounds__(256) void ipm_soc_rhs_kernel(KktDev K, const double* __restrict__ V,
                                                          const double* __restrict__ s,
                                                          const double* __restrict__ y,
                                                          const double* __restrict__ z,
                                                          const double* __restrict__ mu_dev,
                                                          const double* __restrict__ soc_ce,
                                                          const double* __restrict__ soc_cims,
                                                          double* __restrict__ rhs) {
  const double m = mu_dev[0];
  const double* Ae = V + K.off_Ae;
  const double* Ai = V + K.off_Ai;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < K.dim; j += gridDim.x * blockDim.x) {
    if (j >= K.n) {
      rhs[j] = -soc_ce[j - K.n];
      continue;
    }
    const int gs = K.g_src[j];
    double acc = -(gs >= 0 ? V[gs] : 0.0);
    double aey = 0.0;
    for (int q = K.ae_colptr[j]; q < K.ae_colptr[j + 1]; ++q) aey += Ae[q] * y[K.ae_rowidx[q]];
    acc += aey;
    double ait = 0.0;
    for (int q = K.ai_colptr[j]; q < K.ai_colptr[j + 1]; ++q) {
      const int r = K.ai_rowidx[q];
      ait += Ai[q] * soc_rhs_multiplier(m, s[r], z[r], soc_cims[r]);
    }
    rhs[j] = acc + ait;
  }
}

// p_s, p_z of a second-order correction (interior_point.hpp:625-630): the back-substitution
// with (c_i − s)_soc in place of c_i − s.
__global__ __launch_bounds__(256) void ipm_soc_backsub_kernel(KktDev K, const double* __restrict__ V,
                                                              const double* __restrict__ p,
                                                              const double* __restrict__ s,
                                                              const double* __restrict__ z,
                                                              const double* __restrict__ mu_dev,
                                                              const double* __restrict__ soc_cims,
                                                              double* __restrict__ ps, double* __restrict__ pz) {
  const double m = mu_dev[0];
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < K.m_i; r += gridDim.x * blockDim.x) {
    double aipx = 0.0;
    for (int q = K.ai_rowptr[r]; q < K.ai_rowptr[r + 1]; ++q) aipx += V[K.ai_src[q]] * p[K.ai_col[q]];
    const double sinv = 1.0 / s[r];
    const double p_s = soc_cims[r] + aipx;
    ps[r] = p_s;
    pz[r] = backsub_pz_sinv(m, sinv, z[r], p_s);
  }
}

__global__ __launch_bounds__(kIpmErrThreads) void ipm_error_partial_kernel(
    KktDev K, const double* __restrict__ V, int nV, const double* __restrict__ x,
    const double* __restrict__ s, const double* __restrict__ y, const double* __restrict__ z,
    const double* __restrict__ scales, int check_all_V, double* __restrict__ partial, IpmErrFinish fin) {
  __shared__ double lds[kIpmErrLdsDoubles];
  if (fin.skip != nullptr && fin.skip[0] != 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (fin.ctl != nullptr) {  // (a void chain decides nothing: whatever was enqueued behind it passes too)
        fin.ctl->go = 0;
        *fin.gate = 0.0;
        if (fin.go_host != nullptr) *fin.go_host = 0.0;
      }
      ipm_publish(fin.seq_dev, fin.seq_host);
    }
    return;
  }
  ipm_error_block(K, V, nV, x, s, y, z, scales, check_all_V, partial, fin, static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x), lds);
}

__global__ __launch_bounds__(256) void ipm_error_final_kernel(KktDev K, const double* __restrict__ V,
                                                             const double* __restrict__ partial, int n_blocks,
                                                             IpmErrOut* __restrict__ out,
                                                             unsigned long long* __restrict__ seq_dev,
                                                             volatile unsigned long long* seq_host) {
  __shared__ double tot[9 * kIpmErrQ];
  ipm_error_fold(K, V, partial, n_blocks, false, out, seq_dev, seq_host, tot);
}

}  // namespace slpx
