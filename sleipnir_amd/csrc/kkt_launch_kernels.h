// The __global__ entry points of the KKT system outside the factorization: assembly, right-hand side, the step's
// back-substitution and the residual of the plain refinement (their bodies, shared with the factorization kernels:
// kkt_kernels.h).  Non-template kernels mostly: a file that includes this header gets a copy of each, so kernels.hip —
// which launches them — is the only one that does.
#pragma once

#include "device_base.hpp"
#include "device_layout.h"
#include "ipm_reduce.h"
#include "kkt_kernels.h"

namespace slpx {

// ============================================================================
// kkt_assemble / kkt_rhs / step_backsub: pure gathers over static index maps.
// HBM-bound; algorithmic bytes: assemble 12(h+a+i) + 16 m_i + 8 k, rhs
// 16 n + 24 m_e + 24 m_i + 12(a+i).  One thread per output entry,
// consecutive threads write consecutive entries; the sources of consecutive lhs
// entries are (nearly) consecutive in V because both are CSC-ordered.
// ============================================================================
__global__ __launch_bounds__(256) void kkt_assemble_kernel(KktDev K, const double* __restrict__ V,
                                                           int v_stride,
                                                           const double* __restrict__ s,
                                                           const double* __restrict__ z,
                                                           double* __restrict__ lhs) {
  const int b = blockIdx.y;
  kkt_assemble_body(K, V + static_cast<size_t>(b) * v_stride, s + static_cast<size_t>(b) * K.m_i,
                    z + static_cast<size_t>(b) * K.m_i, lhs + static_cast<size_t>(b) * K.nnz_lhs, blockIdx.x,
                    gridDim.x);
}

// Batch variant: one thread serves the SAME entry of kBatchPerThread consecutive problems,
// so every index of the static maps (fast_src, dptr/dsrc, pptr/pa/pb/pr) is fetched once per
// kBatchPerThread problems instead of once per problem — the maps are a fifth of the bytes
// a thread touches — and the problems' gathers are in flight together.
constexpr int kBatchPerThread = 4;

template <int P>
__global__ __launch_bounds__(256) void kkt_assemble_batch_kernel(KktDev K, const double* __restrict__ V,
                                                                 int v_stride,
                                                                 const double* __restrict__ s,
                                                                 const double* __restrict__ z,
                                                                 double* __restrict__ lhs, int batch) {
  const int b0 = blockIdx.y * P;
  const int nb = min(P, batch - b0);
  V += static_cast<size_t>(b0) * v_stride;
  s += static_cast<size_t>(b0) * K.m_i;
  z += static_cast<size_t>(b0) * K.m_i;
  lhs += static_cast<size_t>(b0) * K.nnz_lhs;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K.nnz_lhs; k += gridDim.x * blockDim.x) {
    const int f = K.fast_src[k];
    double v[P];
#pragma unroll
    for (int q = 0; q < P; ++q) v[q] = 0.0;
    if (f >= 0) {
#pragma unroll
      for (int q = 0; q < P; ++q)
        if (q < nb) v[q] = V[static_cast<size_t>(q) * v_stride + f];
    } else if (f == -2) {
      double prod[P];
#pragma unroll
      for (int q = 0; q < P; ++q) prod[q] = 0.0;
      for (int d = K.dptr[k]; d < K.dptr[k + 1]; ++d) {
        const int src = K.dsrc[d];
#pragma unroll
        for (int q = 0; q < P; ++q)
          if (q < nb) v[q] += V[static_cast<size_t>(q) * v_stride + src];
      }
      for (int p = K.pptr[k]; p < K.pptr[k + 1]; ++p) {
        const int r = K.pr[p], a = K.pa[p], bb = K.pb[p];
#pragma unroll
        for (int q = 0; q < P; ++q)
          if (q < nb) {
            const double* Vq = V + static_cast<size_t>(q) * v_stride;
            prod[q] += kkt_prod_term(Vq[a], s[q * K.m_i + r], z[q * K.m_i + r], Vq[bb]);
          }
      }
#pragma unroll
      for (int q = 0; q < P; ++q) v[q] += prod[q];
    }
#pragma unroll
    for (int q = 0; q < P; ++q)
      if (q < nb) lhs[static_cast<size_t>(q) * K.nnz_lhs + k] = v[q];
  }
}

// The batch-interleaved factorization's inputs written WHERE IT READS THEM (ldlt_il_kernels.h:
// [b / 16][entry][16]) — the batch-major lhs / rhs and the two transposing launches between the
// assembly and the factorization (il_gather_kernel: 0.084 ms of a 1.15 ms step at 512 x N=1000) are
// only made when somebody asks for them (DeviceNlp::d_lhs / d_rhs).
// lhs: a thread = one entry of FOUR consecutive problems, four adjacent lanes = the 16 problems of
// the entry's row: every 128-byte row is written whole by one quad, and a wave's loads of one
// problem's V are sixteen consecutive entries' sources.
__device__ __forceinline__ void kkt_assemble_il_body(const KktDev& K, const double* __restrict__ V, int v_stride,
                                                     const double* __restrict__ s, const double* __restrict__ z,
                                                     double* __restrict__ lhs_il, int batch, int vblock, int vgrid) {
  constexpr int P = 4;
  const int g = blockIdx.y, sub = threadIdx.x & 3;
  const int b0 = g * kIlW + sub * P;
  const int nb = max(0, min(P, batch - b0));
  const size_t bb0 = static_cast<size_t>(nb > 0 ? b0 : 0);  // (no problem of this quad exists: nothing is dereferenced)
  V += bb0 * v_stride;
  s += bb0 * K.m_i;
  z += bb0 * K.m_i;
  double* out = lhs_il + static_cast<size_t>(g) * K.nnz_lhs * kIlW + sub * P;
  for (int k = vblock * 64 + (threadIdx.x >> 2); k < K.nnz_lhs; k += vgrid * 64) {
    const int f = K.fast_src[k];
    double v[P];
#pragma unroll
    for (int q = 0; q < P; ++q) v[q] = 0.0;
    if (f >= 0) {
#pragma unroll
      for (int q = 0; q < P; ++q)
        if (q < nb) v[q] = V[static_cast<size_t>(q) * v_stride + f];
    } else if (f == -2) {
      double prod[P];
#pragma unroll
      for (int q = 0; q < P; ++q) prod[q] = 0.0;
      for (int d = K.dptr[k]; d < K.dptr[k + 1]; ++d) {
        const int src = K.dsrc[d];
#pragma unroll
        for (int q = 0; q < P; ++q)
          if (q < nb) v[q] += V[static_cast<size_t>(q) * v_stride + src];
      }
      for (int p = K.pptr[k]; p < K.pptr[k + 1]; ++p) {
        const int r = K.pr[p], a = K.pa[p], c = K.pb[p];
#pragma unroll
        for (int q = 0; q < P; ++q)
          if (q < nb) {
            const double* Vq = V + static_cast<size_t>(q) * v_stride;
            prod[q] += kkt_prod_term(Vq[a], s[q * K.m_i + r], z[q * K.m_i + r], Vq[c]);
          }
      }
#pragma unroll
      for (int q = 0; q < P; ++q) v[q] += prod[q];
    }
    double2* o = reinterpret_cast<double2*>(out + static_cast<size_t>(k) * kIlW);
    o[0] = double2{v[0], v[1]};
    o[1] = double2{v[2], v[3]};
  }
}

__global__ __launch_bounds__(256) void kkt_assemble_il_kernel(KktDev K, const double* __restrict__ V, int v_stride,
                                                              const double* __restrict__ s, const double* __restrict__ z,
                                                              double* __restrict__ lhs_il, int batch) {
  kkt_assemble_il_body(K, V, v_stride, s, z, lhs_il, batch, blockIdx.x, gridDim.x);
}

// rhs: 64 rows x 16 problems per workgroup through LDS — a row is computed by one lane per problem
// group of four (consecutive lanes = consecutive rows: the row's sources in V are nearly consecutive),
// written as whole 128-byte rows.
__device__ __forceinline__ void kkt_rhs_il_body(const KktDev& K, const double* __restrict__ V, int v_stride,
                                                const double* __restrict__ s, const double* __restrict__ y,
                                                const double* __restrict__ z, const double* __restrict__ mu,
                                                double* __restrict__ rhs_il, int batch, int vblock) {
  __shared__ double tile[kIlW][65];
  const int g = blockIdx.y, i0 = vblock * 64;
  const int il = threadIdx.x & 63, bq = threadIdx.x >> 6;
  const int j = i0 + il;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int pl = bq * 4 + q, b = g * kIlW + pl;
    double val = 0.0;
    if (b < batch && j < K.dim) {
      const size_t sb = static_cast<size_t>(b);
      val = kkt_rhs_entry(K, V + sb * v_stride, s + sb * K.m_i, y + sb * K.m_e, z + sb * K.m_i, mu[b], j);
    }
    tile[pl][il] = val;
  }
  __syncthreads();
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int idx = threadIdx.x + 256 * jj, pl = idx & (kIlW - 1), r = idx >> kIlWShift;
    if (i0 + r < K.dim) rhs_il[(static_cast<size_t>(g) * K.dim + i0 + r) * kIlW + pl] = tile[pl][r];
  }
}
__global__ __launch_bounds__(256) void kkt_rhs_il_kernel(KktDev K, const double* __restrict__ V, int v_stride,
                                                         const double* __restrict__ s, const double* __restrict__ y,
                                                         const double* __restrict__ z, const double* __restrict__ mu,
                                                         double* __restrict__ rhs_il, int batch) {
  kkt_rhs_il_body(K, V, v_stride, s, y, z, mu, rhs_il, batch, blockIdx.x);
}
// lhs and rhs in ONE launch (a Newton step builds both: neither reads the other's output) — workgroups
// [0, na) assemble, the rest take 64 rows of the right-hand side each.  A small batch's two launches are
// latency each (64 x N=500: 15 + 16 us); side by side they cost the longer one.
__global__ __launch_bounds__(256) void kkt_build_il_kernel(KktDev K, const double* __restrict__ V, int v_stride,
                                                           const double* __restrict__ s, const double* __restrict__ y,
                                                           const double* __restrict__ z, const double* __restrict__ mu,
                                                           double* __restrict__ lhs_il, double* __restrict__ rhs_il, int batch,
                                                           int na) {
  if (static_cast<int>(blockIdx.x) < na) kkt_assemble_il_body(K, V, v_stride, s, z, lhs_il, batch, blockIdx.x, na);
  else kkt_rhs_il_body(K, V, v_stride, s, y, z, mu, rhs_il, batch, static_cast<int>(blockIdx.x) - na);
}

// Least-squares multiplier estimate (util/lagrange_multiplier_estimate.hpp:56-133) on the
// KKT pattern: the top-left block is I + A_i^T S^-2 A_i (H sources skipped, identity added
// by kkt_add_identity_kernel), the A_e block is unchanged.
__global__ __launch_bounds__(256) void kkt_assemble_lsq_kernel(KktDev K, const double* __restrict__ V,
                                                               int v_stride,
                                                               const double* __restrict__ s,
                                                               double* __restrict__ lhs) {
  const int b = blockIdx.y;
  V += static_cast<size_t>(b) * v_stride;
  s += static_cast<size_t>(b) * K.m_i;
  lhs += static_cast<size_t>(b) * K.nnz_lhs;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K.nnz_lhs; k += gridDim.x * blockDim.x) {
    double direct = 0.0;
    for (int d = K.dptr[k]; d < K.dptr[k + 1]; ++d) {
      const int src = K.dsrc[d];
      if (src >= K.off_Ae && src < K.off_Ai) direct += V[src];
    }
    double prod = 0.0;
    for (int p = K.pptr[k]; p < K.pptr[k + 1]; ++p) {
      const double sinv = 1.0 / s[K.pr[p]];
      prod += (V[K.pa[p]] * (sinv * sinv)) * V[K.pb[p]];
    }
    lhs[k] = direct + prod;
  }
}

__global__ __launch_bounds__(256) void kkt_add_identity_kernel(KktDev K, const int32_t* __restrict__ diag_pos,
                                                               double* __restrict__ lhs) {
  lhs += static_cast<size_t>(blockIdx.y) * K.nnz_lhs;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < K.n; j += gridDim.x * blockDim.x)
    lhs[diag_pos[j]] += 1.0;
}

__global__ __launch_bounds__(256) void kkt_rhs_kernel(KktDev K, const double* __restrict__ V,
                                                      int v_stride, const double* __restrict__ s,
                                                      const double* __restrict__ y,
                                                      const double* __restrict__ z,
                                                      const double* __restrict__ mu,
                                                      double* __restrict__ rhs) {
  const int b = blockIdx.y;
  kkt_rhs_body(K, V + static_cast<size_t>(b) * v_stride, s + static_cast<size_t>(b) * K.m_i,
               y + static_cast<size_t>(b) * K.m_e, z + static_cast<size_t>(b) * K.m_i, mu[b],
               rhs + static_cast<size_t>(b) * K.dim, blockIdx.x, gridDim.x);
}

// lhs, rhs and the separable-sum reductions of the tape in ONE launch: all three only read
// what the sweep left in V, none reads another's output (the sums feed f, which nothing in
// the Newton step consumes).  Block ranges: [0, na) assembly, [na, na + nr) right-hand
// side, the rest one reduction each.
__global__ __launch_bounds__(256) void kkt_build_kernel(KktDev K, double* __restrict__ V, int v_stride,
                                                        const double* __restrict__ s,
                                                        const double* __restrict__ y,
                                                        const double* __restrict__ z,
                                                        const double* __restrict__ mu,
                                                        double* __restrict__ lhs, double* __restrict__ rhs,
                                                        int na, int nr,
                                                        const NlpStructure::SumReduce* __restrict__ red,
                                                        const double* __restrict__ scales) {
  __shared__ double part[64];
  const int b = blockIdx.y;
  V += static_cast<size_t>(b) * v_stride;
  s += static_cast<size_t>(b) * K.m_i;
  z += static_cast<size_t>(b) * K.m_i;
  const int blk = blockIdx.x;
  if (blk < na) {
    kkt_assemble_body(K, V, s, z, lhs + static_cast<size_t>(b) * K.nnz_lhs, blk, na);
  } else if (blk < na + nr) {
    kkt_rhs_body(K, V, s, y + static_cast<size_t>(b) * K.m_e, z, mu[b], rhs + static_cast<size_t>(b) * K.dim,
                 blk - na, nr);
  } else {
    const NlpStructure::SumReduce r = red[blk - na - nr];
    const int tid = threadIdx.x;
    separable_sum_tree(V, r, part, tid);
    if (tid == 0) V[r.dst] = separable_sum_scale(r, scales) * part[0];
  }
}

__global__ __launch_bounds__(256) void step_backsub_kernel(KktDev K, const double* __restrict__ V,
                                                           int v_stride,
                                                           const double* __restrict__ p,
                                                           const double* __restrict__ s,
                                                           const double* __restrict__ z,
                                                           const double* __restrict__ mu,
                                                           double* __restrict__ ps,
                                                           double* __restrict__ pz,
                                                           const LdltStats* __restrict__ stats_src,
                                                           LdltStats* __restrict__ stats_host,
                                                           unsigned long long* __restrict__ seq_dev,
                                                           volatile unsigned long long* seq_host) {
  const int b = blockIdx.y;
  // last kernel of a step: hand the inertia counters of the factorization to the host
  // (pinned memory) instead of spending a copy node on them; with one problem also a
  // sequence number the host spins on — it learns of the result a few microseconds before
  // the stream would report the kernel complete, and what it does next (another attempt or
  // the next step) is ordered behind this kernel by the stream anyway
  if (stats_host != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    stats_host[b] = stats_src[b];
    if (seq_host != nullptr) {
      __threadfence_system();
      const unsigned long long v = *seq_dev + 1;
      *seq_dev = v;
      *seq_host = v;
    }
  }
  V += static_cast<size_t>(b) * v_stride;
  p += static_cast<size_t>(b) * K.dim;
  s += static_cast<size_t>(b) * K.m_i;
  z += static_cast<size_t>(b) * K.m_i;
  ps += static_cast<size_t>(b) * K.m_i;
  pz += static_cast<size_t>(b) * K.m_i;
  step_backsub_body(K, V, p, s, z, mu[b], ps, pz, static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x),
                    static_cast<int>(gridDim.x * blockDim.x));
}

// Iterative refinement of a solve (used where the regularization would otherwise show in the
// answer: the least-squares multiplier estimate): r = b - K p for the UNREGULARIZED symmetric K
// given by its lower CSC values in `lhs`.  One thread per row i: the column i of the lower
// triangle gives K(r, i), r >= i, and a row index of the same triangle (rowptr / rowent / rowcol)
// gives K(i, c), c < i — a fixed order of summation, so the same bits on every run (scattering
// the mirrored half with floating-point atomics made the multiplier estimate, and with it the
// whole trajectory of a solve, differ from run to run in the last bits).
__global__ __launch_bounds__(256) void sym_residual_kernel(int dim, const int32_t* __restrict__ colptr,
                                                           const int32_t* __restrict__ rowidx,
                                                           const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ rowent,
                                                           const int32_t* __restrict__ rowcol,
                                                           const double* __restrict__ lhs,
                                                           const double* __restrict__ p,
                                                           double* __restrict__ res) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < dim; i += gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int q = rowptr[i]; q < rowptr[i + 1]; ++q) acc += lhs[rowent[q]] * p[rowcol[q]];  // K(i, c), c < i
    for (int q = colptr[i]; q < colptr[i + 1]; ++q) acc += lhs[q] * p[rowidx[q]];          // K(r, i), r >= i
    res[i] -= acc;
  }
}
__global__ __launch_bounds__(256) void axpy_kernel(int count, const double* __restrict__ x, double* __restrict__ y) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) y[i] += x[i];
}

}  // namespace slpx
