// The residual of a solve and the device side of its iterative refinement (DeviceNlp::residual and refine_*; the
// loop is NewtonSystem::refine, newton.cpp).  Opt-in: nothing on the path of a Newton step or a solve comes here, and
// the row map and the buffers below are made on the first call.
//
// kkt_residual_kernel: one lane per (row, problem), grid (ceil(dim / 256), batch); the arithmetic and its order are
// row_residual() of kkt_residual.h, the body the CPU tests run.  A lane reads only its own problem's slices of the
// batch-major lhs / rhs / p and that problem's (delta, gamma), so r of a problem has the same bits at any batch size,
// in any slot and under any mask.  The norm is max |r_i| taken on the BIT PATTERNS of |r_i| (abs_bits): an integer
// maximum does not depend on the order it is taken in, and a NaN — above +Inf as an integer — cannot be dropped the way
// fmax drops it.  Every workgroup leaves its maximum in a slot of its own; kkt_residual_norm_kernel folds a problem's
// slots.  Plain vector loads and stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "device.hpp"
#include "kkt_residual.h"

namespace slpx {

constexpr int kResidualThreads = 256;

// max over the workgroup of `bits`, returned by thread 0
__device__ inline unsigned long long block_max_bits(unsigned long long bits, unsigned long long* part, int threads) {
  const int tid = static_cast<int>(threadIdx.x);
  part[tid] = bits;
  __syncthreads();
  for (int w = threads / 2; w > 0; w >>= 1) {
    if (tid < w && part[tid + w] > part[tid]) part[tid] = part[tid + w];
    __syncthreads();
  }
  return part[0];
}

__global__ __launch_bounds__(kResidualThreads) void kkt_residual_kernel(int dim, int n_dec, int nnz, const int32_t* __restrict__ rowptr,
                                                                        const int32_t* __restrict__ ent, const int32_t* __restrict__ col,
                                                                        const double* __restrict__ lhs, const double* __restrict__ rhs,
                                                                        const double* __restrict__ p, const double* __restrict__ reg,
                                                                        const uint8_t* __restrict__ mask, double* __restrict__ res,
                                                                        unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long part[kResidualThreads];
  const int b = static_cast<int>(blockIdx.y);
  if (mask[b] == 0) return;  // (the whole workgroup: r, the partial maxima and the norm of this problem stay as they are)
  const int row = static_cast<int>(blockIdx.x) * kResidualThreads + static_cast<int>(threadIdx.x);
  unsigned long long bits = 0;
  if (row < dim) {
    const size_t at = static_cast<size_t>(b) * dim;
    const double r = row_residual(row, rowptr, ent, col, lhs + static_cast<size_t>(b) * nnz, p + at, rhs[at + row], n_dec, reg[2 * b],
                                  reg[2 * b + 1]);
    res[at + row] = r;
    bits = abs_bits(r);
  }
  const unsigned long long m = block_max_bits(bits, part, kResidualThreads);
  if (threadIdx.x == 0) partial[static_cast<size_t>(b) * gridDim.x + blockIdx.x] = m;
}

__global__ __launch_bounds__(64) void kkt_residual_norm_kernel(int n_part, const unsigned long long* __restrict__ partial,
                                                               const uint8_t* __restrict__ mask, unsigned long long* __restrict__ norm_bits) {
  __shared__ unsigned long long part[64];
  const int b = static_cast<int>(blockIdx.x);
  if (mask[b] == 0) return;
  unsigned long long bits = 0;
  for (int k = static_cast<int>(threadIdx.x); k < n_part; k += 64) {
    const unsigned long long v = partial[static_cast<size_t>(b) * n_part + k];
    if (v > bits) bits = v;
  }
  const unsigned long long m = block_max_bits(bits, part, 64);
  if (threadIdx.x == 0) norm_bits[b] = m;
}

// Row-local: p = kept p + d where the problem's flag says so, the kept p elsewhere (the triangular solves wrote every
// problem's slice of p: a problem that takes no step gets its solution back to the bit).
__global__ __launch_bounds__(256) void refine_accept_kernel(int dim, const double* __restrict__ keep, const double* __restrict__ d,
                                                            const uint8_t* __restrict__ accept, double* __restrict__ p) {
  const int b = static_cast<int>(blockIdx.y);
  const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (i >= dim) return;
  const size_t at = static_cast<size_t>(b) * dim + i;
  p[at] = accept[b] ? keep[at] + d[at] : keep[at];
}

void DeviceNlp::residual_buffers() {
  if (m_rm_rowptr.n != 0) return;
  const int dim = m_kdev.dim, B = m_batch;
  const int n_part = (dim + kResidualThreads - 1) / kResidualThreads;
  const KktRowMap map = build_kkt_row_map(m_k_ref.lhs);
  m_rm_rowptr.upload(map.rowptr);
  m_rm_ent.upload(map.ent);
  m_rm_col.upload(map.col);
  m_res.alloc(static_cast<size_t>(B) * dim);
  m_res.zero(m_stream);
  m_res_reg.alloc(2 * static_cast<size_t>(B));
  m_res_mask.alloc(B);
  m_res_partial.alloc(static_cast<size_t>(B) * n_part);
  m_res_norm.alloc(B);
  m_res_norm.zero(m_stream);
}

void DeviceNlp::residual(const std::vector<uint8_t>& mask, std::vector<double>& norm) {
  const int dim = m_kdev.dim, nnz = m_kdev.nnz_lhs, B = m_batch;
  if (static_cast<int>(mask.size()) != B) throw std::runtime_error("slpx: residual: mask length");
  if (!m_ldlt.solution_valid()) throw std::runtime_error("slpx: residual / refine: no solution in memory (factor and solve first)");
  for (int b = 0; b < B; ++b)
    if (mask[b] && std::isnan(m_ldlt.factored_regularization(b).first))
      throw std::runtime_error("slpx: residual / refine: no factorization in memory (factor and solve first)");
  const int n_part = (dim + kResidualThreads - 1) / kResidualThreads;
  residual_buffers();
  // the system p solves, in batch-major memory: assembled now (at the resident state) if the step evaluated it in
  // place; a system the caller wrote is not stale and stays as given
  materialize_kkt();
  materialize_batch_major();
  std::vector<double> reg(2 * static_cast<size_t>(B), 0.0);
  for (int b = 0; b < B; ++b)
    if (mask[b]) {
      reg[2 * b] = m_ldlt.factored_regularization(b).first;
      reg[2 * b + 1] = m_ldlt.factored_regularization(b).second;
    }
  const hipStream_t st = m_stream;
  SLPX_HIP_CHECK(hipMemcpyAsync(m_res_reg.p, reg.data(), reg.size() * sizeof(double), hipMemcpyHostToDevice, st));
  SLPX_HIP_CHECK(hipMemcpyAsync(m_res_mask.p, mask.data(), static_cast<size_t>(B), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(kkt_residual_kernel, dim3(n_part, B), dim3(kResidualThreads), 0, st, dim, m_kdev.n, nnz, m_rm_rowptr.p, m_rm_ent.p,
                     m_rm_col.p, m_lhs.p, m_rhs.p, m_ldlt.d_p(), m_res_reg.p, m_res_mask.p, m_res.p, m_res_partial.p);
  hipLaunchKernelGGL(kkt_residual_norm_kernel, dim3(B), dim3(64), 0, st, n_part, m_res_partial.p, m_res_mask.p, m_res_norm.p);
  SLPX_HIP_CHECK(hipGetLastError());
  std::vector<unsigned long long> bits(B);
  SLPX_HIP_CHECK(hipMemcpyAsync(bits.data(), m_res_norm.p, static_cast<size_t>(B) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  SLPX_HIP_CHECK(hipStreamSynchronize(st));
  norm.resize(B, std::numeric_limits<double>::quiet_NaN());
  for (int b = 0; b < B; ++b)
    if (mask[b]) std::memcpy(&norm[b], &bits[b], sizeof(double));
}

void DeviceNlp::refine_begin() {
  const size_t count = static_cast<size_t>(m_batch) * m_kdev.dim;
  if (m_ref_keep_p.n == 0) {
    m_ref_keep_p.alloc(count);
    m_ref_keep_b.alloc(count);
    m_ref_d.alloc(count);
  }
  const hipStream_t st = m_stream;
  SLPX_HIP_CHECK(hipMemcpyAsync(m_ref_keep_p.p, m_ldlt.d_p(), count * sizeof(double), hipMemcpyDeviceToDevice, st));
  SLPX_HIP_CHECK(hipMemcpyAsync(m_ref_keep_b.p, m_rhs.p, count * sizeof(double), hipMemcpyDeviceToDevice, st));
}

void DeviceNlp::refine_solve_correction() {
  const size_t bytes = static_cast<size_t>(m_batch) * m_kdev.dim * sizeof(double);
  const hipStream_t st = m_stream;
  SLPX_HIP_CHECK(hipMemcpyAsync(m_rhs.p, m_res.p, bytes, hipMemcpyDeviceToDevice, st));
  system_written_by_caller(/*lhs=*/false, /*rhs=*/true);  // (batch-major memory holds THE right-hand side now)
  solve();
  SLPX_HIP_CHECK(hipMemcpyAsync(m_ref_d.p, m_ldlt.d_p(), bytes, hipMemcpyDeviceToDevice, st));
  SLPX_HIP_CHECK(hipMemcpyAsync(m_rhs.p, m_ref_keep_b.p, bytes, hipMemcpyDeviceToDevice, st));
}

void DeviceNlp::refine_apply(const std::vector<uint8_t>& accept) {
  if (static_cast<int>(accept.size()) != m_batch) throw std::runtime_error("slpx: refine: flag length");
  const int dim = m_kdev.dim;
  const hipStream_t st = m_stream;
  SLPX_HIP_CHECK(hipMemcpyAsync(m_res_mask.p, accept.data(), static_cast<size_t>(m_batch), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(refine_accept_kernel, dim3((dim + 255) / 256, m_batch), dim3(256), 0, st, dim, m_ref_keep_p.p, m_ref_d.p, m_res_mask.p,
                     m_ldlt.d_p());
  SLPX_HIP_CHECK(hipGetLastError());
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (`accept` is the caller's)
}

void DeviceNlp::refine_keep_solution() {
  const size_t bytes = static_cast<size_t>(m_batch) * m_kdev.dim * sizeof(double);
  SLPX_HIP_CHECK(hipMemcpyAsync(m_ref_keep_p.p, m_ldlt.d_p(), bytes, hipMemcpyDeviceToDevice, m_stream));
}

}  // namespace slpx
