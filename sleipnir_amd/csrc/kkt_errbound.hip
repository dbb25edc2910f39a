// The device side of the error bounds of a solve (DeviceNlp::errbound_*; the loops are NewtonSystem::error_bounds and
// NewtonSystem::condest, newton.cpp).  Opt-in like the residual and the refinement beside it: nothing on the path of
// a Newton step or a solve comes here, and every buffer below is made on the first call.
//
// kkt_abs_row_kernel: one lane per (row, problem), grid (ceil(dim / 256), batch), the residual kernel's layout and
// masking; the arithmetic is row_abs_sum / berr_term / residual_rounding_bound of kkt_errbound.h, the bodies the CPU
// tests run.  It writes w and f = |r| + rho and leaves, per workgroup, the maxima of t_i, of the row sums, of |p_i|
// and of f_i — taken on the bit patterns (abs_bits: order-independent, and a NaN is never dropped);
// kkt_abs_fold_kernel folds a problem's slots.
//
// est_fill_kernel / est_reduce_kernel / est_fold_kernel: one round of the 1-norm estimator around DeviceNlp::solve().
// The fill writes each problem's probe vector (its own command: kind, unit index, pre-scale by f, which sign buffer
// is the kept one) into the batch-major right-hand side, zeros for a problem that has finished or is masked out; the
// reduction takes the solution v (post-scaled by f where the command says so) to four scalars per problem: ||v||_1,
// the first index of max |v_i|, "sign(v) equals the kept sign vector", "v is finite" — and stores sign(v) as the
// candidate sign vector.  ||v||_1 is summed in a fixed tree per workgroup and the workgroups' sums are added in index
// order by one lane; the index is the integer maximum of (abs_bits(v_i), ~i).  A lane reads only its own problem's
// slices, so every scalar of a problem has the same bits at any batch size, in any slot and under any mask.
// Plain vector loads and stores only; no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "device.hpp"
#include "kkt_errbound.h"

namespace slpx {

constexpr int kErrThreads = 256;

namespace {

// the fixed tree: part[0] = the reduction of part[0 .. threads) by `op`, pairs (t, t + w) for w = threads / 2, ..., 1
template <class T, class Op>
__device__ inline T block_tree(T mine, T* part, int threads, Op op) {
  const int tid = static_cast<int>(threadIdx.x);
  part[tid] = mine;
  __syncthreads();
  for (int w = threads / 2; w > 0; w >>= 1) {
    if (tid < w) part[tid] = op(part[tid], part[tid + w]);
    __syncthreads();
  }
  const T out = part[0];
  __syncthreads();  // (part is free for the next reduction)
  return out;
}

struct MaxBits {
  __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; }
};
struct SumInOrder {
  __device__ double operator()(double a, double b) const {
#pragma clang fp contract(off) reassociate(off)
    return a + b;
  }
};
// (abs_bits, ~index): the larger magnitude, of equal ones the smaller index
struct ArgMax {
  unsigned long long bits;
  unsigned int not_index;
};
struct MaxArg {
  __device__ ArgMax operator()(const ArgMax& a, const ArgMax& b) const {
    if (b.bits > a.bits || (b.bits == a.bits && b.not_index > a.not_index)) return b;
    return a;
  }
};
struct AndBits {
  __device__ unsigned int operator()(unsigned int a, unsigned int b) const { return a & b; }
};

}  // namespace

// partial[b][workgroup][4] = max t, max row sum, max |p|, max f (bit patterns); want_bounds == 0: the row sums only
__global__ __launch_bounds__(kErrThreads) void kkt_abs_row_kernel(int dim, int n_dec, int nnz, int want_bounds, const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ ent, const int32_t* __restrict__ col,
                                                                  const double* __restrict__ lhs, const double* __restrict__ rhs,
                                                                  const double* __restrict__ p, const double* __restrict__ res,
                                                                  const double* __restrict__ reg, const uint8_t* __restrict__ mask,
                                                                  double* __restrict__ w, double* __restrict__ f,
                                                                  unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long part[kErrThreads];
  const int b = static_cast<int>(blockIdx.y);
  if (mask[b] == 0) return;  // (the whole workgroup)
  const int row = static_cast<int>(blockIdx.x) * kErrThreads + static_cast<int>(threadIdx.x);
  unsigned long long t_bits = 0, sum_bits = 0, p_bits = 0, f_bits = 0;
  if (row < dim) {
    const size_t at = static_cast<size_t>(b) * dim;
    const RowAbs ra = row_abs_sum(row, rowptr, ent, col, lhs + static_cast<size_t>(b) * nnz, p + at, rhs[at + row], n_dec, reg[2 * b],
                                  reg[2 * b + 1]);
    sum_bits = abs_bits(ra.sum);
    if (want_bounds) {
      const double r = res[at + row];
      const double fi = __builtin_fabs(r) + residual_rounding_bound(r, ra.w, ra.terms, ra.exact);
      w[at + row] = ra.w;
      f[at + row] = fi;
      t_bits = abs_bits(berr_term(r, ra.w));
      p_bits = abs_bits(p[at + row]);
      f_bits = abs_bits(fi);
    }
  }
  const unsigned long long t_max = block_tree(t_bits, part, kErrThreads, MaxBits{});
  const unsigned long long sum_max = block_tree(sum_bits, part, kErrThreads, MaxBits{});
  const unsigned long long p_max = block_tree(p_bits, part, kErrThreads, MaxBits{});
  const unsigned long long f_max = block_tree(f_bits, part, kErrThreads, MaxBits{});
  if (threadIdx.x == 0) {
    unsigned long long* out = partial + (static_cast<size_t>(b) * gridDim.x + blockIdx.x) * 4;
    out[0] = t_max;
    out[1] = sum_max;
    out[2] = p_max;
    out[3] = f_max;
  }
}

__global__ __launch_bounds__(64) void kkt_abs_fold_kernel(int n_part, const unsigned long long* __restrict__ partial,
                                                          const uint8_t* __restrict__ mask, unsigned long long* __restrict__ scal) {
  __shared__ unsigned long long part[64];
  const int b = static_cast<int>(blockIdx.x);
  if (mask[b] == 0) return;
  unsigned long long m[4] = {0, 0, 0, 0};
  for (int k = static_cast<int>(threadIdx.x); k < n_part; k += 64)
    for (int c = 0; c < 4; ++c) {
      const unsigned long long v = partial[(static_cast<size_t>(b) * n_part + k) * 4 + c];
      if (v > m[c]) m[c] = v;
    }
  for (int c = 0; c < 4; ++c) {
    const unsigned long long v = block_tree(m[c], part, 64, MaxBits{});
    if (threadIdx.x == 0) scal[4 * static_cast<size_t>(b) + c] = v;
  }
}

// One command per problem and round (NormEstState::probe, kkt_errbound.h).
struct EstCommand {
  int32_t kind;   // NormEstProbe; kProbeNone: zeros in, nothing out
  int32_t j;      // of kProbeUnit
  int32_t scale;  // 1: the probe is multiplied by f before the solve; 2: the solution after it; 0: neither
  int32_t kept;   // which of the two sign buffers holds the kept sign vector (the other takes the candidate)
};

__global__ __launch_bounds__(kErrThreads) void est_fill_kernel(int dim, int batch, const EstCommand* __restrict__ cmd, const double* __restrict__ f,
                                                               const int8_t* __restrict__ sign, double* __restrict__ rhs) {
  const int b = static_cast<int>(blockIdx.y);
  const int i = static_cast<int>(blockIdx.x) * kErrThreads + static_cast<int>(threadIdx.x);
  if (i >= dim) return;
  const EstCommand c = cmd[b];
  const size_t at = static_cast<size_t>(b) * dim + i;
  double x = 0.0;
  switch (c.kind) {
    case kProbeUniform: x = 1.0 / static_cast<double>(dim); break;
    case kProbeUnit: x = i == c.j ? 1.0 : 0.0; break;
    case kProbeSigns: x = static_cast<double>(sign[(static_cast<size_t>(c.kept) * batch + b) * dim + i]); break;
    case kProbeAlternating: {
      // (dim >= 2 here: a problem of one row ends with its first round)
      const double mag = 1.0 + static_cast<double>(i) / static_cast<double>(dim - 1);
      x = (i & 1) ? -mag : mag;
      break;
    }
    default: break;
  }
  if (c.kind != kProbeNone && c.scale == 1) x = x * f[at];
  rhs[at] = x;
}

// partial[b][workgroup][4] = bits of the workgroup's sum of |v_i|, abs_bits of its largest |v_i|, ~(that entry's
// index), flags (bit 0: every sign equals the kept one, bit 1: every v_i is finite)
__global__ __launch_bounds__(kErrThreads) void est_reduce_kernel(int dim, int batch, const EstCommand* __restrict__ cmd, const double* __restrict__ f,
                                                                 const double* __restrict__ v, int8_t* __restrict__ sign,
                                                                 unsigned long long* __restrict__ partial) {
  __shared__ double part_sum[kErrThreads];
  __shared__ ArgMax part_arg[kErrThreads];
  __shared__ unsigned int part_flag[kErrThreads];
  const int b = static_cast<int>(blockIdx.y);
  const EstCommand c = cmd[b];
  if (c.kind == kProbeNone) return;  // (the whole workgroup)
  const int i = static_cast<int>(blockIdx.x) * kErrThreads + static_cast<int>(threadIdx.x);
  double mag = 0.0;
  ArgMax arg{0ull, 0u};  // (below every entry there is: ~i > 0 for every row)
  unsigned int flags = 3u;
  if (i < dim) {
    const size_t at = static_cast<size_t>(b) * dim + i;
    double vi = v[at];
    if (c.scale == 2) vi = vi * f[at];
    mag = __builtin_fabs(vi);
    arg.bits = abs_bits(vi);
    arg.not_index = ~static_cast<unsigned int>(i);
    const int8_t s = vi >= 0.0 ? 1 : -1;
    const size_t plane = static_cast<size_t>(batch) * dim;
    const bool same = sign[static_cast<size_t>(c.kept) * plane + at] == s;
    sign[static_cast<size_t>(1 - c.kept) * plane + at] = s;
    flags = (same ? 1u : 0u) | (arg.bits < 0x7ff0000000000000ull ? 2u : 0u);
  }
  const double sum = block_tree(mag, part_sum, kErrThreads, SumInOrder{});
  const ArgMax best = block_tree(arg, part_arg, kErrThreads, MaxArg{});
  const unsigned int all = block_tree(flags, part_flag, kErrThreads, AndBits{});
  if (threadIdx.x == 0) {
    unsigned long long* out = partial + (static_cast<size_t>(b) * gridDim.x + blockIdx.x) * 4;
    out[0] = __builtin_bit_cast(unsigned long long, sum);
    out[1] = best.bits;
    out[2] = best.not_index;
    out[3] = all;
  }
}

// scal[b][4] = bits of ||v||_1, the first index of max |v_i|, "signs repeated", "finite": the workgroups' slots in
// index order, by one lane (a problem has ceil(dim / 256) of them)
__global__ __launch_bounds__(64) void est_fold_kernel(int n_part, int batch, const EstCommand* __restrict__ cmd,
                                                      const unsigned long long* __restrict__ partial, unsigned long long* __restrict__ scal) {
#pragma clang fp contract(off) reassociate(off)
  const int b = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);  // one lane per problem
  if (b >= batch) return;
  if (cmd[b].kind == kProbeNone) return;
  double sum = 0.0;
  ArgMax best{0ull, 0u};
  unsigned int all = 3u;
  for (int k = 0; k < n_part; ++k) {
    const unsigned long long* in = partial + (static_cast<size_t>(b) * n_part + k) * 4;
    sum = sum + __builtin_bit_cast(double, in[0]);
    best = MaxArg{}(best, ArgMax{in[1], static_cast<unsigned int>(in[2])});
    all &= static_cast<unsigned int>(in[3]);
  }
  unsigned long long* out = scal + 4 * static_cast<size_t>(b);
  out[0] = __builtin_bit_cast(unsigned long long, sum);
  out[1] = ~best.not_index;
  out[2] = all & 1u;
  out[3] = (all >> 1) & 1u;
}

void DeviceNlp::errbound_require(const std::vector<uint8_t>& mask, const char* what) {
  if (static_cast<int>(mask.size()) != m_batch) throw std::runtime_error(std::string("slpx: ") + what + ": mask length");
  if (!m_ldlt.solution_valid()) throw std::runtime_error(std::string("slpx: ") + what + ": no solution in memory (factor and solve first)");
  for (int b = 0; b < m_batch; ++b)
    if (mask[b] && std::isnan(m_ldlt.factored_regularization(b).first))
      throw std::runtime_error(std::string("slpx: ") + what + ": no factorization in memory (factor and solve first)");
}

void DeviceNlp::errbound_rows(const std::vector<uint8_t>& mask, bool want_bounds, std::vector<ErrRowScalars>& out) {
  const int dim = m_kdev.dim, nnz = m_kdev.nnz_lhs, B = m_batch;
  errbound_require(mask, want_bounds ? "error_bounds" : "condest");
  residual_buffers();
  const int n_part = (dim + kErrThreads - 1) / kErrThreads;
  const size_t count = static_cast<size_t>(B) * dim;
  if (m_eb_partial.n == 0) {
    m_eb_partial.alloc(static_cast<size_t>(B) * n_part * 4);
    m_eb_scal.alloc(static_cast<size_t>(B) * 4);
    m_eb_scal.zero(m_stream);
  }
  if (want_bounds && m_eb_w.n == 0) {
    m_eb_w.alloc(count);
    m_eb_f.alloc(count);
    m_eb_w.zero(m_stream);
    m_eb_f.zero(m_stream);
  }
  // (the system p solves, in batch-major memory: as DeviceNlp::residual)
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
  hipLaunchKernelGGL(kkt_abs_row_kernel, dim3(n_part, B), dim3(kErrThreads), 0, st, dim, m_kdev.n, nnz, want_bounds ? 1 : 0, m_rm_rowptr.p,
                     m_rm_ent.p, m_rm_col.p, m_lhs.p, m_rhs.p, m_ldlt.d_p(), m_res.p, m_res_reg.p, m_res_mask.p, m_eb_w.p, m_eb_f.p, m_eb_partial.p);
  hipLaunchKernelGGL(kkt_abs_fold_kernel, dim3(B), dim3(64), 0, st, n_part, m_eb_partial.p, m_res_mask.p, m_eb_scal.p);
  SLPX_HIP_CHECK(hipGetLastError());
  std::vector<unsigned long long> bits(static_cast<size_t>(B) * 4);
  SLPX_HIP_CHECK(hipMemcpyAsync(bits.data(), m_eb_scal.p, bits.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  SLPX_HIP_CHECK(hipStreamSynchronize(st));
  out.assign(B, ErrRowScalars{});
  for (int b = 0; b < B; ++b)
    if (mask[b]) {
      std::memcpy(&out[b].berr, &bits[4 * b + 0], sizeof(double));
      std::memcpy(&out[b].norm1, &bits[4 * b + 1], sizeof(double));
      std::memcpy(&out[b].p_inf, &bits[4 * b + 2], sizeof(double));
      std::memcpy(&out[b].f_inf, &bits[4 * b + 3], sizeof(double));
    }
}

void DeviceNlp::errbound_round(const std::vector<EstRound>& rounds, std::vector<EstScalars>& out) {
  const int dim = m_kdev.dim, B = m_batch;
  if (static_cast<int>(rounds.size()) != B) throw std::runtime_error("slpx: error bounds: one command per problem");
  const int n_part = (dim + kErrThreads - 1) / kErrThreads;
  const size_t count = static_cast<size_t>(B) * dim;
  if (m_eb_sign.n == 0) {
    m_eb_sign.alloc(2 * count);
    m_eb_sign.zero(m_stream);
    m_eb_cmd.alloc(4 * static_cast<size_t>(B));
  }
  if (m_eb_partial.n == 0) {
    m_eb_partial.alloc(static_cast<size_t>(B) * n_part * 4);
    m_eb_scal.alloc(static_cast<size_t>(B) * 4);
    m_eb_scal.zero(m_stream);
  }
  static_assert(sizeof(EstCommand) == 4 * sizeof(int32_t));
  std::vector<EstCommand> cmd(B);
  for (int b = 0; b < B; ++b) {
    cmd[b] = EstCommand{rounds[b].kind, rounds[b].j, rounds[b].scale, rounds[b].kept};
    if (cmd[b].scale != 0 && cmd[b].kind != kProbeNone && m_eb_f.n == 0) throw std::runtime_error("slpx: error bounds: no f in memory");
    if (cmd[b].kind == kProbeUnit && (cmd[b].j < 0 || cmd[b].j >= dim)) throw std::runtime_error("slpx: error bounds: unit index out of range");
    if (cmd[b].kept != 0 && cmd[b].kept != 1) throw std::runtime_error("slpx: error bounds: sign buffer selector");
  }
  const hipStream_t st = m_stream;
  const EstCommand* d_cmd = reinterpret_cast<const EstCommand*>(m_eb_cmd.p);
  SLPX_HIP_CHECK(hipMemcpyAsync(m_eb_cmd.p, cmd.data(), cmd.size() * sizeof(EstCommand), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(est_fill_kernel, dim3(n_part, B), dim3(kErrThreads), 0, st, dim, B, d_cmd, m_eb_f.p, m_eb_sign.p, m_rhs.p);
  SLPX_HIP_CHECK(hipGetLastError());
  system_written_by_caller(/*lhs=*/false, /*rhs=*/true);  // (batch-major memory holds THE right-hand side now)
  solve();
  hipLaunchKernelGGL(est_reduce_kernel, dim3(n_part, B), dim3(kErrThreads), 0, st, dim, B, d_cmd, m_eb_f.p, m_ldlt.d_p(), m_eb_sign.p, m_eb_partial.p);
  hipLaunchKernelGGL(est_fold_kernel, dim3((B + 63) / 64), dim3(64), 0, st, n_part, B, d_cmd, m_eb_partial.p, m_eb_scal.p);
  SLPX_HIP_CHECK(hipGetLastError());
  std::vector<unsigned long long> bits(static_cast<size_t>(B) * 4);
  SLPX_HIP_CHECK(hipMemcpyAsync(bits.data(), m_eb_scal.p, bits.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (`cmd` is this frame's)
  out.assign(B, EstScalars{});
  for (int b = 0; b < B; ++b) {
    if (cmd[b].kind == kProbeNone) continue;
    std::memcpy(&out[b].norm1, &bits[4 * b + 0], sizeof(double));
    out[b].argmax = static_cast<int>(bits[4 * b + 1]);
    out[b].signs_repeated = bits[4 * b + 2] != 0;
    out[b].finite = bits[4 * b + 3] != 0;
  }
}

void DeviceNlp::errbound_restore() {
  const size_t bytes = static_cast<size_t>(m_batch) * m_kdev.dim * sizeof(double);
  const hipStream_t st = m_stream;
  SLPX_HIP_CHECK(hipMemcpyAsync(m_ldlt.d_p(), m_ref_keep_p.p, bytes, hipMemcpyDeviceToDevice, st));
  SLPX_HIP_CHECK(hipMemcpyAsync(m_rhs.p, m_ref_keep_b.p, bytes, hipMemcpyDeviceToDevice, st));
  SLPX_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace slpx
