// gfx950 (MI355X) kernels for the interior-point Newton step, and the DeviceNlp
// host object that owns their buffers.  See DESIGN.md §3 for the roofline of each.
//
//   tape_sweep     (tape_kernels.h) AD refresh: forward values + local partials, then
//                  the per-row adjoint gather, all inside LDS (one workgroup per task)
//                  replaces update_values/append_triplets/setFromTriplets
//                  (expression_graph.hpp:86-153, jacobian.hpp:134-156, hessian.hpp:132-157)
//   kkt_assemble   lhs values by gather   (interior_point.hpp:426-440)
//   kkt_rhs        rhs by column gathers  (interior_point.hpp:444-448)
//   step_backsub   pˢ, pᶻ                 (interior_point.hpp:479-480)
// The factorization and the solves between them: DeviceLdlt, device_ldlt.hip.
#include <hip/hip_runtime.h>

#include <chrono>

#include <algorithm>
#include <bit>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

#include "device.hpp"
#include "device_images.hpp"
#include "kkt_kernels.h"
#include "setup_threads.hpp"
#include "tape_jit.hpp"
#include "ipm_decide.h"
#include "ipm_launch_kernels.h"
#include "tape_kernels.h"
#include "tape_ops.h"
#include "setup_timing.hpp"

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

// Separable sums on their own (tape_reduce_body, tape_kernels.h) — used when the reductions
// cannot ride along with the interpreted tail of the tape (launch_tape).
__global__ __launch_bounds__(64) void tape_reduce_kernel(const NlpStructure::SumReduce* __restrict__ red,
                                                         const double* __restrict__ scales,
                                                         double* __restrict__ V, int v_stride) {
  __shared__ double part[64];
  V += static_cast<size_t>(blockIdx.y) * v_stride;
  tape_reduce_body(red[blockIdx.x], scales, V, part, threadIdx.x);
}

// Can two kernels of this process run at once?  Chained steps (DeviceNlp::sweep_full_for_step) need the
// sweep and the step kernel resident together; a profiler collecting hardware counters (rocprofv3 --pmc)
// or AMD_SERIALIZE_KERNEL runs one kernel at a time, and a step kernel waiting for a sweep that cannot
// start would sit out its spin bound (seen: 247 ms per step under --pmc).  So, once per system: a kernel
// on the sweep's stream waits — a few milliseconds at most — for a word a kernel on the main stream sets.
__global__ void chain_probe_wait_kernel(unsigned int* w) {
  unsigned int seen = 0;
  for (int k = 0; k < 3000 && !seen; ++k) {
    seen = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_sleep(32);
  }
  w[1] = seen ? 1u : 2u;
}
__global__ void chain_probe_set_kernel(unsigned int* w) { __hip_atomic_store(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ============================================================================
// DeviceNlp
// ============================================================================

void TapeDevice::upload(const TapeProgram& p, int batch, uint32_t n_unscaled_inputs, int chain_mode) {
  tasks.upload(p.tasks);
  // families of structurally identical tasks and the big singles get a body in the
  // generated lane-per-task kernel; everything else is interpreted
  TapeJitOptions jit_opt;
  jit_opt.n_unscaled_inputs = n_unscaled_inputs;  // x: set_scaling leaves their factor at 1
  jit_opt.chain_mode = chain_mode;
  const TapeJitResult jit = build_tape_templates(p, jit_opt);
  jit_seconds = jit.compile_seconds;
  tmpl_fn = jit.fn;
  tmpl_params = jit.params;
  {
    std::vector<uint64_t> words((tmpl_params.size() + 7) / 8, 0);
    std::memcpy(words.data(), tmpl_params.data(), tmpl_params.size());
    tmpl_params_dev.upload(words);
  }
  tmpl_mod = jit.mod;
  tmpl_threads = jit.block_threads;
  n_bodies = static_cast<uint32_t>(jit.groups.size());
  n_templated_tasks = 0;
  tmpl_blocks[0] = tmpl_blocks[1] = 0;
  if (n_bodies) {
    const TemplateTables tt = pack_template_tables(p, jit.groups, batch, tmpl_threads);
    n_templated_tasks = tt.n_templated_tasks;
    tmpl_inst.upload(tt.inst);
    for (int m = 0; m < 2; ++m) {
      tmpl_table[m].upload(tt.table[m]);
      tmpl_blocks[m] = tt.blocks[m];
    }
  }
  auto interpreted = [&](const std::vector<uint32_t>& list) {
    std::vector<uint32_t> out;
    for (uint32_t ti : list)
      if (!jit.task_is_templated[ti]) out.push_back(ti);
    return out;
  };
  std::vector<uint32_t> small_rest = interpreted(p.small_tasks), large_rest = interpreted(p.large_tasks);
  uint32_t ride_lds = p.small_lds_bytes;
  tmpl_wide_for_chain = n_bodies && tmpl_threads == 256 && large_rest.empty() && chain_mode != 0;
  if (n_bodies && tmpl_threads == 256) {
    // (tape_jit.cpp: the generated kernel's workgroups are 256 threads: every interpreted task rides in its launch)
    small_rest.insert(small_rest.end(), large_rest.begin(), large_rest.end());
    large_rest.clear();
    ride_lds = std::max(p.small_lds_bytes, p.large_lds_bytes);
  }
  small_list.upload(small_rest);
  large_list.upload(large_rest);
  global_list.upload(p.global_tasks);
  if (std::getenv("SLPX_TAPE_JIT_VERBOSE") && jit.fn)
    std::fprintf(stderr, "slpx tape kernel: %zu bodies, %s code object (%zu bytes of model numbers), %.3f s\n",
                 jit.groups.size(), jit.specialized ? "specialized" : "generic", jit.params.size(), jit.compile_seconds);
  if (std::getenv("SLPX_TAPE_JIT_VERBOSE"))
    for (uint32_t ti : p.global_tasks)
      std::fprintf(stderr, "slpx tape GLOBAL task: leaf %u node %u slot %u vout %u jout %u levels %u+%u\n", p.tasks[ti].n_leaf,
                   p.tasks[ti].n_node, p.tasks[ti].n_slot, p.tasks[ti].n_vout, p.tasks[ti].n_jout, p.tasks[ti].n_lvl, p.tasks[ti].n_slvl);
  leaf_src.upload(p.leaf_src);
  // never empty: the generated bodies read consts[0] in lanes whose leaf is not a constant
  consts.upload(p.consts.empty() ? std::vector<double>{0.0} : p.consts);
  node_rec.upload(p.node_rec);
  lvl_ptr.upload(p.lvl_ptr);
  slot_edge_ptr.upload(p.slot_edge_ptr);
  slvl_ptr.upload(p.slvl_ptr);
  edges.upload(p.edges);
  vout_src.upload(p.vout_src);
  vout_dst.upload(p.vout_dst);
  vout_scale.upload(p.vout_scale);
  jout_slot.upload(p.jout_slot);
  jout_dst.upload(p.jout_dst);
  jout_scale.upload(p.jout_scale);
  node_rec16.upload(p.node_rec16);
  slot_edge_ptr16.upload(p.slot_edge_ptr16);
  edges16.upload(p.edges16);
  n_small = static_cast<uint32_t>(small_rest.size());
  n_large = static_cast<uint32_t>(large_rest.size());
  n_global = static_cast<uint32_t>(p.global_tasks.size());
  small_lds = ride_lds;
  large_lds = p.large_lds_bytes;
  scratch_doubles = p.global_scratch_doubles;
  basic_ops = p.basic_ops;
}

TapeDev TapeDevice::view() const {
  return TapeDev{tasks.p,         leaf_src.p,   consts_stride ? consts_inst.p : consts.p,   node_rec.p,   lvl_ptr.p,
                 slot_edge_ptr.p, slvl_ptr.p,   edges.p,    vout_src.p,   vout_dst.p,
                 vout_scale.p,    jout_slot.p,  jout_dst.p, jout_scale.p, node_rec16.p,
                 slot_edge_ptr16.p, edges16.p,  consts_stride};
}

void KktPlanDevice::upload(const NlpStructure& s, const KktPlan& k) {
  dptr.upload(k.dptr);
  dsrc.upload(k.dsrc);
  pptr.upload(k.pptr);
  pa.upload(k.pa);
  pb.upload(k.pb);
  pr.upload(k.pr);
  g_src.upload(k.g_src);
  ae_colptr.upload(s.Ae.colptr);
  ae_rowidx.upload(s.Ae.rowidx);
  ai_colptr.upload(s.Ai.colptr);
  ai_rowidx.upload(s.Ai.rowidx);
  ai_rowptr.upload(k.ai_rowptr);
  ai_col.upload(k.ai_col);
  ai_src.upload(k.ai_src);
  fast_src.upload(k.fast_src);
  diag_pos.upload(lhs_diagonal_positions(k));
  n = k.n, m_e = k.m_e, m_i = k.m_i, dim = k.dim, nnz_lhs = k.lhs.nnz();
  off_f = s.off_f, off_ce = s.off_ce, off_ci = s.off_ci, off_g = s.off_g, off_Ae = s.off_Ae, off_Ai = s.off_Ai;
}

KktDev KktPlanDevice::view() const {
  KktDev K{};
  K.n = n, K.m_e = m_e, K.m_i = m_i, K.dim = dim, K.nnz_lhs = nnz_lhs;
  K.dptr = dptr.p;
  K.dsrc = dsrc.p;
  K.pptr = pptr.p;
  K.pa = pa.p;
  K.pb = pb.p;
  K.pr = pr.p;
  K.g_src = g_src.p;
  K.ae_colptr = ae_colptr.p;
  K.ae_rowidx = ae_rowidx.p;
  K.ai_colptr = ai_colptr.p;
  K.ai_rowidx = ai_rowidx.p;
  K.ai_rowptr = ai_rowptr.p;
  K.ai_col = ai_col.p;
  K.ai_src = ai_src.p;
  K.fast_src = fast_src.p;
  K.off_f = off_f, K.off_ce = off_ce, K.off_ci = off_ci, K.off_g = off_g, K.off_Ae = off_Ae, K.off_Ai = off_Ai;
  return K;
}

// The phases below run in this order; every upload() of theirs goes into the system's arena — a few allocations, one
// copy each (commit at the end) — so their order is also the order of the plan arrays in memory.
DeviceNlp::DeviceNlp(const NlpStructure& s, const KktPlan& k, const LdltPlan& l, int batch,
                     int device, const Switches& sw)
    : m_s_ref(s), m_k_ref(k), m_l_ref(l), m_batch(batch), m_device(device), m_sw(sw),
      m_ldlt(l, k, batch, DeviceLdlt::Shared{m_stream, m_mode, m_plan, m_sw, m_cus, m_h_seq, s.reduces.size()}) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    throw std::runtime_error("slpx: no HIP device available (the product path has no CPU fallback)");
  SLPX_HIP_CHECK(hipSetDevice(device));
  SetupLap lap;
  struct ArenaGuard {
    ~ArenaGuard() { DeviceArena::current() = nullptr; }
  } arena_guard;
  DeviceArena::current() = &m_arena;

  choose_initial_modes();
  upload_tapes();
  lap("  upload: tapes (+ code objects)");
  raise_lds_limits();
  m_ldlt.raise_lds_limits();
  upload_kkt_plan();
  lap("  upload: kernel attributes, KKT plan");
  m_ldlt.upload_plan();
  lap("  upload: LDLT plan");
  // (the host copies of the inline plans live until the task images are packed from them)
  const InlineKkt inline_kkt = m_mode.fuse_kkt ? build_inline_kkt(s, k, l) : InlineKkt{};
  if (m_mode.fuse_kkt) upload_inline_kkt(inline_kkt);
  lap("    images: inline KKT terms");
  const InlineBacksub inline_backsub = m_mode.fuse_backsub ? build_inline_backsub(k, l) : InlineBacksub{};
  if (m_mode.fuse_backsub) upload_inline_backsub(inline_backsub);
  lap("    images: back-substitution rows");
  note_inline_images(m_mode, inline_kkt.ok, inline_backsub.ok);
  MfImages mf_images;
  mf_images.declined = "not asked for";
  if (wants_multifrontal(m_mode, m_plan, m_sw)) mf_images = build_mf_images(l, inline_kkt, inline_backsub);
  m_ldlt.upload_mf(mf_images);
  lap("    images: multifrontal task images");
  lap("  upload: inline KKT / back-substitution / multifrontal images");
  m_ldlt.alloc_dense_buffers();  // (before the armed buffers, whose uploads follow its pattern arrays in the arena)
  alloc_value_buffers();
  m_ldlt.arm_handover_buffers();
  alloc_interleaved_buffers();
  alloc_pinned();
  DeviceArena::current() = nullptr;
  m_arena.commit();
  lap("  upload: value buffers");
  set_scaling(std::vector<double>(s.n_scales(), 1.0));
  lap("  upload: scaling, static V");
}

// What system_choice.hpp reads of the plan, and the stage of it that needs nothing measured but the device's size.
// (Before the tapes: their kernel is generated for the chain mode.)
void DeviceNlp::choose_initial_modes() {
  const LdltPlan& l = m_l_ref;
  m_plan = PlanFacts{l.dense, l.dense_pivoted, l.tasks.size(), l.factor_lds_bytes, l.mf, l.mf_n_mfma, update_slots_have_one_reader(l)};
  SLPX_HIP_CHECK(hipDeviceGetAttribute(&m_cus, hipDeviceAttributeMultiprocessorCount, m_device));
  m_mode = initial_launch_modes(m_batch, m_plan, m_s_ref.reduces.size(), m_cus, m_sw);
}

void DeviceNlp::upload_tapes() {
  const NlpStructure& s = m_s_ref;
  m_full.upload(s.full, m_batch, static_cast<uint32_t>(s.n), m_mode.chain_mode);
  m_values.upload(s.values, m_batch, static_cast<uint32_t>(s.n));
  m_reduces.upload(s.reduces);
}

// allow > 64 KB dynamic LDS
void DeviceNlp::raise_lds_limits() {
  for (const void* fn : {reinterpret_cast<const void*>(&tape_sweep_lds_kernel<256, true>),
                         reinterpret_cast<const void*>(&tape_sweep_lds_kernel<256, false>),
                         reinterpret_cast<const void*>(&tape_sweep_lds_kernel<64, true>),
                         reinterpret_cast<const void*>(&tape_sweep_lds_kernel<64, false>)})
    SLPX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
}

void DeviceNlp::upload_kkt_plan() {
  m_kplan.upload(m_s_ref, m_k_ref);
  m_kdev = m_kplan.view();
}

void DeviceNlp::upload_inline_kkt(const InlineKkt& ik) {
  m_ldlt.set_factor_lds_inline(ik.factor_lds);
  if (!ik.ok) return;
  m_ent_vsrc.upload(ik.vsrc);
  m_kkt_terms.upload(ik.terms);
  m_task_terms.upload(ik.task_terms);
}

void DeviceNlp::upload_inline_backsub(const InlineBacksub& ib) {
  m_ldlt.set_solve_lds_inline(ib.solve_lds);
  if (!ib.ok) return;
  m_bs_plan.upload(ib.plan);
  m_bs_task_plan.upload(ib.task_plan);
}

void DeviceNlp::alloc_value_buffers() {
  const NlpStructure& s = m_s_ref;
  const KktPlan& k = m_k_ref;
  const size_t B = static_cast<size_t>(m_batch);
  m_in.alloc(B * s.n_inputs());
  m_in.zero();
  m_V.alloc(B * s.nV);
  m_s.alloc(B * std::max(1, s.m_i));
  m_y.alloc(B * std::max(1, s.m_e));
  m_z.alloc(B * std::max(1, s.m_i));
  m_mu.alloc(B);
  m_lhs.alloc(B * k.lhs.nnz());
  m_rhs.alloc(B * k.dim);
  m_ps.alloc(B * std::max(1, s.m_i));
  m_pz.alloc(B * std::max(1, s.m_i));
  const uint64_t scratch = std::max(s.full.global_scratch_doubles, s.values.global_scratch_doubles);
  m_scratch.alloc(B * std::max<uint64_t>(1, scratch));
  // every value buffer starts at zero, the solver's too (DeviceLdlt::alloc_value_buffers says why)
  for (DevBuf<double>* buf : {&m_V, &m_s, &m_y, &m_z, &m_mu, &m_lhs, &m_rhs, &m_ps, &m_pz}) buf->zero();
  m_ldlt.alloc_value_buffers();
  SLPX_HIP_CHECK(hipDeviceSynchronize());  // (the memsets ran on the null stream, the kernels will not)
}

// batch-interleaved LDLT: the system where its kernels read it, [chunk of 64 problems][index][lane]
void DeviceNlp::alloc_interleaved_buffers() {
  if (!m_mode.il) return;
  const size_t C = (static_cast<size_t>(m_batch) + 63) / 64, W = 64;
  m_lhs_il.alloc(C * m_k_ref.lhs.nnz() * W);
  m_rhs_il.alloc(C * m_l_ref.n * W);
  m_ldlt.alloc_interleaved_buffers();
}

// the sequence word the publishing kernels bump and the host spins on (after the solver's pinned words)
void DeviceNlp::alloc_pinned() {
  m_ldlt.alloc_pinned();
  unsigned long long* seq = nullptr;
  SLPX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&seq), sizeof(unsigned long long)));
  *seq = 0;
  m_h_seq = seq;
  m_seq_dev.alloc(1);
  m_seq_dev.zero();
}

DeviceNlp::~DeviceNlp() {
  if (m_h_seq) (void)hipHostFree(const_cast<unsigned long long*>(m_h_seq));
  if (m_ipm_host) (void)hipHostFree(m_ipm_host);
  if (m_ipm_ctl_host) (void)hipHostFree(m_ipm_ctl_host);
  if (m_ipm_ctl_dev) (void)hipFree(m_ipm_ctl_dev);
  if (m_tape_stream) {
    (void)hipStreamSynchronize(m_tape_stream);
    (void)hipStreamDestroy(m_tape_stream);
  }
  if (m_chain_ev) (void)hipEventDestroy(m_chain_ev);
  if (m_stream.ev) (void)hipEventDestroy(m_stream.ev);
}

void DeviceNlp::set_scaling(const std::vector<double>& scales) {
  const NlpStructure& s = m_s_ref;
  if (static_cast<int>(scales.size()) != s.n_scales())
    throw std::runtime_error("set_scaling: wrong length");
  m_scales.upload(scales);
  std::vector<double> in_scale(s.n_inputs(), 1.0);
  for (int j = 0; j < s.m_e; ++j) in_scale[s.n + j] = scales[1 + j];
  for (int j = 0; j < s.m_i; ++j) in_scale[s.n + s.m_e + j] = scales[1 + s.m_e + j];
  m_in_scale.upload(in_scale);
  m_V_static.assign(s.nV, 0.0);
  for (int k = 0; k < s.nV; ++k) {
    const int32_t sc = s.V_scale_idx[k];
    m_V_static[k] = sc >= 0 ? scales[sc] * s.V_static_raw[k] : s.V_static_raw[k];
  }
  std::vector<double> all(static_cast<size_t>(m_batch) * s.nV);
  for (int b = 0; b < m_batch; ++b)
    std::copy(m_V_static.begin(), m_V_static.end(), all.begin() + static_cast<size_t>(b) * s.nV);
  SLPX_HIP_CHECK(hipMemcpy(m_V.p, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice));
  if (m_ipm)
    SLPX_HIP_CHECK(hipMemcpy(m_V_trial.p, m_V_static.data(), m_V_static.size() * sizeof(double), hipMemcpyHostToDevice));
}

void DeviceNlp::upload_x(const double* x) {
  const NlpStructure& s = m_s_ref;
  SLPX_HIP_CHECK(hipMemcpy2DAsync(m_in.p, s.n_inputs() * sizeof(double), x, s.n * sizeof(double),
                                  s.n * sizeof(double), m_batch, hipMemcpyHostToDevice, m_stream));
}

void DeviceNlp::upload_duals(const double* sv, const double* y, const double* z) {
  const NlpStructure& s = m_s_ref;
  const size_t B = m_batch;
  if (s.m_i) {
    SLPX_HIP_CHECK(hipMemcpyAsync(m_s.p, sv, B * s.m_i * sizeof(double), hipMemcpyHostToDevice, m_stream));
    SLPX_HIP_CHECK(hipMemcpyAsync(m_z.p, z, B * s.m_i * sizeof(double), hipMemcpyHostToDevice, m_stream));
    SLPX_HIP_CHECK(hipMemcpy2DAsync(m_in.p + s.n + s.m_e, s.n_inputs() * sizeof(double), z,
                                    s.m_i * sizeof(double), s.m_i * sizeof(double), m_batch,
                                    hipMemcpyHostToDevice, m_stream));
  }
  if (s.m_e) {
    SLPX_HIP_CHECK(hipMemcpyAsync(m_y.p, y, B * s.m_e * sizeof(double), hipMemcpyHostToDevice, m_stream));
    SLPX_HIP_CHECK(hipMemcpy2DAsync(m_in.p + s.n, s.n_inputs() * sizeof(double), y,
                                    s.m_e * sizeof(double), s.m_e * sizeof(double), m_batch,
                                    hipMemcpyHostToDevice, m_stream));
  }
}

void DeviceNlp::upload_mu(const double* mu) {
  SLPX_HIP_CHECK(hipMemcpyAsync(m_mu.p, mu, m_batch * sizeof(double), hipMemcpyHostToDevice, m_stream));
}

void DeviceNlp::download_V(double* V) { download(m_V.p, V, static_cast<size_t>(m_batch) * m_s_ref.nV); }

void DeviceNlp::download(const double* dev, double* host, size_t count) {
  SLPX_HIP_CHECK(hipMemcpyAsync(host, dev, count * sizeof(double), hipMemcpyDeviceToHost, m_stream));
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
}

void DeviceNlp::launch_tape(const TapeDevice& t, bool reverse) {
  launch_tape(t, reverse, m_stream, m_stream);
}

// The task classes are independent; `other`: the stream of the few large / global tasks.
void DeviceNlp::launch_tape(const TapeDevice& t, bool reverse, hipStream_t small_stream,
                            hipStream_t other) {
  const TapeDev view = t.view();
  const int in_stride = m_s_ref.n_inputs(), v_stride = m_s_ref.nV;
  const unsigned long long sstride = m_scratch.n / m_batch;
  const double* in_p = m_in_override ? m_in_override : m_in.p;
  double* V_p = m_V_override ? m_V_override : m_V.p;
  // basic_ops: the program only uses + - * / sin cos sqrt and the piecewise ops, so
  // the kernel specialization without pow/exp/log/erf/... (fewer VGPRs, less code)
  // generated template kernels: one lane per task instance (tape_jit.hpp)
  // interpreted 64-thread tasks ride along in the generated kernel's launch when there is one
  const bool small_rides = t.n_bodies > 0 && t.n_small > 0;
  if (t.n_bodies) {
    const int mode = reverse ? 1 : 0;
    const unsigned* table = t.tmpl_table[mode].p;
    int n_bodies = static_cast<int>(t.n_bodies);
    const unsigned* inst = t.tmpl_inst.p;
    const unsigned* leaf_src = view.leaf_src;
    const double* consts = view.consts;
    const double* in = in_p;
    int in_stride_arg = in_stride;
    const double* in_scale = m_in_scale.p;
    const double* scales = m_scales.p;
    double* V = V_p;
    int v_stride_arg = v_stride;
    const unsigned* vout_dst = view.vout_dst;
    const int* vout_scale = view.vout_scale;
    const unsigned* jout_dst = view.jout_dst;
    const int* jout_scale = view.jout_scale;
    TapeDev view_arg = view;
    const unsigned* task_list = t.small_list.p;
    int n_template_blocks = static_cast<int>(t.tmpl_blocks[mode]);
    int do_reverse = reverse ? 1 : 0;
    const uint64_t* params_dev = t.tmpl_params_dev.p;
    unsigned int* chain = m_chain_args.chain;
    unsigned int wait_step = m_chain_args.wait_step, this_step = m_chain_args.this_step;
    const unsigned grid = t.tmpl_blocks[mode] + (small_rides ? t.n_small : 0u);
    unsigned int n_workgroups = m_chain_args.skip_flag ? 0u : grid * static_cast<unsigned>(m_batch);
    m_last_tape_workgroups = grid * static_cast<unsigned>(m_batch);
    void* args[] = {&table,  &n_bodies, &inst,         &leaf_src, &consts,     &in,       &in_stride_arg,
                    &in_scale, &scales, &V,            &v_stride_arg, &vout_dst, &vout_scale, &jout_dst,
                    &jout_scale, &view_arg, &task_list, &n_template_blocks, &do_reverse,
                    &params_dev, &chain, &wait_step, &this_step, &n_workgroups};
    SLPX_HIP_CHECK(hipModuleLaunchKernel(t.tmpl_fn, grid, m_batch, 1, t.tmpl_threads, 1, 1, small_rides ? t.small_lds : 0u,
                                         small_stream, args, nullptr));
  }
  auto small_fn = t.basic_ops ? tape_sweep_lds_kernel<64, false> : tape_sweep_lds_kernel<64, true>;
  auto large_fn = t.basic_ops ? tape_sweep_lds_kernel<256, false> : tape_sweep_lds_kernel<256, true>;
  if (t.n_small && !small_rides)
    hipLaunchKernelGGL(small_fn, dim3(t.n_small, m_batch), dim3(64), t.small_lds, small_stream, view,
                       t.small_list.p, in_p, in_stride, m_in_scale.p, m_scales.p, V_p, v_stride,
                       reverse ? 1 : 0);
  if (t.n_large)
    hipLaunchKernelGGL(large_fn, dim3(t.n_large, m_batch), dim3(256), t.large_lds, other, view,
                       t.large_list.p, in_p, in_stride, m_in_scale.p, m_scales.p, V_p, v_stride,
                       reverse ? 1 : 0);
  if (t.n_global)
    hipLaunchKernelGGL(tape_sweep_global_kernel, dim3(t.n_global, m_batch), dim3(1024), 0, other,
                       view, t.global_list.p, in_p, in_stride, m_in_scale.p, m_scales.p, V_p,
                       v_stride, m_scratch.p, sstride, reverse ? 1 : 0);
  if (m_reduces.n && m_tape_reduce)
    hipLaunchKernelGGL(tape_reduce_kernel, dim3(static_cast<uint32_t>(m_reduces.n), m_batch), dim3(64), 0,
                       small_stream, m_reduces.p, m_scales.p, V_p, v_stride);
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::sweep_full(bool with_reduce) {
  m_tape_reduce = with_reduce;
  launch_tape(m_full, true);
  m_tape_reduce = true;
}
void DeviceNlp::sweep_full_for_step() {
  const TapeDevice& t = m_full;
  // one generated kernel is the whole sweep (nothing interpreted beside it), the step is the one-launch
  // multifrontal kernel
  // (and its workgroups are single waves: g-fold's sweep, 256-thread workgroups interpreting its packs of
  // rows, shares the chip badly with the step kernel — 13.3 k steps/s chained against 13.6 k)
  const bool one_kernel = t.n_bodies > 0 && t.n_large == 0 && t.n_global == 0 && (t.tmpl_threads == 64 || t.tmpl_wide_for_chain);
  if (!m_mode.chain_on || !one_kernel || m_batch != 1 || !m_ldlt.step_possible() || !m_mode.fuse_solve) {
    sweep_full(/*with_reduce=*/false);
    return;
  }
  if (m_tape_stream == nullptr) {
    SLPX_HIP_CHECK(hipStreamCreateWithFlags(&m_tape_stream, hipStreamNonBlocking));
    SLPX_HIP_CHECK(hipEventCreateWithFlags(&m_chain_ev, hipEventDisableTiming));
    SLPX_HIP_CHECK(hipEventCreateWithFlags(&m_stream.ev, hipEventDisableTiming));
    m_stream.tape = m_tape_stream;
    {
      // (tests: the running totals start so far below their bound, so that a few thousand chained steps cross it —
      // SLPX_DEBUG_CHAIN_TOTALS_HEADROOM workgroups of headroom — and the restart of the counts is exercised)
      std::vector<unsigned int> words(128, 0u);
      if (const char* env = std::getenv("SLPX_DEBUG_CHAIN_TOTALS_HEADROOM")) {
        const unsigned int headroom = static_cast<unsigned int>(std::max(1L, std::atol(env)));
        m_chain_sweep_wgs = m_chain_step_wgs = (1u << 29) - std::min(headroom, 1u << 28);
        words[16] = m_chain_sweep_wgs;
        words[48] = m_chain_step_wgs;
      }
      m_chain.upload(words);
    }
    // (words 96, 97: the concurrency probe, see chain_probe_wait_kernel)
    hipLaunchKernelGGL(chain_probe_wait_kernel, dim3(1), dim3(1), 0, m_tape_stream, m_chain.p + 96);
    hipLaunchKernelGGL(chain_probe_set_kernel, dim3(1), dim3(1), 0, m_stream.raw(), m_chain.p + 96);
    SLPX_HIP_CHECK(hipStreamSynchronize(m_tape_stream));
    SLPX_HIP_CHECK(hipStreamSynchronize(m_stream.raw()));
    unsigned int verdict = 0;
    SLPX_HIP_CHECK(hipMemcpy(&verdict, m_chain.p + 97, sizeof(verdict), hipMemcpyDeviceToHost));
    if (verdict != 1u) {
      unchain(m_mode);  // kernels run one at a time here: the sweep stays in the main stream
      if (std::getenv("SLPX_LDLT_VERBOSE")) std::fprintf(stderr, "slpx: kernels of two streams do not run at once here: steps are not chained\n");
      sweep_full(/*with_reduce=*/false);
      return;
    }
  }
  m_tape_reduce = false;
  if (m_stream.tape_pending) {
    // The last chained sweep was never consumed (its step threw before the step kernel was launched, or
    // the caller swept twice): no step kernel will signal the word a chained sweep would wait for.  Order
    // the streams by an event and start over.
    (void)static_cast<hipStream_t>(m_stream);  // waits for that sweep, marks the stream touched
    m_last_step_chained = false;
  }
  if (m_chain_seq >= (1u << 30) - 1u || m_chain_sweep_wgs >= (1u << 29) || m_chain_step_wgs >= (1u << 29)) {
    // step numbers stay in [1, 2^30) (the kernels compare them as signed differences, use 0 for "no wait"
    // and bit 31 for failure): every ~14 hours of chained steps, one unchained step and a fresh count
    SLPX_HIP_CHECK(hipStreamSynchronize(m_tape_stream));
    SLPX_HIP_CHECK(hipStreamSynchronize(m_stream.raw()));
    SLPX_HIP_CHECK(hipMemset(m_chain.p, 0, 64 * sizeof(unsigned int)));
    m_chain_seq = 0;
    m_chain_sweep_wgs = m_chain_step_wgs = 0;
    m_last_step_chained = false;
    m_stream.touched = true;
  }
  if (m_stream.touched) {
    // Something else went to the main stream since the last step (an upload of the state, a download of
    // the result, another kernel): this step's sweep goes there too, behind all of it — the pattern of a
    // caller that looks at every step costs nothing extra.  Only steps that FOLLOW a step directly chain.
    m_stream.touched = false;
    launch_tape(m_full, true, m_stream.raw(), m_stream.raw());
    m_tape_reduce = true;
    return;
  }
  // the step kernel before this sweep: a chained one tells the sweep itself when its last workgroup is
  // through; any other (the first step of a run, a re-attempt of the policy loop) through an event, once
  unsigned int wait_step = m_chain_step_wgs;  // (every workgroup of the chained step kernels so far)
  if (!m_last_step_chained) {
    SLPX_HIP_CHECK(hipEventRecord(m_chain_ev, m_stream.raw()));
    SLPX_HIP_CHECK(hipStreamWaitEvent(m_tape_stream, m_chain_ev, 0));
    wait_step = 0;
  }
  if (m_debug_break_chain && wait_step != 0u) {
    m_debug_break_chain = false;
    wait_step += 1u << 20;  // (slpx_debug_chain) step kernels nobody launched
  }
  ++m_chain_seq;
  m_chain_args = ChainArgs{m_chain.p, wait_step, m_chain_seq};
  launch_tape(m_full, true, m_tape_stream, m_tape_stream);
  m_chain_sweep_wgs += m_last_tape_workgroups;
  m_tape_reduce = true;
  m_chain_args = ChainArgs{};
  m_stream.tape_pending = true;  // until the step kernel that waits for this sweep is launched
}
// A chained step reported kLdltChainFailure: one of the two kernels gave up waiting for the other (never
// expected — a shared / preempted / serialized GPU).  Drain both streams, clear the words, keep this
// system's steps unchained from now on and leave V as a fresh sweep of the current state writes it.
void DeviceNlp::recover_from_chain_failure() {
  if (m_tape_stream != nullptr) SLPX_HIP_CHECK(hipStreamSynchronize(m_tape_stream));
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream.raw()));
  if (m_chain.p != nullptr) SLPX_HIP_CHECK(hipMemset(m_chain.p, 0, 64 * sizeof(unsigned int)));
  unchain(m_mode);
  m_chain_sweep_wgs = m_chain_step_wgs = 0;
  m_last_step_chained = false;
  m_stream.tape_pending = false;
  m_stream.touched = true;
  ++m_chain_failures;
  if (std::getenv("SLPX_LDLT_VERBOSE")) std::fprintf(stderr, "slpx: a chained step lost its hand-over: the step is redone, steps are unchained from here on\n");
  sweep_full(/*with_reduce=*/false);
}
void DeviceNlp::sweep_values() { launch_tape(m_values, false); }
void DeviceNlp::sweep_values_trial() {
  m_in_override = m_trial_in.p;
  m_V_override = m_V_trial.p;
  m_tape_reduce = false;  // ipm_trial_metrics_kernel, the only reader of these values, finishes the sums
  launch_tape(m_values, false);
  m_tape_reduce = true;
  m_in_override = nullptr;
  m_V_override = nullptr;
}

static inline int grid_for(int work, int block, int cap = 2048) {
  return std::max(1, std::min((work + block - 1) / block, cap));
}

// lhs / rhs of the CURRENT state into memory, if the last step did without them
void DeviceNlp::materialize_kkt() {
  if (m_kkt_pending) {  // the factorization that was to evaluate the system never came
    const bool with_reduce = m_kkt_pending == 2;
    m_kkt_pending = 0;
    build_kkt(with_reduce);
    return;
  }
  if (m_lhs_stale) assemble();
  if (m_rhs_stale) build_rhs();
}

// batch-major lhs / rhs for whoever asks (slpx_system_get, a caller that writes its own system):
// out of the interleaved arrays the assembly kernels filled; what the caller does with the pointer
// is not known, so the next factorization transposes again
void DeviceNlp::materialize_batch_major() {
  if (!m_mode.il) return;
  if (m_lhs_in_il) {
    m_ldlt.to_batch_major(m_lhs_il.p, m_kdev.nnz_lhs, m_lhs.p);
    m_lhs_in_il = false;
  }
  if (m_rhs_in_il) {
    m_ldlt.to_batch_major(m_rhs_il.p, m_kdev.dim, m_rhs.p);
    m_rhs_in_il = false;
  }
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::assemble() {
  m_lhs_stale = false;
  m_lhs_in_il = false;
  if (m_mode.il) {
    hipLaunchKernelGGL(kkt_assemble_il_kernel, dim3(grid_for(m_kdev.nnz_lhs, 64), il_groups(m_batch)), dim3(256), 0, m_stream,
                       m_kdev, m_V.p, m_s_ref.nV, m_s.p, m_z.p, m_lhs_il.p, m_batch);
    m_lhs_in_il = true;
  } else if (m_batch >= kBatchPerThread) {
    // measured at 512 x N=1000: 1 problem per thread 0.084 ms, 2: 0.083, 4: 0.079, 8: 0.090
    hipLaunchKernelGGL(kkt_assemble_batch_kernel<kBatchPerThread>,
                       dim3(grid_for(m_kdev.nnz_lhs, 256), (m_batch + kBatchPerThread - 1) / kBatchPerThread),
                       dim3(256), 0, m_stream, m_kdev, m_V.p, m_s_ref.nV, m_s.p, m_z.p, m_lhs.p, m_batch);
  } else {
    // four entries per thread (see the kernel)
    hipLaunchKernelGGL(kkt_assemble_kernel, dim3(grid_for((m_kdev.nnz_lhs + 3) / 4, 256), m_batch),
                       dim3(256), 0, m_stream, m_kdev, m_V.p, m_s_ref.nV, m_s.p, m_z.p, m_lhs.p);
  }
  SLPX_HIP_CHECK(hipGetLastError());
}

// lhs + rhs (+ the separable-sum reductions a sweep_full(false) left out) in one launch
void DeviceNlp::build_kkt(bool with_reduce) {
  if (m_batch >= kBatchPerThread) {  // throughput regime: the batch kernels, separately
    if (m_mode.il) {
      // (interleaved lhs and rhs: one launch, kkt_build_il_kernel)
      const int na = grid_for(m_kdev.nnz_lhs, 64), nr = (m_kdev.dim + 63) / 64;
      hipLaunchKernelGGL(kkt_build_il_kernel, dim3(na + nr, il_groups(m_batch)), dim3(256), 0, m_stream, m_kdev, m_V.p,
                         m_s_ref.nV, m_s.p, m_y.p, m_z.p, m_mu.p, m_lhs_il.p, m_rhs_il.p, m_batch, na);
      m_lhs_stale = m_rhs_stale = false;
      m_lhs_in_il = m_rhs_in_il = true;
    } else {
      assemble();
      build_rhs();
    }
    if (with_reduce && m_reduces.n)
      hipLaunchKernelGGL(tape_reduce_kernel, dim3(static_cast<uint32_t>(m_reduces.n), m_batch), dim3(64), 0,
                         m_stream, m_reduces.p, m_scales.p, m_V.p, m_s_ref.nV);
    SLPX_HIP_CHECK(hipGetLastError());
    return;
  }
  if (m_defer_kkt) {  // evaluated inside the factorization's launch (take_kkt_fuse)
    m_kkt_pending = with_reduce ? 2 : 1;
    m_lhs_stale = m_rhs_stale = true;
    return;
  }
  m_lhs_stale = m_rhs_stale = false;
  m_lhs_in_il = m_rhs_in_il = false;
  const int na = grid_for((m_kdev.nnz_lhs + 3) / 4, 256), nr = grid_for(m_kdev.dim, 256);
  const int nred = with_reduce ? static_cast<int>(m_reduces.n) : 0;
  hipLaunchKernelGGL(kkt_build_kernel, dim3(na + nr + nred, m_batch), dim3(256), 0, m_stream, m_kdev, m_V.p,
                     m_s_ref.nV, m_s.p, m_y.p, m_z.p, m_mu.p, m_lhs.p, m_rhs.p, na, nr, m_reduces.p, m_scales.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

// build_kkt() when a factorization attempt is the next thing enqueued (a Newton step): the
// assembly then rides in that launch (device.hpp: KktFuse)
void DeviceNlp::build_kkt_for_step(bool with_reduce) {
  m_defer_kkt = m_mode.fuse_kkt;
  build_kkt(with_reduce);
  m_defer_kkt = false;
}

void DeviceNlp::assemble_lsq() {
  m_lhs_stale = false;
  m_lhs_in_il = false;
  hipLaunchKernelGGL(kkt_assemble_lsq_kernel, dim3(grid_for(m_kdev.nnz_lhs, 256), m_batch), dim3(256),
                     0, m_stream, m_kdev, m_V.p, m_s_ref.nV, m_s.p, m_lhs.p);
  hipLaunchKernelGGL(kkt_add_identity_kernel, dim3(grid_for(m_kdev.n, 256), m_batch), dim3(256), 0,
                     m_stream, m_kdev, m_kplan.diag_pos.p, m_lhs.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

int DeviceNlp::debug_tmpl_clocks(unsigned long long* out, int blocks) {
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  hipDeviceptr_t p = nullptr;
  size_t bytes = 0;
  if (!m_full.tmpl_mod || hipModuleGetGlobal(&p, &bytes, m_full.tmpl_mod, "slpx_tmpl_clocks") != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  const size_t want = std::min<size_t>(bytes, static_cast<size_t>(blocks) * 8 * sizeof(unsigned long long));
  SLPX_HIP_CHECK(hipMemcpy(out, p, want, hipMemcpyDeviceToHost));
  return static_cast<int>(m_full.tmpl_blocks[1]);
}

void DeviceNlp::debug_tape_clocks(unsigned long long* out16) {
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  SLPX_HIP_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_tape_clocks), 16 * sizeof(unsigned long long)));
}

void DeviceNlp::refresh_params(const Graph& g) {
  std::vector<double> values;
  for (NodeId node : m_s_ref.parameter_nodes()) values.push_back(g.val[node]);
  set_parameters(values.data(), /*per_instance=*/false);
}

void DeviceNlp::set_parameters(const double* values, bool per_instance) {
  const std::vector<NodeId> nodes = m_s_ref.parameter_nodes();
  if (nodes.empty()) {
    if (per_instance) throw std::runtime_error("slpx: set_parameters: the model has no parameters");
    return;
  }
  if (values == nullptr) throw std::runtime_error("slpx: set_parameters: values is null");
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));  // (no sweep in flight reads the pool that is rewritten)
  const size_t n_p = nodes.size(), B = static_cast<size_t>(m_batch);
  auto install = [&](const TapeProgram& prog, TapeDevice& dev) {
    if (prog.params.empty()) return;
    const size_t nc = prog.consts.size();
    // where parameter j of the caller's vector sits in this program's pool (slot j: both programs claim
    // `param_order` first — looked up all the same, so that a program that reaches fewer parameters is served too)
    std::vector<std::pair<size_t, uint32_t>> slot_of;  // (j, slot)
    for (const auto& [node, slot] : prog.params) {
      const size_t j = static_cast<size_t>(std::lower_bound(nodes.begin(), nodes.end(), node) - nodes.begin());
      if (slot >= nc) throw std::runtime_error("slpx: set_parameters: a parameter slot outside the constant pool");
      slot_of.emplace_back(j, slot);
    }
    if (!per_instance) {
      std::vector<double> c = prog.consts;
      for (const auto& [j, slot] : slot_of) c[slot] = values[j];
      SLPX_HIP_CHECK(hipMemcpy(dev.consts.p, c.data(), nc * sizeof(double), hipMemcpyHostToDevice));
      dev.consts_stride = 0;
      return;
    }
    std::vector<double> c(B * nc);
    for (size_t b = 0; b < B; ++b) {
      std::copy(prog.consts.begin(), prog.consts.end(), c.begin() + b * nc);
      for (const auto& [j, slot] : slot_of) c[b * nc + slot] = values[b * n_p + j];
    }
    if (dev.consts_inst.n != c.size()) dev.consts_inst.alloc(c.size());
    SLPX_HIP_CHECK(hipMemcpy(dev.consts_inst.p, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice));
    dev.consts_stride = static_cast<uint32_t>(nc);
  };
  install(m_s_ref.full, m_full);
  install(m_s_ref.values, m_values);
  // (a program without parameters keeps its shared pool, stride 0, in either mode)
}

void DeviceNlp::build_rhs() {
  m_rhs_stale = false;
  m_rhs_in_il = false;
  if (m_mode.il) {
    hipLaunchKernelGGL(kkt_rhs_il_kernel, dim3((m_kdev.dim + 63) / 64, il_groups(m_batch)), dim3(256), 0, m_stream, m_kdev,
                       m_V.p, m_s_ref.nV, m_s.p, m_y.p, m_z.p, m_mu.p, m_rhs_il.p, m_batch);
    m_rhs_in_il = true;
    SLPX_HIP_CHECK(hipGetLastError());
    return;
  }
  // (a batch variant like kkt_assemble_batch_kernel was measured SLOWER here: 0.102 ms vs
  // 0.070 ms at 512 x N=1000 — the per-column loops are short and the extra registers cost
  // occupancy)
  hipLaunchKernelGGL(kkt_rhs_kernel, dim3(grid_for(m_kdev.dim, 256), m_batch), dim3(256), 0, m_stream,
                     m_kdev, m_V.p, m_s_ref.nV, m_s.p, m_y.p, m_z.p, m_mu.p, m_rhs.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

// the system evaluated inside the factorization's launch, if a build_kkt_for_step() asked for it
KktFuse DeviceNlp::kkt_fuse_for(int kkt_mode) const {
  KktFuse f;
  if (kkt_mode) {
    f.inline_kkt = 1;
    f.n_blocks = kkt_mode == 2 ? static_cast<int>(m_reduces.n) : 0;
    f.V = m_V.p;
    f.s = m_s.p;
    f.y = m_y.p;
    f.z = m_z.p;
    f.mu = m_mu.p;
    f.ent_vsrc = m_ent_vsrc.p;
    f.terms = reinterpret_cast<const uint4*>(m_kkt_terms.p);
    f.task_terms = m_task_terms.p;
    f.Vw = m_V.p;
    if (m_mode.fuse_kkt_store) {
      f.store_lhs = m_lhs.p;
      f.store_rhs = m_rhs.p;
    }
    f.red = m_reduces.p;
    f.scales = m_scales.p;
  }
  return f;
}
KktFuse DeviceNlp::take_kkt_fuse() {
  const KktFuse f = kkt_fuse_for(m_kkt_pending);
  if (m_kkt_pending) {
    if (m_mode.fuse_kkt_store) m_lhs_stale = m_rhs_stale = false;
    m_kkt_pending = 0;
  }
  return f;
}

BacksubFuse DeviceNlp::backsub_fuse() {
  BacksubFuse f;
  f.on = 1;
  f.V = m_V.p;
  f.s = m_s.p;
  f.z = m_z.p;
  f.mu = m_mu.p;
  f.ps = m_ps.p;
  f.pz = m_pz.p;
  f.off_ci = m_kdev.off_ci;
  f.plan = reinterpret_cast<const uint4*>(m_bs_plan.p);
  f.task_plan = m_bs_task_plan.p;
  f.seq_dev = m_seq_dev.p;
  f.seq_host = m_h_seq;
  return f;
}

void DeviceNlp::factor(const std::vector<double>& delta, const std::vector<double>& gamma,
                       const std::vector<uint8_t>& active) {
  if (!m_kkt_pending) materialize_kkt();  // e.g. a second attempt after one that evaluated the system in place
  m_ldlt.factor(delta, gamma, active, system(), m_ldlt.factor_evaluates_inline() ? take_kkt_fuse() : KktFuse{});
}

// What rides in a launch of the step kernel made now: the system or its evaluation in place, the back-substitution,
// the chain link of a chained step (sweep_full_for_step) and the gate of a step enqueued ahead.
LdltStepRiders DeviceNlp::step_riders(const KktFuse& f, bool chained) {
  LdltStepRiders r;
  r.kkt = f;
  r.backsub = backsub_fuse();
  r.lhs = m_lhs.p;
  r.rhs = m_rhs.p;
  if (chained) {
    r.chain = m_chain.p;
    r.wait_step = m_chain_sweep_wgs;  // (every workgroup of the chained sweeps so far, this step's included)
  }
  r.this_step = m_chain_seq;
  if (m_gate_next_step) {  // (one launch: the step enqueued before the iteration in front of it was decided)
    r.gate = m_ipm_gate.p;
    m_gate_next_step = false;
  }
  return r;
}

void DeviceNlp::factor_solve_publish(const std::vector<double>& delta, const std::vector<double>& gamma,
                                     const std::vector<uint8_t>& active) {
  if (!m_mode.fuse_solve || !m_ldlt.step_possible()) {
    factor(delta, gamma, active);
    solve_backsub_publish();
    return;
  }
  if (!m_kkt_pending) materialize_kkt();
  const KktFuse f = take_kkt_fuse();
  // a chained step: the kernel variant that waits for its sweep itself and whose last workgroup tells the next step's
  // sweep; the main stream stays "untouched" by a step's own launches
  const bool chained = m_stream.tape_pending;
  const unsigned int workgroups = m_ldlt.step(delta, gamma, active, step_riders(f, chained));
  if (chained) m_chain_step_wgs += workgroups;  // (what the next chained sweep waits for in chain[48])
  m_stream.tape_pending = false;
  m_last_step_chained = chained;
  m_ldlt.stats_handed_to_host(++m_seq_expected);
}

// ---- twin attempt (DeviceLdlt::step_twin) ----
bool DeviceNlp::twin_ready() {
  if (!m_ldlt.twin_available()) return false;
  if (m_ps_tw.n == 0) {
    for (auto [tw, first] : {std::pair{&m_ps_tw, &m_ps}, {&m_pz_tw, &m_pz}}) {
      tw->alloc(std::max<size_t>(1, first->n));
      tw->zero();
    }
    SLPX_HIP_CHECK(hipDeviceSynchronize());  // (the memsets ran on the null stream)
  }
  return true;
}

void DeviceNlp::launch_twin(double delta0, double gamma0, double delta1, double gamma1, int mode, const KktFuse& f, const double* lhs2,
                            const double* rhs2) {
  LdltStepRiders r = step_riders(f, false);
  r.ps2 = m_ps_tw.p;
  r.pz2 = m_pz_tw.p;
  r.lhs2 = lhs2;
  r.rhs2 = rhs2;
  MfRide ride;
  if (m_ride_next) {
    ride = ipm_take_ride();
    r.ride = &ride;
    r.gate = nullptr;  // (nothing in front of this launch is undecided: its own riding workgroups decide)
  }
  m_ldlt.step_twin(delta0, gamma0, delta1, gamma1, mode, r);
  m_stream.tape_pending = false;
  m_last_step_chained = false;
  m_ldlt.stats_handed_to_host(++m_seq_expected);
}

bool DeviceNlp::factor_solve_publish_twin(double delta0, double gamma0, double delta1, double gamma1, int mode) {
  if (!twin_ready() || m_stream.tape_pending) return false;
  if (!m_kkt_pending) materialize_kkt();
  launch_twin(delta0, gamma0, delta1, gamma1, mode, take_kkt_fuse(), nullptr, nullptr);
  return true;
}

bool DeviceNlp::factor_solve_publish_twin_written(double delta0, double gamma0, double delta1, double gamma1, int mode, const double* lhs2,
                                                  const double* rhs2) {
  if (!twin_ready() || m_stream.tape_pending || m_kkt_pending || m_lhs_stale || m_rhs_stale) return false;
  launch_twin(delta0, gamma0, delta1, gamma1, mode, KktFuse{}, lhs2, rhs2);
  return true;
}

void DeviceNlp::adopt_twin() {
  m_ldlt.adopt_twin();
  m_ps.swap(m_ps_tw);
  m_pz.swap(m_pz_tw);
}

// Full solve for a right-hand side that arrived AFTER the factorization (second-order
// corrections, multiplier estimate, slpx_ldlt_solve)
void DeviceNlp::solve() {
  if (m_rhs_stale) build_rhs();
  m_ldlt.solve(system());
}

void DeviceNlp::solve_after_factor() {
  if (m_mode.dense && m_rhs_stale) build_rhs();  // (nothing rides in a dense factorization: it solves from the rhs in memory)
  m_ldlt.solve_after_factor(system());
}

// backward solve, back-substitution and the hand-over of the current attempt's counters to the
// host: one launch where the back-substitution can ride along (device_base.hpp: BacksubFuse)
void DeviceNlp::solve_backsub_publish() {
  if (m_mode.fuse_backsub) {
    if (m_mode.dense && m_rhs_stale) build_rhs();
    const BacksubFuse f = backsub_fuse();
    m_ldlt.solve_after_factor(system(), &f);
    if (m_batch == 1) m_ldlt.stats_handed_to_host(++m_seq_expected);
    else m_ldlt.stats_handed_to_host();
  } else {
    solve_after_factor();
    backsub_and_publish(true);
  }
}

// p <- p + K_reg^-1 (b - K p), `iters` times: b = the right-hand side now in m_rhs, p = the
// solution of the last solve(), K = the unregularized matrix in m_lhs, K_reg = what was factored.
// Converges like (regularization / smallest eigenvalue)^iters.  Single problem.
void DeviceNlp::refine_solution(int iters) {
  materialize_kkt();
  if (m_batch != 1) throw std::runtime_error("slpx: refine_solution handles one problem");
  const int dim = m_kdev.dim;
  if (m_lhs_colptr.n == 0) {
    m_lhs_colptr.upload(m_k_ref.lhs.colptr);
    m_lhs_rowidx.upload(m_k_ref.lhs.rowidx);
    {
      // the strictly lower triangle by rows, entries of a row in column order
      const CscPattern& lp = m_k_ref.lhs;
      std::vector<int32_t> rowptr(dim + 1, 0), rowent, rowcol;
      for (int c = 0; c < dim; ++c)
        for (int q = lp.colptr[c]; q < lp.colptr[c + 1]; ++q)
          if (lp.rowidx[q] != c) ++rowptr[lp.rowidx[q] + 1];
      for (int i = 0; i < dim; ++i) rowptr[i + 1] += rowptr[i];
      rowent.resize(std::max(1, rowptr[dim]));
      rowcol.resize(std::max(1, rowptr[dim]));
      std::vector<int32_t> fill(rowptr.begin(), rowptr.end() - 1);
      for (int c = 0; c < dim; ++c)
        for (int q = lp.colptr[c]; q < lp.colptr[c + 1]; ++q)
          if (lp.rowidx[q] != c) {
            const int at = fill[lp.rowidx[q]]++;
            rowent[at] = q;
            rowcol[at] = c;
          }
      m_lhs_rowptr.upload(rowptr);
      m_lhs_rowent.upload(rowent);
      m_lhs_rowcol.upload(rowcol);
    }
    m_rhs0.alloc(dim);
    m_p_acc.alloc(dim);
  }
  SLPX_HIP_CHECK(hipMemcpyAsync(m_rhs0.p, m_rhs.p, dim * sizeof(double), hipMemcpyDeviceToDevice, m_stream));
  SLPX_HIP_CHECK(hipMemcpyAsync(m_p_acc.p, m_ldlt.d_p(), dim * sizeof(double), hipMemcpyDeviceToDevice, m_stream));
  for (int it = 0; it < iters; ++it) {
    SLPX_HIP_CHECK(hipMemcpyAsync(m_rhs.p, m_rhs0.p, dim * sizeof(double), hipMemcpyDeviceToDevice, m_stream));
    hipLaunchKernelGGL(sym_residual_kernel, dim3(grid_for(dim, 256)), dim3(256), 0, m_stream, dim, m_lhs_colptr.p,
                       m_lhs_rowidx.p, m_lhs_rowptr.p, m_lhs_rowent.p, m_lhs_rowcol.p, m_lhs.p, m_p_acc.p, m_rhs.p);
    solve();  // m_rhs -> m_p
    hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(dim, 256)), dim3(256), 0, m_stream, dim, m_ldlt.d_p(), m_p_acc.p);
  }
  SLPX_HIP_CHECK(hipMemcpyAsync(m_ldlt.d_p(), m_p_acc.p, dim * sizeof(double), hipMemcpyDeviceToDevice, m_stream));
  SLPX_HIP_CHECK(hipMemcpyAsync(m_rhs.p, m_rhs0.p, dim * sizeof(double), hipMemcpyDeviceToDevice, m_stream));
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::backsub() { backsub_and_publish(false); }

// back-substitution that also hands the counters of the factorization just enqueued to the
// host (read_stats() then needs no copy)
void DeviceNlp::backsub_publish() { backsub_and_publish(true); }

// publish: also copy the current attempt's counters to the pinned host buffer
void DeviceNlp::backsub_and_publish(bool publish) {
  if (m_kdev.m_i == 0 && !publish) return;
  hipLaunchKernelGGL(step_backsub_kernel, dim3(grid_for(std::max(1, m_kdev.m_i), 256), m_batch),
                     dim3(256), 0, m_stream, m_kdev, m_V.p, m_s_ref.nV, m_ldlt.d_p(), m_s.p, m_z.p, m_mu.p,
                     m_ps.p, m_pz.p, publish ? m_ldlt.stats_now() : nullptr, publish ? m_ldlt.stats_host() : nullptr, m_seq_dev.p,
                     (publish && m_batch == 1) ? m_h_seq : nullptr);
  if (publish) {
    if (m_batch == 1) m_ldlt.stats_handed_to_host(++m_seq_expected);
    else m_ldlt.stats_handed_to_host();
  }
  SLPX_HIP_CHECK(hipGetLastError());
}

// ============================================================================
// Interior-point iteration on the device (ipm_kernels.h)
// ============================================================================

void DeviceNlp::ipm_enable() {
  if (m_ipm) return;
  if (m_batch != 1) throw std::runtime_error("slpx: the device-resident IPM iteration handles one problem");
  const NlpStructure& s = m_s_ref;
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  m_trial_in.alloc(s.n_inputs());
  SLPX_HIP_CHECK(hipMemcpy(m_trial_in.p, m_in.p, s.n_inputs() * sizeof(double), hipMemcpyDeviceToDevice));
  m_V_trial.alloc(s.nV);
  // the trial V starts as a copy of V: static entries in place, the swept ones overwritten
  SLPX_HIP_CHECK(hipMemcpy(m_V_trial.p, m_V.p, static_cast<size_t>(s.nV) * sizeof(double), hipMemcpyDeviceToDevice));
  m_soc_ce.alloc(std::max(1, s.m_e));
  m_soc_cims.alloc(std::max(1, s.m_i));
  m_p_keep.alloc(m_kdev.dim);
  m_ps_keep.alloc(std::max(1, s.m_i));
  m_pz_keep.alloc(std::max(1, s.m_i));
  m_ipm_alpha.alloc(4);  // alpha_max, alpha_z, "this attempt's look-ahead chain is void", -
  m_ipm_alpha.zero();
  m_s_ahead.alloc(std::max(1, s.m_i));
  m_y_ahead.alloc(std::max(1, s.m_e));
  m_z_ahead.alloc(std::max(1, s.m_i));
  SLPX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m_ipm_host), 2 * sizeof(IpmHost)));
  std::memset(m_ipm_host, 0, 2 * sizeof(IpmHost));
  SLPX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m_ipm_ctl_host), 3 * sizeof(IpmCtl)));
  for (int k = 0; k < 3; ++k) m_ipm_ctl_host[k] = IpmCtl{};
  SLPX_HIP_CHECK(hipMalloc(&m_ipm_ctl_dev, sizeof(IpmCtl)));
  SLPX_HIP_CHECK(hipMemset(m_ipm_ctl_dev, 0, sizeof(IpmCtl)));
  m_ipm_gate.upload(std::vector<double>(1, 1.0));
  m_ipm = true;
}

void DeviceNlp::ipm_set_error_scaling(const std::vector<double>& scales) {
  if (static_cast<int>(scales.size()) != m_s_ref.n_scales())
    throw std::runtime_error("ipm_set_error_scaling: wrong length");
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  m_ipm_scales.upload(scales);
}

// After ipm_trial_metrics() / ipm_errors(): spins on the sequence number those launches
// publish (the stream is consulted now and then so a failed launch cannot hang the host).
void DeviceNlp::wait_published() {
  spin_on_published([&] { return *m_h_seq >= m_seq_expected; }, m_stream.raw(), "slpx: chain finished without publishing");
}

void DeviceNlp::wait() {
  hipError_t st;
  while ((st = hipStreamQuery(m_stream.raw())) == hipErrorNotReady) {
  }
  SLPX_HIP_CHECK(st);
}

void DeviceNlp::ipm_direction(double tau) {
  hipLaunchKernelGGL(ipm_direction_kernel, dim3(1), dim3(kIpmThreads), 0, m_stream, m_kdev, m_V.p, m_in.p, m_s.p,
                     m_z.p, m_ldlt.d_p(), m_ps.p, m_pz.p, m_mu.p, tau, m_trial_in.p, m_ipm_alpha.p, &m_ipm_host[m_ipm_slot].dir);
  SLPX_HIP_CHECK(hipGetLastError());
}

IpmLookaheadArgs DeviceNlp::lookahead_args(double tau, int twin_mode) {
  IpmLookaheadArgs a;
  a.n = m_kdev.n;
  a.m_e = m_kdev.m_e;
  a.m_i = m_kdev.m_i;
  a.g_src = m_kdev.g_src;
  a.V = m_V.p;
  a.in = m_in.p;
  a.s = m_s.p;
  a.y = m_y.p;
  a.z = m_z.p;
  a.p = m_ldlt.d_p();
  a.ps = m_ps.p;
  a.pz = m_pz.p;
  a.mu = m_mu.p;
  a.tau = tau;
  a.in_t = m_trial_in.p;
  a.s_t = m_s_ahead.p;
  a.y_t = m_y_ahead.p;
  a.z_t = m_z_ahead.p;
  a.alpha_dev = m_ipm_alpha.p;
  a.out = &m_ipm_host[m_ipm_slot].dir;
  a.stats = m_ldlt.stats_now();
  if (twin_mode != 0) {  // (a twin launch: the kernel takes the direction of the attempt the policy takes)
    a.tw.mode = twin_mode;
    a.tw.p = m_ldlt.d_p_twin();
    a.tw.ps = m_ps_tw.p;
    a.tw.pz = m_pz_tw.p;
    a.tw.stats = m_ldlt.twin_stats_now();
  }
  return a;
}

void DeviceNlp::ipm_lookahead(double tau) {
  hipLaunchKernelGGL(ipm_lookahead_kernel, dim3(1), dim3(kIpmThreads), 0, m_stream, lookahead_args(tau, m_ldlt.twin_mode()));
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::sweep_full_lookahead(bool with_reduce, bool skippable) {
  m_in_override = m_trial_in.p;
  m_V_override = m_V_trial.p;
  m_tape_reduce = with_reduce;  // false: the separable sums ride in ipm_errors(.., sums_ride, ahead)
  // (the generated kernel leaves at once when the look-ahead launch flagged the attempt as rejected: `chain` with
  // n_workgroups = 0 is that flag, tape_jit.cpp)
  if (skippable && m_full.n_bodies && m_ipm_alpha.p != nullptr) {
    m_chain_args = ChainArgs{reinterpret_cast<unsigned int*>(m_ipm_alpha.p + 2), 0u, 0u};
    m_chain_args.skip_flag = true;
  }
  launch_tape(m_full, true);
  m_chain_args = ChainArgs{};
  m_tape_reduce = true;
  m_in_override = nullptr;
  m_V_override = nullptr;
}

void DeviceNlp::ipm_accept_lookahead() {
  // every launch takes these pointers when it is made: the next step reads the accepted iterate
  m_in.swap(m_trial_in);
  m_s.swap(m_s_ahead);
  m_y.swap(m_y_ahead);
  m_z.swap(m_z_ahead);
  m_V.swap(m_V_trial);
  m_lhs_stale = m_rhs_stale = true;
}

void DeviceNlp::ipm_trial_point(double alpha) {
  hipLaunchKernelGGL(ipm_trial_point_kernel, dim3(grid_for(m_kdev.n, 256)), dim3(256), 0, m_stream, m_kdev.n,
                     m_in.p, m_ldlt.d_p(), alpha, m_trial_in.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::ipm_trial_metrics(double alpha, bool s_from_ci) {
  hipLaunchKernelGGL(ipm_trial_metrics_kernel, dim3(1), dim3(kIpmThreads), 0, m_stream, m_kdev, m_V_trial.p,
                     m_s.p, m_ps.p, alpha, m_ipm_alpha.p, s_from_ci ? 1 : 0, &m_ipm_host[m_ipm_slot].trial, m_seq_dev.p, m_h_seq,
                     m_reduces.p, static_cast<int>(m_reduces.n), m_scales.p);
  ++m_seq_expected;
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::ipm_commit(double alpha, double alpha_z, bool s_from_ci) {
  const int work = std::max({m_kdev.n, m_kdev.m_e, m_kdev.m_i, 1});
  hipLaunchKernelGGL(ipm_commit_kernel, dim3(grid_for(work, 256)), dim3(256), 0, m_stream, m_kdev, m_V_trial.p,
                     m_ldlt.d_p(), m_ps.p, m_pz.p, alpha, alpha_z, m_mu.p, s_from_ci ? 1 : 0, m_in.p, m_s.p, m_y.p,
                     m_z.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

// `sums_ride`: the sweep before this call left the tape's separable sums out
// (sweep_full(false)); they ride in this launch
void DeviceNlp::ipm_errors(bool check_all_V, bool sums_ride, bool ahead) {
  const int work = std::max({m_kdev.n, m_kdev.m_e, m_kdev.m_i, 1});
  // eight lanes per column (ipm_error_accumulate): up to 64 workgroups of 256
  const int blocks = grid_for(8 * work, kIpmErrThreads, 64);
  if (m_ipm_partial.n < static_cast<size_t>(blocks) * kIpmErrQ) m_ipm_partial.alloc(static_cast<size_t>(256) * kIpmErrQ);
  if (m_ipm_err_done.n == 0) m_ipm_err_done.upload(std::vector<unsigned int>(1, 0u));
  const int n_sums = sums_ride ? static_cast<int>(m_reduces.n) : 0;
  IpmErrFinish fin;
  fin.n_err_blocks = blocks;
  fin.n_total_blocks = blocks + n_sums;
  fin.red = m_reduces.p;
  fin.tape_scales = m_scales.p;
  fin.Vw = ahead ? m_V_trial.p : m_V.p;
  fin.done = m_ipm_err_done.p;
  fin.out = ahead ? &m_ipm_host[m_ipm_slot].err_ahead : &m_ipm_host[m_ipm_slot].err;
  if (ahead && m_errors_decide) {
    fin.ctl = static_cast<IpmCtl*>(m_ipm_ctl_dev);
    fin.dir = m_ipm_alpha.p;
    fin.gate = m_ipm_gate.p;
    fin.go_host = &m_ipm_host[m_ipm_slot].go;
  }
  fin.seq_dev = m_seq_dev.p;
  fin.seq_host = m_h_seq;
  fin.skip = ahead ? m_ipm_alpha.p + 2 : nullptr;
  hipLaunchKernelGGL(ipm_error_partial_kernel, dim3(blocks + n_sums), dim3(kIpmErrThreads), 0, m_stream, m_kdev, fin.Vw,
                     m_s_ref.nV, ahead ? m_trial_in.p : m_in.p, ahead ? m_s_ahead.p : m_s.p, ahead ? m_y_ahead.p : m_y.p,
                     ahead ? m_z_ahead.p : m_z.p, m_ipm_scales.p, check_all_V ? 1 : 0, m_ipm_partial.p, fin);
  ++m_seq_expected;
  SLPX_HIP_CHECK(hipGetLastError());
}

bool DeviceNlp::ipm_ride_errors_in_next_step(int slot_out) {
  if (!ipm_ride_possible()) return false;
  m_ride_next = true;
  m_ride_slot = slot_out;
  return true;
}

bool DeviceNlp::ipm_ride_possible() {
  if (!twin_ready()) return false;
  if (m_mode.ride < 0) {
    int per_cu = 0;
    if (m_sw.ipm_ride) {
      per_cu = m_ldlt.riding_twin_workgroups_per_cu();
      if (m_ipm_ride_verdict.n == 0) m_ipm_ride_verdict.upload(std::vector<double>(1, 0.0));
    }
    choose_ride(m_mode, m_plan, m_reduces.n, static_cast<size_t>(per_cu) * m_cus, m_sw);
    if (m_sw.ipm_ride && std::getenv("SLPX_LDLT_VERBOSE"))
      std::fprintf(stderr, "ldlt riding error launch: %zu workgroups, %d of %d threads per CU x %d CUs%s\n", riding_workgroups(m_plan, m_reduces.n),
                   per_cu, m_mode.twin_threads, m_cus, m_mode.ride ? "" : ": NOT resident at once");
  }
  return m_mode.ride != 0;
}

// The armed error launch (ipm_ride_errors_in_next_step) as the next twin launch carries it: its workgroups in front of
// the tasks, on the CURRENT buffers — the look-ahead iterate has been made current —, the tape's sums with them
MfRide DeviceNlp::ipm_take_ride() {
  m_ride_next = false;
  const int work = std::max({m_kdev.n, m_kdev.m_e, m_kdev.m_i, 1});
  const int blocks = grid_for(8 * work, kIpmErrThreads, 64);
  if (m_ipm_partial.n < static_cast<size_t>(blocks) * kIpmErrQ) m_ipm_partial.alloc(static_cast<size_t>(256) * kIpmErrQ);
  if (m_ipm_err_done.n == 0) m_ipm_err_done.upload(std::vector<unsigned int>(1, 0u));
  const int n_sums = static_cast<int>(m_reduces.n);
  m_ride_ticket += 1.0;
  MfRide ride;
  ride.n_blocks = static_cast<uint32_t>(blocks + n_sums);
  ride.K = m_kdev;
  ride.V = m_V.p;
  ride.x = m_in.p;
  ride.s = m_s.p;
  ride.y = m_y.p;
  ride.z = m_z.p;
  ride.scales = m_ipm_scales.p;
  ride.nV = m_s_ref.nV;
  ride.partial = m_ipm_partial.p;
  IpmErrFinish& fin = ride.fin;
  fin.n_err_blocks = blocks;
  fin.n_total_blocks = blocks + n_sums;
  fin.red = m_reduces.p;
  fin.tape_scales = m_scales.p;
  fin.Vw = m_V.p;
  fin.done = m_ipm_err_done.p;
  fin.out = &m_ipm_host[m_ride_slot].err_ahead;
  fin.ctl = static_cast<IpmCtl*>(m_ipm_ctl_dev);
  fin.dir = m_ipm_alpha.p;
  fin.gate = m_ipm_gate.p;
  fin.go_host = &m_ipm_host[m_ride_slot].go;
  fin.check_host = &m_ipm_host[m_ride_slot].check;
  fin.ride_verdict = m_ipm_ride_verdict.p;
  fin.ride_ticket = m_ride_ticket;
  return ride;
}

bool DeviceNlp::ipm_ride_wait(int slot_out) {
  volatile IpmHost* h = &m_ipm_host[slot_out];
  const double ticket = m_ride_ticket;
  double verdict = 0.0;
  // (the verdict AND every word it announces: writes to host memory may arrive in any order — IpmHost::check)
  auto handed_over = [&] {
    const double go = h->go;
    if (std::fabs(go) != ticket) return false;
    unsigned long long bits = std::bit_cast<unsigned long long>(go);
    const volatile unsigned long long* w = reinterpret_cast<const volatile unsigned long long*>(&h->err_ahead);
    for (size_t k = 0; k < sizeof(IpmErrOut) / sizeof(unsigned long long); ++k) bits ^= w[k];
    if (bits != h->check) return false;
    verdict = go;
    return true;
  };
  spin_on_published(handed_over, m_stream.raw(), "slpx: a riding error launch finished without its verdict");
  return verdict > 0.0;
}

void DeviceNlp::ipm_errors_deciding(bool sums_ride) {
  m_errors_decide = true;
  ipm_errors(false, sums_ride, /*ahead=*/true);
  m_errors_decide = false;
}

// (only the used part of the filter's table travels, either way)
static size_t ipm_ctl_bytes(const IpmCtl& c) { return offsetof(IpmCtl, filter) + offsetof(FilterState, ent) + 16u * static_cast<size_t>(c.filter.n); }
void DeviceNlp::ipm_pipeline_upload(const IpmCtl& ctl) {
  m_ipm_ctl_stage = 1 + (m_ipm_ctl_stage & 1);  // (1, 2, 1, ...: the copy of the upload before this one has long run)
  IpmCtl& stage = m_ipm_ctl_host[m_ipm_ctl_stage];
  std::memcpy(&stage, &ctl, ipm_ctl_bytes(ctl));
  SLPX_HIP_CHECK(hipMemcpyAsync(m_ipm_ctl_dev, &stage, ipm_ctl_bytes(ctl), hipMemcpyHostToDevice, m_stream));
}
const IpmCtl& DeviceNlp::ipm_pipeline_fetch() {
  IpmCtl& into = m_ipm_ctl_host[0];
  // (the head says how long the table is)
  SLPX_HIP_CHECK(hipMemcpyAsync(&into, m_ipm_ctl_dev, offsetof(IpmCtl, filter) + offsetof(FilterState, ent), hipMemcpyDeviceToHost, m_stream));
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  if (into.filter.n > 0) {
    SLPX_HIP_CHECK(hipMemcpyAsync(into.filter.ent, static_cast<const char*>(m_ipm_ctl_dev) + offsetof(IpmCtl, filter) + offsetof(FilterState, ent),
                                  16u * static_cast<size_t>(into.filter.n), hipMemcpyDeviceToHost, m_stream));
    SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  }
  return into;
}

void DeviceNlp::wait_published_until(unsigned long long seq) {
  spin_on_published([&] { return *m_h_seq >= seq; }, m_stream.raw(), "slpx: chain finished without publishing");
}

void DeviceNlp::ipm_soc_accumulate(double alpha, bool first, bool s_from_ci) {
  const int work = std::max({m_kdev.m_e, m_kdev.m_i, 1});
  hipLaunchKernelGGL(ipm_soc_accumulate_kernel, dim3(grid_for(work, 256)), dim3(256), 0, m_stream, m_kdev, m_V.p,
                     m_V_trial.p, m_s.p, m_ps.p, alpha, first ? 1 : 0, s_from_ci ? 1 : 0, m_soc_ce.p,
                     m_soc_cims.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::ipm_soc_rhs() {
  m_rhs_stale = false;
  m_rhs_in_il = false;
  hipLaunchKernelGGL(ipm_soc_rhs_kernel, dim3(grid_for(m_kdev.dim, 256)), dim3(256), 0, m_stream, m_kdev, m_V.p,
                     m_s.p, m_y.p, m_z.p, m_mu.p, m_soc_ce.p, m_soc_cims.p, m_rhs.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::ipm_soc_backsub() {
  if (m_kdev.m_i == 0) return;
  hipLaunchKernelGGL(ipm_soc_backsub_kernel, dim3(grid_for(m_kdev.m_i, 256)), dim3(256), 0, m_stream, m_kdev,
                     m_V.p, m_ldlt.d_p(), m_s.p, m_z.p, m_mu.p, m_soc_cims.p, m_ps.p, m_pz.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::ipm_save_direction() {
  hipLaunchKernelGGL(ipm_copy_direction_kernel, dim3(grid_for(m_kdev.dim, 256)), dim3(256), 0, m_stream, m_kdev.dim, m_kdev.m_i,
                     m_ldlt.d_p(), m_ps.p, m_pz.p, m_p_keep.p, m_ps_keep.p, m_pz_keep.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceNlp::ipm_restore_direction() {
  hipLaunchKernelGGL(ipm_copy_direction_kernel, dim3(grid_for(m_kdev.dim, 256)), dim3(256), 0, m_stream, m_kdev.dim, m_kdev.m_i,
                     m_p_keep.p, m_ps_keep.p, m_pz_keep.p, m_ldlt.d_p(), m_ps.p, m_pz.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

}  // namespace slpx
