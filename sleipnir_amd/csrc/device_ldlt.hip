// DeviceLdlt (device_ldlt.hpp): the LDLᵀ kernels for gfx950 and everything that launches, sizes or measures them.
// See DESIGN.md §3 for the roofline of each.
//
//   ldlt_factor    (ldlt_kernels.h) one round of the task-parallel left-looking LDLᵀ
//                  + inertia (sparse_regularized_ldlt.hpp:74-83,105-109, inertia.hpp:40-50)
//   ldlt_fwd/bwd   (ldlt_kernels.h) triangular solves (sparse_regularized_ldlt.hpp:159-161)
//   ldlt_*_il      (ldlt_il_kernels.h) the same, batch-interleaved
//   ldlt_dense_*   (ldlt_dense_kernels.h) the dense branch, plain or pivoted
//   ldlt_mf_*      (ldlt_mf_kernels.h) the one-launch multifrontal step, its twin, the solve through the fronts
//
// This is the ONLY translation unit that includes those four headers: a kernel template instantiated in two files is
// two device functions, and an attribute set or an occupancy measured on one says nothing about the other.
#include <hip/hip_runtime.h>

#include <chrono>

#include <algorithm>
#include <bit>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device_ldlt.hpp"
#include "device_images.hpp"
#include "ldlt_kernels.h"
#include "ldlt_mf_kernels.h"
#include "ldlt_dense_kernels.h"
#include "ldlt_il_kernels.h"

namespace slpx {

void LdltPlanDevice::upload(const LdltPlan& l) {
  tasks.upload(l.tasks);
  ent_src.upload(l.ent_src);
  ent_flags.upload(l.ent_flags);
  ent_col.upload(l.ent_col);
  ent_out.upload(l.ent_out);
  ent_pair_ptr.upload(l.ent_pair_ptr);
  ent_contrib_ptr.upload(l.ent_contrib_ptr);
  contrib_idx.upload(l.contrib_idx);
  ext_dst.upload(l.ext_dst);
  lvl_ptr.upload(l.lvl_ptr);
  pairs.upload(l.pairs);
  col_perm.upload(l.col_perm);
  col_lvl_ptr.upload(l.col_lvl_ptr);
  fwd_ptr.upload(l.fwd_ptr);
  fwd_contrib_ptr.upload(l.fwd_contrib_ptr);
  scontrib_idx.upload(l.scontrib_idx);
  fwd_items.upload(l.fwd_items);
  sext_ptr.upload(l.sext_ptr);
  sext_dst.upload(l.sext_dst);
  sext_items.upload(l.sext_items);
  bwd_ptr.upload(l.bwd_ptr);
  bwd_items.upload(l.bwd_items);
  perm.upload(l.perm);
  round_ptr.upload(l.round_ptr);
  sn_desc.upload(l.sn_desc);
  sn_lvl_ptr.upload(l.sn_lvl_ptr);
  col_sn.upload(l.col_sn);
  const LdltLevelTables lt = pack_ldlt_level_tables(l);
  lvl_pack.upload(lt.lvl_pack);
  col_lvl_pack.upload(lt.col_lvl_pack);
  bwd_range.upload(lt.bwd_range);
  n_rounds = l.n_rounds;
}

LdltDev LdltPlanDevice::view() const {
  LdltDev L{};
  L.tasks = tasks.p;
  L.ent_src = ent_src.p;
  L.ent_flags = ent_flags.p;
  L.ent_col = ent_col.p;
  L.ent_out = ent_out.p;
  L.ent_pair_ptr = ent_pair_ptr.p;
  L.ent_contrib_ptr = ent_contrib_ptr.p;
  L.contrib_idx = contrib_idx.p;
  L.ext_dst = ext_dst.p;
  L.lvl_ptr = lvl_ptr.p;
  L.pairs = pairs.p;
  L.col_perm = col_perm.p;
  L.col_lvl_ptr = col_lvl_ptr.p;
  L.fwd_ptr = fwd_ptr.p;
  L.fwd_contrib_ptr = fwd_contrib_ptr.p;
  L.scontrib_idx = scontrib_idx.p;
  L.fwd_items = fwd_items.p;
  L.sext_ptr = sext_ptr.p;
  L.sext_dst = sext_dst.p;
  L.sext_items = sext_items.p;
  L.bwd_ptr = bwd_ptr.p;
  L.bwd_items = bwd_items.p;
  L.perm = perm.p;
  L.round_ptr = round_ptr.p;
  L.n_rounds = n_rounds;
  L.sn_desc = sn_desc.p;
  L.sn_lvl_ptr = sn_lvl_ptr.p;
  L.col_sn = col_sn.p;
  L.lvl_pack = lvl_pack.p;
  L.col_lvl_pack = col_lvl_pack.p;
  L.bwd_range = bwd_range.p;
  L.clock_task = 0xffffffffu;
  return L;
}

DeviceLdlt::DeviceLdlt(const LdltPlan& l, const KktPlan& k, int batch, const Shared& sh)
    : m_l(l), m_k(k), m_batch(batch), m_nnz_lhs(k.lhs.nnz()), m_stream(sh.stream), m_mode(sh.mode), m_facts(sh.facts), m_sw(sh.sw),
      m_cus(sh.cus), m_h_seq(sh.seq_host), m_n_sums(sh.n_sums) {}

DeviceLdlt::~DeviceLdlt() {
  if (m_h_reg) (void)hipHostFree(m_h_reg);
  if (m_h_stats) (void)hipHostFree(m_h_stats);
}

int DeviceLdlt::workgroups_per_cu(const void* kernel, int threads, size_t lds, size_t* static_lds) {
  int per_cu = 0;
  SLPX_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (static_lds != nullptr) {
    hipFuncAttributes attr{};
    SLPX_HIP_CHECK(hipFuncGetAttributes(&attr, kernel));
    *static_lds = std::max(*static_lds, attr.sharedSizeBytes);
  }
  SLPX_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds));
  return per_cu;
}

// allow > 64 KB dynamic LDS
void DeviceLdlt::raise_lds_limits() {
  for (const void* fn : {reinterpret_cast<const void*>(&ldlt_factor_kernel<256>),
                         reinterpret_cast<const void*>(&ldlt_factor_kernel<1024>),
                         reinterpret_cast<const void*>(&ldlt_fwd_kernel),
                         reinterpret_cast<const void*>(&ldlt_bwd_kernel)})
    SLPX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
}

void DeviceLdlt::upload_plan() {
  m_lplan.upload(m_l);
  m_ldev = m_lplan.view();
  // the round counters of the single-launch kernels ([2][batch][n_rounds]), cleared once here
  std::vector<unsigned int> zero(2 * static_cast<size_t>(m_batch) * std::max(1, m_l.n_rounds), 0u);
  m_fround_cnt.upload(zero);
  m_bround_cnt.upload(zero);
}

// the dense branch: dim x dim per problem, the pattern of lhs for the scatter; LDS: column k and its scaled copy
void DeviceLdlt::alloc_dense_buffers() {
  if (!m_mode.dense) return;
  const KktPlan& k = m_k;
  const LdltPlan& l = m_l;
  const size_t B = static_cast<size_t>(m_batch);
  m_dense_A.alloc(B * static_cast<size_t>(l.n) * l.n);
  m_dense_colptr.upload(k.lhs.colptr);
  m_dense_rowidx.upload(k.lhs.rowidx);
  m_dense_lds = 16u * static_cast<uint32_t>(l.n) + 320u;
  if (m_mode.dense_pivoted) {
    m_dense_trans.alloc(B * static_cast<size_t>(l.n));
    m_dense_trans.zero();
    SLPX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ldlt_dense_pivoted_factor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  if (m_dense_lds > 160u * 1024u) throw std::runtime_error("slpx: the dense factorization holds two columns in LDS: at most 10 000 rows");
  SLPX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ldlt_dense_factor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  SLPX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ldlt_dense_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
}

void DeviceLdlt::alloc_value_buffers() {
  const LdltPlan& l = m_l;
  const size_t B = static_cast<size_t>(m_batch);
  m_p.alloc(B * m_k.dim);
  m_D.alloc(B * l.n);
  m_Lx.alloc(B * std::max<int64_t>(1, l.nnzL));
  m_contrib.alloc(B * std::max<uint32_t>(1, l.n_contrib));
  m_scontrib.alloc(B * std::max<uint32_t>(1, l.n_scontrib));
  m_zv.alloc(B * l.n);
  m_xg.alloc(B * l.n);
  // Every value buffer starts at zero, not at whatever the allocator hands back: the right-hand
  // side rides in the factorization as an extra row, and compute() may come before any rhs was
  // set (RegularizedLDLT::compute(lhs), regularized_ldlt.hpp:72) — recycled memory of an earlier
  // system can hold the hand-over sentinel (a NaN pattern: the armed slots below), a NaN keeps
  // its payload through arithmetic, and an update block that IS the sentinel is never taken
  // (seen on the pair-list kernels: the fourth solver of a process spinning to its time-out).
  for (DevBuf<double>* buf : {&m_p, &m_D, &m_Lx, &m_scontrib, &m_zv}) buf->zero();
}

// What the kernels hand over through the data starts out armed (kSlotEmpty), the counters cleared.
void DeviceLdlt::arm_handover_buffers() {
  const LdltPlan& l = m_l;
  const size_t B = static_cast<size_t>(m_batch);
  const double empty = std::bit_cast<double>(kSlotEmpty);
  if (m_mode.slot_handoff) {
    const std::vector<double> armed(m_contrib.n, empty);
    SLPX_HIP_CHECK(hipMemcpy(m_contrib.p, armed.data(), armed.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // the backward solve's hand-over through the data (ldlt_kernels.h: slot_read): two buffers of
  // x, both armed
  if (m_mode.xg_by_data) {
    const std::vector<double> armed(B * l.n, empty);
    m_xg.upload(armed);
    m_xg2.upload(armed);
  }
  // two inertia-counter buffers (see factor()), both cleared once here
  m_stats.upload(std::vector<LdltStats>(2 * B, LdltStats{0, 0, 0, 0, 0x7ff0000000000000ull}));
}

// batch-interleaved LDLT (ldlt_il_kernels.h): [chunk of 64 problems][index][lane]
void DeviceLdlt::alloc_interleaved_buffers() {
  if (!m_mode.il) return;
  const LdltPlan& l = m_l;
  const size_t B = static_cast<size_t>(m_batch);
  const size_t C = (B + 63) / 64, W = 64;
  m_Lx_il.alloc(C * std::max<int64_t>(1, l.nnzL) * W);
  m_D_il.alloc(C * l.n * W);
  m_contrib_il.alloc(C * std::max<uint32_t>(1, l.n_contrib) * W);
  m_scontrib_il.alloc(C * std::max<uint32_t>(1, l.n_scontrib) * W);
  m_zv_il.alloc(C * l.n * W);
  m_xg_il.alloc(C * l.n * W);
  m_stats_part.alloc(l.tasks.size() * B);
  for (auto* buf : {&m_Lx_il, &m_D_il, &m_zv_il, &m_xg_il, &m_contrib_il, &m_scontrib_il}) buf->zero();
  const IlMeta im = pack_il_meta(l);
  m_il_meta.upload(im.meta);
  m_il_meta_off.upload(im.meta_off);
  m_il_factor_lds = im.factor_lds;
  m_il_solve_lds = im.solve_lds;
  if (m_il_factor_lds > 160u * 1024u)
    throw std::runtime_error("slpx: an LDLT task does not fit the interleaved kernel's LDS (LdltOptions::task_entries)");
  SLPX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ldlt_factor_il_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  SLPX_HIP_CHECK(hipDeviceSynchronize());
}

// what the host and the kernels pass each other through pinned memory: (delta, gamma), the counters
void DeviceLdlt::alloc_pinned() {
  const size_t B = static_cast<size_t>(m_batch);
  SLPX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m_h_reg), 2 * static_cast<size_t>(std::max<int>(B, 6)) * sizeof(double)));  // (B = 1: a twin attempt's second pair)
  if (B > 8) m_reg_dev.alloc(2 * B);
  SLPX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m_h_stats), static_cast<size_t>(std::max<int>(B, 2)) * sizeof(LdltStats)));
}

constexpr int kFactorThreadsSingle = 1024;
// The multifrontal step (ldlt_mf_kernels.h) with the task images of build_mf_images: co-residency of every task's
// workgroup, then the uploads.
void DeviceLdlt::upload_mf(const MfImages& im) {
  const LdltPlan& l = m_l;
  MfFit fit;
  fit.declined = im.declined != nullptr;
  fit.lds_bytes = im.lds;
  int per_cu[2] = {0, 0};  // at 1024, at 512 threads
  if (!fit.declined && im.lds <= 160u * 1024u) {
    auto fp = [](auto kernel) { return reinterpret_cast<const void*>(kernel); };
    const bool mfma = l.mf_n_mfma > 0;
    auto both = [&](const void* chained, const void* plain, int threads) {
      return std::min(workgroups_per_cu(chained, threads, im.lds, &fit.static_lds_bytes), workgroups_per_cu(plain, threads, im.lds, &fit.static_lds_bytes));
    };
    per_cu[0] = mfma ? both(fp(&ldlt_mf_step_kernel<1024, true, true>), fp(&ldlt_mf_step_kernel<1024, true, false>), 1024)
                     : both(fp(&ldlt_mf_step_kernel<1024, false, true>), fp(&ldlt_mf_step_kernel<1024, false, false>), 1024);
    per_cu[1] = mfma ? both(fp(&ldlt_mf_step_kernel<512, true, true>), fp(&ldlt_mf_step_kernel<512, true, false>), 512)
                     : both(fp(&ldlt_mf_step_kernel<512, false, true>), fp(&ldlt_mf_step_kernel<512, false, false>), 512);
    fit.step = Residency{static_cast<size_t>(per_cu[0]) * m_cus, static_cast<size_t>(per_cu[1]) * m_cus};
    if (m_sw.mf_solve)
      fit.solve = Residency{static_cast<size_t>(workgroups_per_cu(fp(&ldlt_mf_solve_kernel<1024>), 1024, im.lds)) * m_cus,
                            static_cast<size_t>(workgroups_per_cu(fp(&ldlt_mf_solve_kernel<512>), 512, im.lds)) * m_cus};
  }
  choose_multifrontal(m_mode, m_facts, m_n_sums, fit, m_sw);
  if (fit.declined) return;
  if (std::getenv("SLPX_LDLT_VERBOSE"))
    std::fprintf(stderr, "ldlt multifrontal step: %zu tasks, LDS %u bytes (static %zu), images %zu bytes, %d workgroup(s) of %d threads per CU x %d CUs%s\n",
                 l.tasks.size(), im.lds, fit.static_lds_bytes, 16 * im.image.size(), per_cu[m_mode.mf_threads == 1024 ? 0 : 1], m_mode.mf_threads, m_cus,
                 m_mode.mf ? "" : ": NOT resident at once");
  if (!m_mode.mf) return;
  m_mf_tasks.upload(l.mf_tasks);
  m_mf_fronts.upload(l.mf_fronts);
  m_mf_image.upload(im.image);
  m_mf_image_stride16 = im.stride16;
  m_mf_image_desc.upload(im.desc);
  m_mf_contrib.upload(std::vector<double>(std::max<uint32_t>(1, l.mf_n_contrib), std::bit_cast<double>(kSlotEmpty)));
  if (m_exit_cnt.n == 0) m_exit_cnt.upload(std::vector<unsigned int>(1, 0u));
  m_mf_lds = im.lds;
}

void DeviceLdlt::download(const double* dev, double* host, size_t count) {
  SLPX_HIP_CHECK(hipMemcpyAsync(host, dev, count * sizeof(double), hipMemcpyDeviceToHost, m_stream));
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
}

void DeviceLdlt::to_interleaved(const double* batch_major, int count, double* il, hipStream_t stream) {
  const int C = (m_batch + 63) / 64;
  hipLaunchKernelGGL(il_gather_kernel, dim3((count + 63) / 64, C), dim3(256), 0, stream, batch_major, static_cast<long long>(count), count,
                     il, m_batch);
}
void DeviceLdlt::to_batch_major(const double* il, int count, double* batch_major) {
  const int C = (m_batch + 63) / 64;
  hipLaunchKernelGGL(il_scatter_kernel, dim3((count + 63) / 64, C), dim3(256), 0, m_stream, il, count, batch_major,
                     static_cast<long long>(count), m_batch);
}

void DeviceLdlt::debug_clocks(unsigned int next_round, unsigned long long* out24) {
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
#ifdef SLPX_MF_CLOCKS
  if ((next_round >> 16) == 0xffffu) {  // (the instrumented build: the slots of task (next_round & 0xffff) in the last launch)
    SLPX_HIP_CHECK(hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_mf_clocks), 24 * sizeof(unsigned long long),
                                       24 * sizeof(unsigned long long) * (next_round & 0xffffu)));
    return;
  }
#endif
  SLPX_HIP_CHECK(hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_ldlt_clocks), 24 * sizeof(unsigned long long)));
  // (bits 8 and up: which task of the round, 0 = its first)
  const unsigned int round = next_round & 0xffu, within = next_round >> 8;
  m_ldev.clock_task = 0xffffffffu;
  if (round < static_cast<unsigned int>(m_l.n_rounds) && m_l.round_ptr[round] + within < m_l.round_ptr[round + 1])
    m_ldev.clock_task = m_l.round_ptr[round] + within;
}

// Control traffic of one factorization attempt is kept off the critical path: the kernels
// read (δ, γ) straight from pinned host memory (δ = NaN marks a problem the policy loop is
// done with), and the inertia counters are double-buffered — the launch of attempt k
// clears the buffer attempt k+1 will accumulate into — so no copy and no reset kernel run.
// The host only rewrites m_h_reg after read_stats() has synchronized.
void DeviceLdlt::write_reg(const std::vector<double>& delta, const std::vector<double>& gamma,
                           const std::vector<uint8_t>& active) {
  for (int b = 0; b < m_batch; ++b) {
    m_h_reg[2 * b] = active[b] ? delta[b] : std::numeric_limits<double>::quiet_NaN();
    m_h_reg[2 * b + 1] = gamma[b];
    if (active[b]) note_factored(b, delta[b], gamma[b]);
  }
}

void DeviceLdlt::enqueue_factor(int parity, hipStream_t stream, const LdltSystem& sys, const KktFuse& f) {
  const LdltPlan& l = m_l;
  LdltStats* cur = m_stats.p + static_cast<size_t>(parity) * m_batch;
  LdltStats* next = m_stats.p + static_cast<size_t>(parity ^ 1) * m_batch;
  const long long lxs = static_cast<long long>(std::max<int64_t>(1, l.nnzL));
  const int cs = static_cast<int>(std::max<uint32_t>(1, l.n_contrib));
  // a handful of workgroups read (δ, γ) straight from pinned host memory; the tens of
  // thousands of a big batch would each pay a PCIe round trip, so those get a device copy
  const double* reg = m_h_reg;
  if (m_batch > 8) {
    // (only when the values changed: consecutive steps of a batch mostly make the same first attempt, and the copy is a
    // launch of its own in front of every factorization — 6 us of a 64-problem step's 280, 21 us of a 512-problem step's)
    const size_t count = 2 * static_cast<size_t>(m_batch);
    if (m_reg_shadow.size() != count || std::memcmp(m_reg_shadow.data(), m_h_reg, count * sizeof(double)) != 0) {
      m_reg_shadow.assign(m_h_reg, m_h_reg + count);
      SLPX_HIP_CHECK(hipMemcpyAsync(m_reg_dev.p, m_h_reg, count * sizeof(double), hipMemcpyHostToDevice, stream));
    }
    reg = m_reg_dev.p;
  }
  if (m_mode.dense) {
    if (m_mode.dense_pivoted)
      hipLaunchKernelGGL(ldlt_dense_pivoted_factor_kernel, dim3(m_batch), dim3(kDenseThreads), m_dense_lds, stream, l.n, l.n_dec,
                         m_dense_colptr.p, m_dense_rowidx.p, m_nnz_lhs, sys.lhs, reg, m_dense_A.p, m_dense_trans.p, m_D.p, cur, next);
    else
    hipLaunchKernelGGL(ldlt_dense_factor_kernel, dim3(m_batch), dim3(kDenseThreads), m_dense_lds, stream, l.n, l.n_dec,
                       m_dense_colptr.p, m_dense_rowidx.p, m_nnz_lhs, sys.lhs, reg, m_dense_A.p, m_D.p, m_Lx.p, lxs, cur, next);
    SLPX_HIP_CHECK(hipGetLastError());
    return;
  }
  if (m_mode.il) {
    const int C = (m_batch + 63) / 64;
    const int nnz = m_nnz_lhs;
    // (the assembly kernels wrote the interleaved arrays themselves unless somebody else made lhs / rhs)
    if (!sys.lhs_in_il) to_interleaved(sys.lhs, nnz, sys.lhs_il, stream);
    if (!sys.rhs_in_il) to_interleaved(sys.rhs, l.n, sys.rhs_il, stream);
    for (int r = 0; r < l.n_rounds; ++r) {
      const uint32_t nt = l.round_ptr[r + 1] - l.round_ptr[r];
      hipLaunchKernelGGL(ldlt_factor_il_kernel, dim3(nt, kIlRowsPerChunk * C), dim3(kIlFactorThreads), m_il_factor_lds, stream, m_ldev,
                         l.round_ptr[r], sys.lhs_il, nnz, sys.rhs_il, l.n, reg, m_Lx_il.p, lxs, m_D_il.p,
                         m_contrib_il.p, cs, m_zv_il.p, m_stats_part.p, m_batch, m_il_meta.p, m_il_meta_off.p);
    }
    hipLaunchKernelGGL(ldlt_stats_il_kernel, dim3(m_batch), dim3(64), 0, stream, m_stats_part.p,
                       static_cast<int>(l.tasks.size()), reg, cur, m_batch);
    m_il_outputs_stale = true;
  } else if (m_mode.single_launch) {
    // every round in one launch; tasks wait on device-side round counters
    hipLaunchKernelGGL(ldlt_factor_kernel<kFactorThreadsSingle>,
                       dim3(static_cast<uint32_t>(l.tasks.size()) + static_cast<uint32_t>(f.n_blocks), m_batch),
                       dim3(kFactorThreadsSingle), f.inline_kkt ? m_factor_lds_inline : l.factor_lds_bytes, stream,
                       m_ldev, 0u, sys.lhs, m_nnz_lhs, reg, m_Lx.p, lxs, m_D.p, l.n, m_contrib.p, cs, cur, next,
                       sys.rhs, m_zv.p, m_fround_cnt.p, m_mode.slot_handoff ? 1 : 0, f);
  } else {
    for (int r = 0; r < l.n_rounds; ++r) {
      const uint32_t nt = l.round_ptr[r + 1] - l.round_ptr[r];
      hipLaunchKernelGGL(ldlt_factor_kernel<256>, dim3(nt, m_batch), dim3(256), l.factor_lds_bytes, stream,
                         m_ldev, l.round_ptr[r], sys.lhs, m_nnz_lhs, reg, m_Lx.p, lxs, m_D.p,
                         l.n, m_contrib.p, cs, cur, r == 0 ? next : nullptr, sys.rhs, m_zv.p,
                         static_cast<unsigned int*>(nullptr), 0, KktFuse{});
    }
  }
  SLPX_HIP_CHECK(hipGetLastError());
}

void DeviceLdlt::factor(const std::vector<double>& delta, const std::vector<double>& gamma, const std::vector<uint8_t>& active,
                        const LdltSystem& sys, const KktFuse& f) {
  write_reg(delta, gamma, active);
  m_twin_mode = 0;
  m_stats_cur ^= 1;
  m_stats_in_host = false;
  enqueue_factor(m_stats_cur, m_stream, sys, f);
}

// ---- twin attempt (ldlt_mf_twin_kernel) ----
bool DeviceLdlt::twin_available() {
  if (m_mode.twin != 0) return m_mode.twin > 0 && m_mode.mf && xg_other() != nullptr;
  const LdltPlan& l = m_l;
  auto fp = [](auto kernel) { return reinterpret_cast<const void*>(kernel); };
  int per_cu[2] = {0, 0};  // at 1024, at 512 threads
  const bool measure = twin_worth_measuring(m_mode, m_batch, m_sw);
  if (measure) {
    if (m_mode.mf_threads == 1024) per_cu[0] = workgroups_per_cu(fp(&ldlt_mf_twin_kernel<1024, false>), 1024, m_mf_lds);
    per_cu[1] = workgroups_per_cu(fp(&ldlt_mf_twin_kernel<512, false>), 512, m_mf_lds);
  }
  choose_twin(m_mode, m_batch, m_facts, m_n_sums, Residency{static_cast<size_t>(per_cu[0]) * m_cus, static_cast<size_t>(per_cu[1]) * m_cus}, m_sw);
  if (measure && std::getenv("SLPX_LDLT_VERBOSE"))
    std::fprintf(stderr, "ldlt twin attempt: 2 x %zu tasks, %d workgroup(s) of %d threads per CU x %d CUs%s\n", l.tasks.size(),
                 per_cu[m_mode.twin_threads == 1024 ? 0 : 1], m_mode.twin_threads, m_cus, m_mode.twin > 0 ? "" : ": NOT resident at once");
  if (m_mode.twin < 0) return false;
  for (auto [tw, first] : {std::pair{&m_Lx_tw, &m_Lx}, {&m_D_tw, &m_D}, {&m_zv_tw, &m_zv}, {&m_p_tw, &m_p}}) {
    tw->alloc(std::max<size_t>(1, first->n));
    tw->zero();
  }
  m_mf_contrib_tw.upload(std::vector<double>(std::max<size_t>(1, m_mf_contrib.n), std::bit_cast<double>(kSlotEmpty)));
  const std::vector<double> armed(static_cast<size_t>(l.n), std::bit_cast<double>(kSlotEmpty));
  m_xg_tw.upload(armed);
  m_xg2_tw.upload(armed);
  m_stats_tw.upload(std::vector<LdltStats>(2, LdltStats{0, 0, 0, 0, 0x7ff0000000000000ull}));
  SLPX_HIP_CHECK(hipDeviceSynchronize());  // (the memsets ran on the null stream)
  return true;
}

int DeviceLdlt::riding_twin_workgroups_per_cu() {
  // the riding workgroups' LDS (ipm_error_block) beside the tasks': the launch takes the larger of the two
  const size_t lds = std::max<size_t>(m_mf_lds, sizeof(double) * kIpmErrLdsDoubles);
  return m_mode.twin_threads == 1024 ? workgroups_per_cu(reinterpret_cast<const void*>(&ldlt_mf_twin_kernel<1024, true>), 1024, lds)
                                     : workgroups_per_cu(reinterpret_cast<const void*>(&ldlt_mf_twin_kernel<512, true>), 512, lds);
}

MfDev DeviceLdlt::mf_dev() const {
  MfDev md;
  md.tasks = m_mf_tasks.p;
  md.fronts = m_mf_fronts.p;
  md.image = m_mf_image.p;
  md.image_stride16 = m_mf_image_stride16;
  md.image_desc = m_mf_image_desc.p;
  md.n_tasks = static_cast<unsigned int>(m_l.tasks.size());
  return md;
}

// One launch of the multifrontal step kernel (twin_mode != 0: two attempts, ldlt_mf_twin_kernel) with the buffer
// roles and parities of this moment; book_mf_step() is what the launch changes on the host.
unsigned int DeviceLdlt::launch_mf_step(int twin_mode, const double* reg, const LdltStepRiders& r) {
  const LdltPlan& l = m_l;
  m_solution_valid = true;
  const int parity = m_stats_cur ^ 1;
  LdltStats* cur = m_stats.p + static_cast<size_t>(parity);
  LdltStats* next = m_stats.p + static_cast<size_t>(parity ^ 1);
  const KktFuse& f = r.kkt;
  BacksubFuse bf = r.backsub;
  bf.stats_src = cur;
  bf.stats_host = m_h_stats;
  MfDev md = mf_dev();
  md.exit_cnt = m_exit_cnt.p;
  // a chained step (DeviceNlp::sweep_full_for_step): the kernel variant that waits for its sweep itself and whose last
  // workgroup tells the next step's sweep; the main stream stays "untouched" by a step's own launches
  const bool chained = r.chain != nullptr;
  md.chain = r.chain;
  md.wait_step = r.wait_step;
  md.this_step = r.this_step;
  md.delta = reg[0];  // (by value: MfDev)
  md.gamma = reg[1];
  md.gate = r.gate;  // (one launch: the step enqueued before the iteration in front of it was decided)
  const double* const reg_by_value = nullptr;
  if (twin_mode != 0) {
    const int tw_parity = m_stats_tw_cur ^ 1;
    MfTwin tw;
    tw.first_end = md.n_tasks + static_cast<unsigned int>(f.n_blocks);
    tw.delta = reg[2];
    tw.gamma = reg[3];
    tw.Lx = m_Lx_tw.p;
    tw.D = m_D_tw.p;
    tw.contrib = m_mf_contrib_tw.p;
    tw.zv = m_zv_tw.p;
    tw.xg = m_xg_tw_parity ? m_xg2_tw.p : m_xg_tw.p;
    tw.xg_next = m_xg_tw_parity ? m_xg_tw.p : m_xg2_tw.p;
    tw.out = m_p_tw.p;
    tw.ps = r.ps2;
    tw.pz = r.pz2;
    tw.stats = m_stats_tw.p + static_cast<size_t>(tw_parity);
    tw.stats_next = m_stats_tw.p + static_cast<size_t>(tw_parity ^ 1);
    tw.lhs = r.lhs2;
    tw.rhs = r.rhs2;
    MfRide ride;
    size_t lds = m_mf_lds;
    if (r.ride != nullptr) {
      // the error launch of the iteration before this step (DeviceNlp::ipm_ride_errors_in_next_step): its workgroups in
      // front of the tasks
      ride = *r.ride;
      md.ride_verdict = ride.fin.ride_verdict;
      md.ride_ticket = ride.fin.ride_ticket;
      lds = std::max<size_t>(lds, sizeof(double) * kIpmErrLdsDoubles);
    }
    const dim3 grid(2u * md.n_tasks + static_cast<uint32_t>(f.n_blocks) + ride.n_blocks);
    md.n_workgroups = grid.x;
    auto launch = [&](auto kernel, int threads) {
      hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, m_stream.raw(), m_ldev, md, r.lhs, r.rhs, reg_by_value, m_Lx.p, m_D.p, l.n,
                         m_mf_contrib.p, cur, next, m_zv.p, f, xg_now(), xg_other(), m_p.p, bf, tw, ride);
    };
    if (ride.n_blocks != 0) {
      if (m_mode.twin_threads == 1024) launch(&ldlt_mf_twin_kernel<1024, true>, 1024);
      else launch(&ldlt_mf_twin_kernel<512, true>, 512);
    } else {
      if (m_mode.twin_threads == 1024) launch(&ldlt_mf_twin_kernel<1024, false>, 1024);
      else launch(&ldlt_mf_twin_kernel<512, false>, 512);
    }
  } else {
    const dim3 grid(static_cast<uint32_t>(l.tasks.size()) + static_cast<uint32_t>(f.n_blocks));
    md.n_workgroups = grid.x;
    auto launch = [&](auto kernel, int threads) {
      hipLaunchKernelGGL(kernel, grid, dim3(threads), m_mf_lds, m_stream.raw(), m_ldev, md, r.lhs, r.rhs, reg_by_value, m_Lx.p, m_D.p,
                         l.n, m_mf_contrib.p, cur, next, m_zv.p, f, xg_now(), xg_other(), m_p.p, bf);
    };
    if (m_mode.mf_threads == 1024) {
      if (chained) m_mode.mf_mfma ? launch(&ldlt_mf_step_kernel<1024, true, true>, 1024) : launch(&ldlt_mf_step_kernel<1024, false, true>, 1024);
      else m_mode.mf_mfma ? launch(&ldlt_mf_step_kernel<1024, true, false>, 1024) : launch(&ldlt_mf_step_kernel<1024, false, false>, 1024);
    } else {
      if (chained) m_mode.mf_mfma ? launch(&ldlt_mf_step_kernel<512, true, true>, 512) : launch(&ldlt_mf_step_kernel<512, false, true>, 512);
      else m_mode.mf_mfma ? launch(&ldlt_mf_step_kernel<512, true, false>, 512) : launch(&ldlt_mf_step_kernel<512, false, false>, 512);
    }
  }
  SLPX_HIP_CHECK(hipGetLastError());
  return md.n_workgroups;
}

void DeviceLdlt::book_mf_step(int twin_mode) {
  m_stats_cur ^= 1;
  if (twin_mode != 0) {
    m_stats_tw_cur ^= 1;
    m_xg_tw_parity ^= 1;
  }
  xg_flip();
  m_twin_mode = twin_mode;
}

unsigned int DeviceLdlt::step(const std::vector<double>& delta, const std::vector<double>& gamma, const std::vector<uint8_t>& active,
                              const LdltStepRiders& r) {
  if (!step_possible()) throw std::logic_error("slpx: a one-launch step without the multifrontal plan");
  write_reg(delta, gamma, active);
  const unsigned int workgroups = launch_mf_step(0, m_h_reg, r);
  book_mf_step(0);
  return workgroups;
}

void DeviceLdlt::step_twin(double delta0, double gamma0, double delta1, double gamma1, int mode, const LdltStepRiders& r) {
  m_h_reg[0] = delta0;
  m_h_reg[1] = gamma0;
  m_h_reg[2] = delta1;
  m_h_reg[3] = gamma1;
  note_factored(0, delta0, gamma0);
  m_fact_tw[0] = delta1;
  m_fact_tw[1] = gamma1;
  launch_mf_step(mode, m_h_reg, r);
  book_mf_step(mode);
}

void DeviceLdlt::adopt_twin() {
  // every launch takes these pointers when it is made (ipm_accept_lookahead): later solves with this factorization,
  // the committed direction and the counters are the second attempt's
  m_Lx.swap(m_Lx_tw);
  m_D.swap(m_D_tw);
  m_zv.swap(m_zv_tw);
  m_p.swap(m_p_tw);
  m_stats.swap(m_stats_tw);
  std::swap(m_stats_cur, m_stats_tw_cur);
  m_h_stats[0] = m_h_stats[1];
  m_twin_mode = 0;
  note_factored(0, m_fact_tw[0], m_fact_tw[1]);
}

void DeviceLdlt::read_stats(std::vector<LdltStats>& out) {
  out.resize(m_batch);
  if (!m_stats_in_host)
    SLPX_HIP_CHECK(hipMemcpyAsync(m_h_stats, m_stats.p + static_cast<size_t>(m_stats_cur) * m_batch,
                                  m_batch * sizeof(LdltStats), hipMemcpyDeviceToHost, m_stream));
  // Busy-poll instead of a blocking wait: the interrupt-driven wake-up of
  // hipStreamSynchronize costs tens of microseconds, a tenth of a whole Newton step.
  if (m_stats_in_host && m_batch == 1) {
    // the publishing kernel's sequence number (see step_backsub_kernel); the stream is
    // consulted now and then so that a failed launch cannot hang the host
    spin_on_published([&] { return *m_h_seq >= m_stats_seq; }, m_stream.raw(), "slpx: step finished without publishing its counters");
  } else {
    hipError_t st;
    while ((st = hipStreamQuery(m_stream.raw())) == hipErrorNotReady) {
    }
    SLPX_HIP_CHECK(st);
  }
  std::copy(m_h_stats, m_h_stats + m_batch, out.begin());
  // (an experiment's knob: the host sits on the verdict for so many nanoseconds — how much of its reaction a step
  // hides: profiles/host_slack.sh)
  static const long delay_ns = [] {
    const char* env = std::getenv("SLPX_DEBUG_STATS_DELAY_NS");
    return env ? std::atol(env) : 0L;
  }();
  if (delay_ns > 0) {
    const auto until = std::chrono::steady_clock::now() + std::chrono::nanoseconds(delay_ns);
    while (std::chrono::steady_clock::now() < until) {
    }
  }
}

// Full solve for a right-hand side that arrived AFTER the factorization (second-order
// corrections, multiplier estimate, slpx_ldlt_solve): forward, then backward.
void DeviceLdlt::solve(const LdltSystem& sys) {
  m_solution_valid = true;
  const LdltPlan& l = m_l;
  if (m_mode.dense) {
    solve_after_factor(sys);
    return;
  }
  if (m_mode.mf && m_mode.mf_solve && m_batch == 1 && xg_other() != nullptr) {
    const MfDev md = mf_dev();
    const dim3 grid(static_cast<uint32_t>(l.tasks.size()));
    if (m_mode.mf_threads == 1024)
      hipLaunchKernelGGL(ldlt_mf_solve_kernel<1024>, grid, dim3(1024), m_mf_lds, m_stream, m_ldev, md, m_Lx.p, m_D.p, sys.rhs,
                         m_mf_contrib.p, xg_now(), xg_other(), m_p.p);
    else
      hipLaunchKernelGGL(ldlt_mf_solve_kernel<512>, grid, dim3(512), m_mf_lds, m_stream, m_ldev, md, m_Lx.p, m_D.p, sys.rhs,
                         m_mf_contrib.p, xg_now(), xg_other(), m_p.p);
    xg_flip();
    SLPX_HIP_CHECK(hipGetLastError());
    return;
  }
  const long long lxs = static_cast<long long>(std::max<int64_t>(1, l.nnzL));
  const int scs = static_cast<int>(std::max<uint32_t>(1, l.n_scontrib));
  if (m_mode.il) {
    const int C = (m_batch + 63) / 64;
    if (!sys.rhs_in_il) to_interleaved(sys.rhs, l.n, sys.rhs_il, m_stream);
    for (int r = 0; r < l.n_rounds; ++r) {
      const uint32_t nt = l.round_ptr[r + 1] - l.round_ptr[r];
      hipLaunchKernelGGL(ldlt_fwd_il_kernel, dim3(nt, C), dim3(kIlLanes), m_il_solve_lds, m_stream, m_ldev,
                         l.round_ptr[r], sys.rhs_il, l.n, m_Lx_il.p, lxs, m_D_il.p, m_scontrib_il.p, scs,
                         m_zv_il.p);
    }
    solve_after_factor(sys);
    return;
  }
  if (m_mode.single_launch && m_batch == 1) {
    // one problem: every round in ONE launch (the tasks order themselves through the round counters)
    hipLaunchKernelGGL(ldlt_fwd_kernel, dim3(static_cast<uint32_t>(l.tasks.size()), 1), dim3(256), l.solve_lds_bytes, m_stream,
                       m_ldev, 0u, sys.rhs, l.n, m_Lx.p, lxs, m_D.p, m_scontrib.p, scs, m_zv.p, m_fround_cnt.p);
  } else {
    for (int r = 0; r < l.n_rounds; ++r) {
      const uint32_t nt = l.round_ptr[r + 1] - l.round_ptr[r];
      hipLaunchKernelGGL(ldlt_fwd_kernel, dim3(nt, m_batch), dim3(256), l.solve_lds_bytes, m_stream,
                         m_ldev, l.round_ptr[r], sys.rhs, l.n, m_Lx.p, lxs, m_D.p, m_scontrib.p, scs,
                         m_zv.p, static_cast<unsigned int*>(nullptr));
    }
  }
  solve_after_factor(sys);
}

// The factorization carried the rhs along as an extra row and left z = D⁻¹L⁻¹Pb behind
// (ldlt_symbolic.cpp), so only the backward substitution remains; with `riding`, the back-substitution and
// the hand-over of the current attempt's counters to the host in the same launch (device_base.hpp: BacksubFuse).
void DeviceLdlt::solve_after_factor(const LdltSystem& sys, const BacksubFuse* riding) {
  const LdltPlan& l = m_l;
  m_solution_valid = true;
  const long long lxs = static_cast<long long>(std::max<int64_t>(1, l.nnzL));
  if (m_mode.dense) {  // (nothing rides in a dense factorization: forward and backward substitution from the rhs in memory)
    hipLaunchKernelGGL(ldlt_dense_solve_kernel, dim3(m_batch), dim3(kDenseThreads), 8u * static_cast<uint32_t>(l.n) + 16u, m_stream, l.n,
                       m_dense_A.p, sys.rhs, m_p.p, m_mode.dense_pivoted ? m_dense_trans.p : nullptr);
    SLPX_HIP_CHECK(hipGetLastError());
    return;
  }
  if (m_mode.il) {
    const int C = (m_batch + 63) / 64;
    for (int r = l.n_rounds - 1; r >= 0; --r) {
      const uint32_t nt = l.round_ptr[r + 1] - l.round_ptr[r];
      hipLaunchKernelGGL(ldlt_bwd_il_kernel, dim3(nt, C), dim3(kIlLanes * kIlBwdWaves), m_il_solve_lds, m_stream, m_ldev,
                         l.round_ptr[r], l.n, m_Lx_il.p, lxs, m_zv_il.p, m_xg_il.p, m_p.p, m_batch);
    }
    SLPX_HIP_CHECK(hipGetLastError());
    return;
  }
  if (m_mode.single_launch) {
    const uint32_t nt = static_cast<uint32_t>(l.tasks.size());
    BacksubFuse f;
    if (riding != nullptr) {
      f = *riding;
      f.stats_src = stats_now();
      f.stats_host = m_h_stats;
    }
    hipLaunchKernelGGL(ldlt_bwd_kernel, dim3(nt, m_batch), dim3(256), f.on ? m_solve_lds_inline : l.solve_lds_bytes,
                       m_stream, m_ldev, nt - 1, l.n, m_Lx.p, lxs, m_zv.p, xg_now(), xg_other(), m_p.p, m_bround_cnt.p, f);
    xg_flip();
  } else {
    for (int r = l.n_rounds - 1; r >= 0; --r) {
      const uint32_t nt = l.round_ptr[r + 1] - l.round_ptr[r];
      hipLaunchKernelGGL(ldlt_bwd_kernel, dim3(nt, m_batch), dim3(256), l.solve_lds_bytes, m_stream,
                         m_ldev, l.round_ptr[r], l.n, m_Lx.p, lxs, m_zv.p, m_xg.p, static_cast<double*>(nullptr), m_p.p,
                         static_cast<unsigned int*>(nullptr), BacksubFuse{});
    }
  }
  SLPX_HIP_CHECK(hipGetLastError());
}

// Batch-interleaved mode keeps L and D as [chunk][index][lane]; the batch-major copies that
// slpx_system_get hands out are made on demand.
void DeviceLdlt::materialize_factor() {
  if (!m_mode.il || !m_il_outputs_stale) return;
  const LdltPlan& l = m_l;
  to_batch_major(m_Lx_il.p, static_cast<int>(std::max<int64_t>(1, l.nnzL)), m_Lx.p);
  to_batch_major(m_D_il.p, l.n, m_D.p);
  SLPX_HIP_CHECK(hipGetLastError());
  m_il_outputs_stale = false;
}

size_t DeviceLdlt::download_factor_scratch(int which, std::vector<double>& out) {
  const LdltPlan& l = m_l;
  const size_t B = static_cast<size_t>(m_batch);
  const size_t count = which == 0 ? static_cast<size_t>(l.n) : std::max<uint32_t>(1, l.n_contrib);
  out.assign(B * count, 0.0);
  if (!m_mode.il) {
    download(which == 0 ? m_zv.p : m_contrib.p, out.data(), B * count);
    return count;
  }
  // [group of kIlW problems][index][problem of the group] -> [problem][index]
  const DevBuf<double>& src = which == 0 ? m_zv_il : m_contrib_il;
  std::vector<double> raw(src.n);
  download(src.p, raw.data(), raw.size());
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < count; ++i) out[b * count + i] = raw[((b / kIlW) * count + i) * kIlW + b % kIlW];
  return count;
}

}  // namespace slpx
