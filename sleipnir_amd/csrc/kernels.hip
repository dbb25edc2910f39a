// DeviceNlp's host code: the device-side state of one compiled NLP, the launches of the KKT system's kernels around
// the factorization and of the interior-point iteration.  See DESIGN.md §3 for the roofline of each kernel.
//
//   kkt_assemble   lhs values by gather   (interior_point.hpp:426-440)      kkt_launch_kernels.h
//   kkt_rhs        rhs by column gathers  (interior_point.hpp:444-448)
//   step_backsub   pˢ, pᶻ                 (interior_point.hpp:479-480)
//   ipm_*          the iteration's scalars and iterates                     ipm_launch_kernels.h
// The tape sweeps: DeviceTape, device_tape.hip.  The chained-step protocol: StepChain, step_chain.hpp.  The
// factorization and the solves between them: DeviceLdlt, device_ldlt.hip.
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
#include "ipm_decide.h"
#include "ipm_launch_kernels.h"
#include "kkt_launch_kernels.h"
#include "setup_timing.hpp"

namespace slpx {

// ============================================================================
// DeviceNlp
// ============================================================================

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
    : m_s_ref(s), m_k_ref(k), m_l_ref(l), m_batch(batch), m_device(device), m_sw(sw), m_tape(s, batch, m_stream),
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
  m_tape.upload(m_mode.chain_mode);
  lap("  upload: tapes (+ code objects)");
  m_tape.raise_lds_limits();
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
  m_tape.alloc_scratch();
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
}

void DeviceNlp::set_scaling(const std::vector<double>& scales) {
  const NlpStructure& s = m_s_ref;
  if (static_cast<int>(scales.size()) != s.n_scales())
    throw std::runtime_error("set_scaling: wrong length");
  m_tape.set_scaling(scales);
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

void DeviceNlp::sweep_full(bool with_reduce) {
  const hipStream_t stream = m_stream;
  m_tape.launch(DeviceTape::Full, true, {m_in.p, m_V.p, with_reduce, stream, {}});
}
void DeviceNlp::sweep_full_for_step() {
  // the tape's side of a chained step, and the step is the one-launch multifrontal kernel
  if (!m_mode.chain_on || !m_tape.full_sweep_can_chain() || m_batch != 1 || !m_ldlt.step_possible() || !m_mode.fuse_solve) {
    sweep_full(/*with_reduce=*/false);
    return;
  }
  const StepChain::Route route = m_chain.begin_sweep(m_stream.raw(), m_mode);
  if (route.kind == StepChain::Route::NotChained) {
    sweep_full(/*with_reduce=*/false);
    return;
  }
  const bool chained = route.kind == StepChain::Route::Chained;
  const hipStream_t stream = chained ? m_chain.tape_stream() : m_stream.raw();
  const DeviceTape::Link link = chained ? DeviceTape::Link::chain(route.words, route.wait_step, route.this_step) : DeviceTape::Link{};
  const unsigned int workgroups = m_tape.launch(DeviceTape::Full, true, {m_in.p, m_V.p, false, stream, link});
  if (chained) m_chain.sweep_launched(workgroups);
}
// A chained step reported kLdltChainFailure: one of the two kernels gave up waiting for the other (never
// expected — a shared / preempted / serialized GPU).  Drain both streams, clear the words, keep this
// system's steps unchained from now on and leave V as a fresh sweep of the current state writes it.
void DeviceNlp::recover_from_chain_failure() {
  m_chain.recover(m_stream.raw());
  unchain(m_mode);
  if (std::getenv("SLPX_LDLT_VERBOSE")) std::fprintf(stderr, "slpx: a chained step lost its hand-over: the step is redone, steps are unchained from here on\n");
  sweep_full(/*with_reduce=*/false);
}
void DeviceNlp::sweep_values() {
  const hipStream_t stream = m_stream;
  m_tape.launch(DeviceTape::Values, false, {m_in.p, m_V.p, true, stream, {}});
}
// (no reductions: ipm_trial_metrics_kernel, the only reader of these values, finishes the sums)
void DeviceNlp::sweep_values_trial() {
  const hipStream_t stream = m_stream;
  m_tape.launch(DeviceTape::Values, false, {m_trial_in.p, m_V_trial.p, false, stream, {}});
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
void DeviceNlp::build_kkt(bool with_reduce, bool defer) {
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
    if (with_reduce && m_tape.n_reduces()) m_tape.reduce(m_V.p, m_stream);
    SLPX_HIP_CHECK(hipGetLastError());
    return;
  }
  if (defer) {  // evaluated inside the factorization's launch (take_kkt_fuse)
    m_kkt_pending = with_reduce ? 2 : 1;
    m_lhs_stale = m_rhs_stale = true;
    return;
  }
  m_lhs_stale = m_rhs_stale = false;
  m_lhs_in_il = m_rhs_in_il = false;
  const int na = grid_for((m_kdev.nnz_lhs + 3) / 4, 256), nr = grid_for(m_kdev.dim, 256);
  const int nred = with_reduce ? static_cast<int>(m_tape.n_reduces()) : 0;
  hipLaunchKernelGGL(kkt_build_kernel, dim3(na + nr + nred, m_batch), dim3(256), 0, m_stream, m_kdev, m_V.p,
                     m_s_ref.nV, m_s.p, m_y.p, m_z.p, m_mu.p, m_lhs.p, m_rhs.p, na, nr, m_tape.reduces_dev(), m_tape.scales_dev());
  SLPX_HIP_CHECK(hipGetLastError());
}

// build_kkt() when a factorization attempt is the next thing enqueued (a Newton step): the
// assembly then rides in that launch (device.hpp: KktFuse)
void DeviceNlp::build_kkt(bool with_reduce) { build_kkt(with_reduce, /*defer=*/false); }
void DeviceNlp::build_kkt_for_step(bool with_reduce) {
  build_kkt(with_reduce, /*defer=*/m_mode.fuse_kkt);
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
    f.n_blocks = kkt_mode == 2 ? static_cast<int>(m_tape.n_reduces()) : 0;
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
    f.red = m_tape.reduces_dev();
    f.scales = m_tape.scales_dev();
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
LdltStepRiders DeviceNlp::step_riders(const KktFuse& f) {
  LdltStepRiders r;
  r.kkt = f;
  r.backsub = backsub_fuse();
  r.lhs = m_lhs.p;
  r.rhs = m_rhs.p;
  const ChainLedger::StepLink link = m_chain.step_link();
  if (link.chained) {
    r.chain = m_chain.words();
    r.wait_step = link.wait_step;  // (every workgroup of the chained sweeps so far, this step's included)
  }
  r.this_step = link.this_step;
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
  m_chain.step_launched(m_ldlt.step(delta, gamma, active, step_riders(f)));  // (its workgroups: what the next chained sweep waits for)
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
  LdltStepRiders r = step_riders(f);  // (never chained: no twin is launched over a pending sweep)
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
  m_chain.twin_launched();
  m_ldlt.stats_handed_to_host(++m_seq_expected);
}

bool DeviceNlp::factor_solve_publish_twin(double delta0, double gamma0, double delta1, double gamma1, int mode) {
  if (!twin_ready() || m_chain.sweep_pending()) return false;
  if (!m_kkt_pending) materialize_kkt();
  launch_twin(delta0, gamma0, delta1, gamma1, mode, take_kkt_fuse(), nullptr, nullptr);
  return true;
}

bool DeviceNlp::factor_solve_publish_twin_written(double delta0, double gamma0, double delta1, double gamma1, int mode, const double* lhs2,
                                                  const double* rhs2) {
  if (!twin_ready() || m_chain.sweep_pending() || m_kkt_pending || m_lhs_stale || m_rhs_stale) return false;
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
  // with_reduce false: the separable sums ride in ipm_errors(.., sums_ride, ahead)
  // (the generated kernel leaves at once when the look-ahead launch flagged the attempt as rejected)
  DeviceTape::Link link;
  if (skippable && m_tape.full_has_generated_kernel() && m_ipm_alpha.p != nullptr)
    link = DeviceTape::Link::skip_if(reinterpret_cast<unsigned int*>(m_ipm_alpha.p + 2));
  const hipStream_t stream = m_stream;
  m_tape.launch(DeviceTape::Full, true, {m_trial_in.p, m_V_trial.p, with_reduce, stream, link});
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
                     m_tape.reduces_dev(), static_cast<int>(m_tape.n_reduces()), m_tape.scales_dev());
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
  const int n_sums = sums_ride ? static_cast<int>(m_tape.n_reduces()) : 0;
  IpmErrFinish fin;
  fin.n_err_blocks = blocks;
  fin.n_total_blocks = blocks + n_sums;
  fin.red = m_tape.reduces_dev();
  fin.tape_scales = m_tape.scales_dev();
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
    choose_ride(m_mode, m_plan, m_tape.n_reduces(), static_cast<size_t>(per_cu) * m_cus, m_sw);
    if (m_sw.ipm_ride && std::getenv("SLPX_LDLT_VERBOSE"))
      std::fprintf(stderr, "ldlt riding error launch: %zu workgroups, %d of %d threads per CU x %d CUs%s\n", riding_workgroups(m_plan, m_tape.n_reduces()),
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
  const int n_sums = static_cast<int>(m_tape.n_reduces());
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
  fin.red = m_tape.reduces_dev();
  fin.tape_scales = m_tape.scales_dev();
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
