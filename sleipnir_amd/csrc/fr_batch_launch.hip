// Launch wrappers of BatchFrDevice (fr_batch.hpp; kernels: fr_batch_kernels.h).
#include <algorithm>

#include "fr_batch.hpp"

#include "fr_batch_kernels.h"

namespace slpx {

namespace {
int chunks(int work) { return std::max(1, (work + kFrBatchThreads - 1) / kFrBatchThreads); }
size_t at_least_1(size_t k) { return k ? k : 1; }
}  // namespace

BatchFrDevice::BatchFrDevice(NewtonSystem& sys_) : BatchDevice(sys_) {
  const KktPlan& k = sys.kkt();
  M = 2 * m_e + 2 * m_i;
  nnz = k.lhs.nnz();
  std::vector<int32_t> diag_of(at_least_1(static_cast<size_t>(nnz)), -1);
  for (int c = 0; c < k.dim; ++c)
    for (int p = k.lhs.colptr[c]; p < k.lhs.colptr[c + 1]; ++p)
      if (k.lhs.rowidx[p] == c) diag_of[p] = c;
  m_diag_of.upload(diag_of);
  for (auto* v : {&delta, &mu, &tau, &alpha_z, &mu_outer}) v->assign(B, 0.0);
  soc.assign(B, 0);
  rhs_only.assign(B, 0);
  for (auto* b : {&m_delta, &m_mu, &m_tau, &m_alpha_z, &m_mu_outer}) b->alloc(B);
  for (auto* b : {&m_soc, &m_rhs_only}) b->alloc(B);
  const size_t Bn = at_least_1(static_cast<size_t>(B) * n), Be = at_least_1(static_cast<size_t>(B) * m_e),
               Bi = at_least_1(static_cast<size_t>(B) * m_i), BM = at_least_1(static_cast<size_t>(B) * M),
               Bd = at_least_1(static_cast<size_t>(B) * dim);
  for (auto* b : {&m_xr, &m_w, &m_g_outer}) b->alloc(Bn);
  for (auto* b : {&m_s0, &m_z0, &m_s_outer, &m_ps0, &m_pz0, &m_soc_c0, &m_keep_ps0, &m_keep_pz0}) b->alloc(Bi);
  m_soc_ce.alloc(Be);
  for (auto* b : {&m_pn, &m_sxx, &m_zx, &m_dpn, &m_psx, &m_pzx, &m_soc_x, &m_keep_dpn, &m_keep_psx, &m_keep_pzx}) b->alloc(BM);
  for (auto* b : {&m_p, &m_keep_p}) b->alloc(Bd);
  m_fr_out.alloc(static_cast<size_t>(B) * kFrBatchErrN);
  m_vt.alloc(static_cast<size_t>(B) * sys.structure().off_g);
  // (an instance that never entered a phase is never active; its slices are defined all the same)
  for (auto* b : {&m_xr, &m_w, &m_g_outer, &m_s0, &m_z0, &m_s_outer, &m_ps0, &m_pz0, &m_soc_c0, &m_keep_ps0, &m_keep_pz0, &m_soc_ce, &m_pn,
                  &m_sxx, &m_zx, &m_dpn, &m_psx, &m_pzx, &m_soc_x, &m_keep_dpn, &m_keep_psx, &m_keep_pzx, &m_p, &m_keep_p, &m_fr_out, &m_vt, &m_x, &m_y,
                  &m_Vcur})
    b->zero(sys.device().stream());
  m_cur = BatchIter{m_x.p, m_s0.p, m_y.p, m_z0.p};
  m_trial = m_cur;
  m_mu_of_errors = m_mu.p;
  SLPX_HIP_CHECK(hipStreamSynchronize(sys.device().stream()));
}

void BatchFrDevice::upload() {
  put_async(m_delta, delta);
  put_async(m_mu, mu);
  put_async(m_tau, tau);
  put_async(m_alpha_z, alpha_z);
  put_async(m_mu_outer, mu_outer);
  put_async(m_soc, soc);
  put_async(m_rhs_only, rhs_only);
  BatchDevice::upload();
}

void BatchFrDevice::begin(int b, const double* x, const double* s0, const double* y, const double* z0, const double* x_r, const double* w,
                          const double* g_outer, const double* s_outer, const double* pn, const double* sx, const double* zx) {
  if (b < 0 || b >= B) throw std::runtime_error("BatchFrDevice::begin: no such instance");
  hipStream_t st = sys.device().stream();
  const size_t sb = static_cast<size_t>(b);
  auto up = [&](DevBuf<double>& buf, const double* src, int count) {
    if (count > 0)
      SLPX_HIP_CHECK(hipMemcpyAsync(buf.p + sb * count, src, static_cast<size_t>(count) * sizeof(double), hipMemcpyHostToDevice, st));
  };
  up(m_x, x, n);
  up(m_s0, s0, m_i);
  up(m_y, y, m_e);
  up(m_z0, z0, m_i);
  up(m_xr, x_r, n);
  up(m_w, w, n);
  up(m_g_outer, g_outer, n);
  up(m_s_outer, s_outer, m_i);
  up(m_pn, pn, M);
  up(m_sxx, sx, M);
  up(m_zx, zx, M);
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (the host vectors may go away)
}

void BatchFrDevice::download_instance(int b, double* x, double* s0, double* y, double* z0, double* pn, double* sx, double* zx) {
  if (b < 0 || b >= B) throw std::runtime_error("BatchFrDevice::download_instance: no such instance");
  DeviceNlp& dev = sys.device();
  const size_t sb = static_cast<size_t>(b);
  auto down = [&](const DevBuf<double>& buf, double* dst, int count) {
    if (count > 0) dev.download(buf.p + sb * count, dst, count);
  };
  down(m_x, x, n);
  down(m_s0, s0, m_i);
  down(m_y, y, m_e);
  down(m_z0, z0, m_i);
  down(m_pn, pn, M);
  down(m_sxx, sx, M);
  down(m_zx, zx, M);
}

void BatchFrDevice::download_direction(int b, double* p, double* ps0, double* pz0, double* dpn, double* psx, double* pzx) {
  if (b < 0 || b >= B) throw std::runtime_error("BatchFrDevice::download_direction: no such instance");
  DeviceNlp& dev = sys.device();
  const size_t sb = static_cast<size_t>(b);
  auto down = [&](const DevBuf<double>& buf, double* dst, int count) {
    if (count > 0) dev.download(buf.p + sb * count, dst, count);
  };
  down(m_p, p, dim);
  down(m_ps0, ps0, m_i);
  down(m_pz0, pz0, m_i);
  down(m_dpn, dpn, M);
  down(m_psx, psx, M);
  down(m_pzx, pzx, M);
}

void BatchFrDevice::download_V(int b, double* V) {
  if (b < 0 || b >= B) throw std::runtime_error("BatchFrDevice::download_V: no such instance");
  sys.device().download(m_Vcur.p + static_cast<size_t>(b) * nV, V, nV);
}

void BatchFrDevice::fill(FrBatchArgs& G) {
  DeviceNlp& dev = sys.device();
  const NlpStructure& s = sys.structure();
  FrDevice::Args& a = G.A;
  a = FrDevice::Args{};
  a.n = n;
  a.m_e = m_e;
  a.m_i = m_i;
  a.off_Hf = s.off_Hf;
  a.off_Hc = s.off_Hc;
  a.rho = kFrRho;
  a.K = dev.kdev();
  a.V = m_Vcur.p;
  a.Vt = dev.d_V();
  a.in = m_x.p;
  a.trial_in = dev.d_x();
  a.s0 = m_s0.p;
  a.y = m_y.p;
  a.z0 = m_z0.p;
  a.p = m_p.p;
  a.ps0 = m_ps0.p;
  a.pz0 = m_pz0.p;
  a.xr = m_xr.p;
  a.w = m_w.p;
  a.g_outer = m_g_outer.p;
  a.s_outer = m_s_outer.p;
  a.scales = m_scales.p;
  a.pn = m_pn.p;
  a.sx = m_sxx.p;
  a.zx = m_zx.p;
  a.dpn = m_dpn.p;
  a.psx = m_psx.p;
  a.pzx = m_pzx.p;
  a.soc_ce = m_soc_ce.p;
  a.soc_c0 = m_soc_c0.p;
  a.soc_x = m_soc_x.p;
  G.nV = nV;
  G.nin = s.n_inputs();
  G.diag_of = m_diag_of.p;
  G.delta = m_delta.p;
  G.mu = m_mu.p;
  G.tau = m_tau.p;
  G.alpha = m_alpha.p;
  G.alpha_soc = m_alpha_soc.p;
  G.alpha_z = m_alpha_z.p;
  G.mu_outer = m_mu_outer.p;
  G.soc = m_soc.p;
  G.first = m_first.p;
  G.rhs_only = m_rhs_only.p;
  G.active = m_active.p;
  G.lhs = dev.lhs_raw();
  G.rhs = dev.rhs_raw();
  G.p_sys = dev.ldlt().d_p();
  G.keep_p = m_keep_p.p;
  G.keep_ps0 = m_keep_ps0.p;
  G.keep_pz0 = m_keep_pz0.p;
  G.keep_dpn = m_keep_dpn.p;
  G.keep_psx = m_keep_psx.p;
  G.keep_pzx = m_keep_pzx.p;
  G.vt_keep = m_vt.p;
  G.nhead = s.off_g;
  G.out = m_fr_out.p;
}

void BatchFrDevice::download_fr_out(size_t per_instance, std::vector<double>& out) {
  // (every kernel leaves instance b's scalars at out[b * kFrBatchErrN]: a skipped instance's are nobody else's)
  std::vector<double> all(static_cast<size_t>(B) * kFrBatchErrN);
  sys.device().download(m_fr_out.p, all.data(), all.size());
  out.resize(static_cast<size_t>(B) * per_instance);
  for (int b = 0; b < B; ++b)
    std::copy_n(all.begin() + static_cast<size_t>(b) * kFrBatchErrN, per_instance, out.begin() + static_cast<size_t>(b) * per_instance);
}

void BatchFrDevice::sweep() {
  DeviceNlp& dev = sys.device();
  sweep_iterate(/*with_state=*/false);
  hipLaunchKernelGGL(fr_batch_keep_V_kernel, dim3(chunks(nV), B), dim3(kFrBatchThreads), 0, dev.stream(), dev.d_V(), m_Vcur.p, nV, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void BatchFrDevice::build() {
  DeviceNlp& dev = sys.device();
  FrBatchArgs G;
  fill(G);
  const int work = std::max({nnz, dim, 1});
  hipLaunchKernelGGL(fr_batch_build_kernel, dim3(std::min(chunks(work), 2048), B), dim3(kFrBatchThreads), 0, dev.stream(), G);
  SLPX_HIP_CHECK(hipGetLastError());
  const bool lhs_written = std::any_of(rhs_only.begin(), rhs_only.end(), [](uint8_t r) { return r == 0; });
  dev.system_written_by_caller(lhs_written, true);
}

void BatchFrDevice::expand(std::vector<double>& dir) {
  DeviceNlp& dev = sys.device();
  FrBatchArgs G;
  fill(G);
  hipLaunchKernelGGL(fr_batch_expand_kernel, dim3(B), dim3(kFrBatchThreads), 0, dev.stream(), G);
  SLPX_HIP_CHECK(hipGetLastError());
  download_fr_out(4, dir);
}

void BatchFrDevice::trial_values(std::vector<double>& met, bool after_expand) {
  DeviceNlp& dev = sys.device();
  FrBatchArgs G;
  fill(G);
  if (!after_expand) {
    hipLaunchKernelGGL(fr_batch_trial_point_kernel, dim3(B), dim3(kFrBatchThreads), 0, dev.stream(), G);
    SLPX_HIP_CHECK(hipGetLastError());
  }
  dev.sweep_values();
  scale_V(sys.structure().off_g);
  hipLaunchKernelGGL(fr_batch_trial_metrics_kernel, dim3(B), dim3(kFrBatchThreads), 0, dev.stream(), G);
  SLPX_HIP_CHECK(hipGetLastError());
  download_fr_out(4, met);
}

void BatchFrDevice::soc_accumulate() {
  DeviceNlp& dev = sys.device();
  FrBatchArgs G;
  fill(G);
  hipLaunchKernelGGL(fr_batch_soc_accumulate_kernel, dim3(B), dim3(kFrBatchThreads), 0, dev.stream(), G);
  SLPX_HIP_CHECK(hipGetLastError());
}

void BatchFrDevice::copy_direction(bool restore) {
  DeviceNlp& dev = sys.device();
  FrBatchArgs G;
  fill(G);
  hipLaunchKernelGGL(fr_batch_copy_direction_kernel, dim3(B), dim3(kFrBatchThreads), 0, dev.stream(), G, restore ? 1 : 0);
  SLPX_HIP_CHECK(hipGetLastError());
}
void BatchFrDevice::save_direction() { copy_direction(false); }
void BatchFrDevice::restore_direction() { copy_direction(true); }

void BatchFrDevice::commit() {
  DeviceNlp& dev = sys.device();
  FrBatchArgs G;
  fill(G);
  hipLaunchKernelGGL(fr_batch_commit_kernel, dim3(B), dim3(kFrBatchThreads), 0, dev.stream(), G);
  SLPX_HIP_CHECK(hipGetLastError());
}

void BatchFrDevice::errors(bool check_all_V, std::vector<double>& err) {
  DeviceNlp& dev = sys.device();
  FrBatchArgs G;
  fill(G);
  hipLaunchKernelGGL(fr_batch_errors_kernel, dim3(B), dim3(kFrBatchThreads), 0, dev.stream(), G, check_all_V ? 1 : 0);
  SLPX_HIP_CHECK(hipGetLastError());
  download_fr_out(kFrBatchErrN, err);
}

}  // namespace slpx
