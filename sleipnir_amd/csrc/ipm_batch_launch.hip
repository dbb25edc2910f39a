// Launch wrappers of the batched drivers' kernels: BatchDevice, the state and the errors, scaling and input kernels
// every driver shares; BatchIpmDevice (ipm_batch_kernels.h); BatchEqDevice (eq_batch_kernels.h).
#include <algorithm>

#include "eq_batch.hpp"
#include "ipm_batch.hpp"

#include "eq_batch_kernels.h"
#include "ipm_batch_kernels.h"
#include "warm_start_batch_kernels.h"

namespace slpx {

namespace {
int chunks(int work) { return (work + kBatchThreads - 1) / kBatchThreads; }
size_t at_least_1(size_t k) { return k ? k : 1; }
}  // namespace

// ---- BatchDevice (batch_lockstep.hpp) ----

BatchDevice::BatchDevice(NewtonSystem& sys_) : sys(sys_) {
  const NlpStructure& s = sys.structure();
  B = sys.batch();
  n = s.n;
  m_e = s.m_e;
  m_i = s.m_i;
  dim = n + m_e;
  ns = s.n_scales();
  nV = s.nV;
  alpha.assign(B, 0.0);
  alpha_soc.assign(B, 0.0);
  mode.assign(B, 0);
  first.assign(B, 0);
  active.assign(B, 0);
  m_scale_idx.upload(s.V_scale_idx);
  m_is_static.upload(s.V_is_static);
  m_static_raw.upload(s.V_static_raw);
  m_scales.alloc(static_cast<size_t>(B) * ns);
  for (auto* b : {&m_active, &m_first}) b->alloc(B);
  m_mode.alloc(B);
  for (auto* b : {&m_alpha, &m_alpha_soc}) b->alloc(B);
  m_out.alloc(static_cast<size_t>(B) * kBatchErrN);
  const size_t Bn = at_least_1(static_cast<size_t>(B) * n), Be = at_least_1(static_cast<size_t>(B) * m_e);
  for (auto* b : {&m_x, &m_tx, &m_sx}) b->alloc(Bn);
  for (auto* b : {&m_y, &m_ty, &m_sy, &m_tce, &m_sce}) b->alloc(Be);
  m_Vcur.alloc(static_cast<size_t>(B) * nV);
}

void BatchDevice::upload() {
  put_async(m_active, active);
  put_async(m_alpha, alpha);
  put_async(m_alpha_soc, alpha_soc);
  put_async(m_mode, mode);
  put_async(m_first, first);
  // (pageable sources: the host may change its vectors once the copies are through)
  SLPX_HIP_CHECK(hipStreamSynchronize(sys.device().stream()));
}

void BatchDevice::set_scales(const std::vector<double>& scales) {
  if (scales.size() != m_scales.n) throw std::runtime_error("BatchDevice::set_scales: wrong length");
  SLPX_HIP_CHECK(hipMemcpy(m_scales.p, scales.data(), scales.size() * sizeof(double), hipMemcpyHostToDevice));
}

void BatchDevice::set_iterate(const std::vector<double>& x, const std::vector<double>& s, const std::vector<double>& y,
                              const std::vector<double>& z) {
  const size_t Bs = B;
  if (x.size() != Bs * n || s.size() != Bs * m_i || y.size() != Bs * m_e || z.size() != Bs * m_i)
    throw std::runtime_error("BatchDevice::set_iterate: wrong lengths");
  auto put = [](double* d, const std::vector<double>& h) {
    if (!h.empty()) SLPX_HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  };
  put(m_cur.x, x);
  put(m_cur.s, s);
  put(m_cur.y, y);
  put(m_cur.z, z);
}

void BatchDevice::get_iterate(std::vector<double>& x, std::vector<double>& s, std::vector<double>& y, std::vector<double>& z) {
  DeviceNlp& dev = sys.device();
  x.resize(static_cast<size_t>(B) * n);
  s.resize(static_cast<size_t>(B) * m_i);
  y.resize(static_cast<size_t>(B) * m_e);
  z.resize(static_cast<size_t>(B) * m_i);
  if (!x.empty()) dev.download(m_cur.x, x.data(), x.size());
  if (!s.empty()) dev.download(m_cur.s, s.data(), s.size());
  if (!y.empty()) dev.download(m_cur.y, y.data(), y.size());
  if (!z.empty()) dev.download(m_cur.z, z.data(), z.size());
}

void BatchDevice::get_instance(int b, std::vector<double>& x, std::vector<double>& s, std::vector<double>& y,
                               std::vector<double>& z, std::vector<double>& V) {
  if (b < 0 || b >= B) throw std::runtime_error("BatchDevice::get_instance: no such instance");
  DeviceNlp& dev = sys.device();
  x.resize(n);
  s.resize(m_i);
  y.resize(m_e);
  z.resize(m_i);
  V.resize(nV);
  if (n) dev.download(m_cur.x + static_cast<size_t>(b) * n, x.data(), n);
  if (m_i) dev.download(m_cur.s + static_cast<size_t>(b) * m_i, s.data(), m_i);
  if (m_e) dev.download(m_cur.y + static_cast<size_t>(b) * m_e, y.data(), m_e);
  if (m_i) dev.download(m_cur.z + static_cast<size_t>(b) * m_i, z.data(), m_i);
  dev.download(m_Vcur.p + static_cast<size_t>(b) * nV, V.data(), nV);
}

void BatchDevice::put_instance(int b, const std::vector<double>& x, const std::vector<double>& s, const std::vector<double>& y,
                               const std::vector<double>& z) {
  if (b < 0 || b >= B || x.size() != static_cast<size_t>(n) || s.size() != static_cast<size_t>(m_i) ||
      y.size() != static_cast<size_t>(m_e) || z.size() != static_cast<size_t>(m_i))
    throw std::runtime_error("BatchDevice::put_instance: wrong instance or lengths");
  auto put = [](double* d, const std::vector<double>& h) {
    if (!h.empty()) SLPX_HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  };
  put(m_cur.x + static_cast<size_t>(b) * n, x);
  put(m_cur.s + static_cast<size_t>(b) * m_i, s);
  put(m_cur.y + static_cast<size_t>(b) * m_e, y);
  put(m_cur.z + static_cast<size_t>(b) * m_i, z);
}

void BatchDevice::scale_V(int count) {
  DeviceNlp& dev = sys.device();
  hipLaunchKernelGGL(batch_scale_V_kernel, dim3(chunks(count), B), dim3(kBatchThreads), 0, dev.stream(), dev.d_V(), nV,
                     count, m_scale_idx.p, m_is_static.p, m_static_raw.p, m_scales.p, ns, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void BatchDevice::download_out(size_t per_instance, std::vector<double>& out) {
  out.resize(static_cast<size_t>(B) * per_instance);
  sys.device().download(m_out.p, out.data(), out.size());
}

void BatchDevice::errors(const double* V, bool trial, std::vector<double>& err) {
  DeviceNlp& dev = sys.device();
  hipLaunchKernelGGL(batch_errors_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(), V, nV, nV,
                     trial ? m_trial : m_cur, m_mu_of_errors, m_scales.p, ns, m_active.p, m_out.p);
  SLPX_HIP_CHECK(hipGetLastError());
  download_out(kBatchErrN, err);
}

void BatchDevice::sweep_iterate(bool with_state) {
  DeviceNlp& dev = sys.device();
  hipStream_t st = dev.stream();
  hipLaunchKernelGGL(batch_load_state_kernel, dim3(B), dim3(kBatchThreads), 0, st, dev.kdev(), dev.d_x(),
                     sys.structure().n_inputs(), m_cur, m_scales.p, ns, dev.d_s(), dev.d_y(), dev.d_z(), with_state ? 1 : 0,
                     m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
  dev.sweep_full();
  scale_V(nV);
}

void BatchDevice::refresh(std::vector<double>& err) {
  DeviceNlp& dev = sys.device();
  sweep_iterate(true);
  SLPX_HIP_CHECK(hipMemcpyAsync(m_Vcur.p, dev.d_V(), m_Vcur.n * sizeof(double), hipMemcpyDeviceToDevice, dev.stream()));
  errors(m_Vcur.p, false, err);
}

void BatchDevice::warm_start(const BatchWarmStart& ws, const std::vector<uint8_t>& run, const std::vector<double>& mu_min,
                             std::vector<double>& out) {
  DeviceNlp& dev = sys.device();
  const size_t Bs = B;
  if (run.size() != Bs || mu_min.size() != Bs) throw std::runtime_error("BatchDevice::warm_start: wrong lengths");
  auto put = [&](DevBuf<double>& buf, const double* h, size_t count) -> const double* {
    if (h == nullptr || count == 0) return nullptr;
    if (buf.n != count) buf.alloc(count);
    SLPX_HIP_CHECK(hipMemcpy(buf.p, h, count * sizeof(double), hipMemcpyHostToDevice));
    return buf.p;
  };
  std::vector<double> mu_in(2 * Bs);
  for (size_t b = 0; b < Bs; ++b) {
    mu_in[2 * b] = ws.mu ? ws.mu[b] : 0.0;
    mu_in[2 * b + 1] = mu_min[b];
  }
  BatchWarmArgs A{};
  A.n = n;
  A.m_e = m_e;
  A.m_i = m_i;
  A.s0 = put(m_ws_s, ws.s, Bs * m_i);
  A.y0 = put(m_ws_y, ws.y, Bs * m_e);
  A.z0 = put(m_ws_z, ws.z, Bs * m_i);
  A.mu_in = put(m_ws_mu, mu_in.data(), 2 * Bs);
  A.V = dev.d_V();
  A.v_stride = nV;
  A.off_ci = sys.structure().off_ci;
  A.S = m_scales.p;
  A.ns = ns;
  A.cur = m_cur;
  if (m_ws_run.n != Bs) m_ws_run.alloc(Bs);
  SLPX_HIP_CHECK(hipMemcpy(m_ws_run.p, run.data(), Bs, hipMemcpyHostToDevice));
  A.run = m_ws_run.p;
  if (m_ws_out.n != Bs * kWarmOutN) m_ws_out.alloc(Bs * kWarmOutN);
  m_ws_out.zero(dev.stream());
  A.out = m_ws_out.p;
  hipLaunchKernelGGL(batch_warm_start_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), A);
  SLPX_HIP_CHECK(hipGetLastError());
  out.resize(Bs * kWarmOutN);
  dev.download(m_ws_out.p, out.data(), out.size());
}

void BatchDevice::unscaled_iterate(const std::vector<uint8_t>& run, std::vector<double>& s_u, std::vector<double>& y_u,
                                   std::vector<double>& z_u) {
  DeviceNlp& dev = sys.device();
  const size_t Bs = B;
  if (run.size() != Bs) throw std::runtime_error("BatchDevice::unscaled_iterate: wrong lengths");
  // (the three outputs in the buffers a warm start's inputs came in: they are not needed any more)
  const size_t Bi = at_least_1(Bs * m_i), Be = at_least_1(Bs * m_e);
  if (m_ws_s.n != Bi) m_ws_s.alloc(Bi);
  if (m_ws_y.n != Be) m_ws_y.alloc(Be);
  if (m_ws_z.n != Bi) m_ws_z.alloc(Bi);
  for (auto* b : {&m_ws_s, &m_ws_y, &m_ws_z}) b->zero(dev.stream());
  if (m_ws_run.n != Bs) m_ws_run.alloc(Bs);
  SLPX_HIP_CHECK(hipMemcpy(m_ws_run.p, run.data(), Bs, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(batch_unscale_iterate_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), m_e, m_i, m_cur, m_scales.p,
                     ns, m_ws_run.p, m_ws_s.p, m_ws_y.p, m_ws_z.p);
  SLPX_HIP_CHECK(hipGetLastError());
  s_u.resize(Bs * m_i);
  y_u.resize(Bs * m_e);
  z_u.resize(Bs * m_i);
  if (!s_u.empty()) dev.download(m_ws_s.p, s_u.data(), s_u.size());
  if (!y_u.empty()) dev.download(m_ws_y.p, y_u.data(), y_u.size());
  if (!z_u.empty()) dev.download(m_ws_z.p, z_u.data(), z_u.size());
}

// ---- BatchIpmDevice (ipm_batch.hpp) ----

BatchIpmDevice::BatchIpmDevice(NewtonSystem& sys_) : BatchDevice(sys_) {
  mu.assign(B, 0.0);
  tau.assign(B, 0.0);
  alpha_z.assign(B, 0.0);
  s_from_ci.assign(B, 0);
  m_s_from_ci.alloc(B);
  for (auto* b : {&m_mu, &m_tau, &m_alpha_z}) b->alloc(B);
  const size_t Bi = at_least_1(static_cast<size_t>(B) * m_i);
  for (auto* b : {&m_s, &m_z, &m_ts, &m_tz, &m_ss, &m_sz, &m_ps, &m_pz, &m_tci, &m_scims, &m_t}) b->alloc(Bi);
  m_p.alloc(static_cast<size_t>(B) * dim);
  m_cur = BatchIter{m_x.p, m_s.p, m_y.p, m_z.p};
  m_trial = BatchIter{m_tx.p, m_ts.p, m_ty.p, m_tz.p};
  m_mu_of_errors = m_mu.p;
}

void BatchIpmDevice::upload() {
  put_async(m_mu, mu);
  put_async(m_tau, tau);
  put_async(m_alpha_z, alpha_z);
  put_async(m_s_from_ci, s_from_ci);
  BatchDevice::upload();
}

void BatchIpmDevice::newton_direction(std::vector<double>& dir) {
  DeviceNlp& dev = sys.device();
  hipStream_t st = dev.stream();
  SLPX_HIP_CHECK(hipMemcpyAsync(m_p.p, dev.ldlt().d_p(), m_p.n * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (m_i) {
    SLPX_HIP_CHECK(hipMemcpyAsync(m_ps.p, dev.d_ps(), static_cast<size_t>(B) * m_i * sizeof(double), hipMemcpyDeviceToDevice, st));
    SLPX_HIP_CHECK(hipMemcpyAsync(m_pz.p, dev.d_pz(), static_cast<size_t>(B) * m_i * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  hipLaunchKernelGGL(batch_direction_kernel, dim3(B), dim3(kBatchThreads), 0, st, dev.kdev(), m_Vcur.p, nV, m_s.p, m_z.p, m_p.p,
                     m_ps.p, m_pz.p, m_mu.p, m_tau.p, m_active.p, m_out.p);
  SLPX_HIP_CHECK(hipGetLastError());
  download_out(3, dir);
}

void BatchIpmDevice::launch_trial(int with_duals) {
  DeviceNlp& dev = sys.device();
  BatchTrialArgs A{};
  A.cur = m_cur;
  A.trial = m_trial;
  A.soc = BatchIter{m_sx.p, m_ss.p, m_sy.p, m_sz.p};
  A.p = m_p.p;
  A.ps = m_ps.p;
  A.pz = m_pz.p;
  A.mode = m_mode.p;
  A.s_from_ci = m_s_from_ci.p;
  A.alpha = m_alpha.p;
  A.alpha_z = m_alpha_z.p;
  A.in = dev.d_x();
  A.in_stride = sys.structure().n_inputs();
  A.S = m_scales.p;
  A.ns = ns;
  A.with_duals = with_duals;
  hipLaunchKernelGGL(batch_trial_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(), A, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void BatchIpmDevice::trial_values(std::vector<double>& met) {
  DeviceNlp& dev = sys.device();
  launch_trial(0);
  dev.sweep_values();
  scale_V(sys.structure().off_g);
  hipLaunchKernelGGL(batch_trial_metrics_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(), dev.d_V(), nV,
                     m_s_from_ci.p, m_mode.p, m_ts.p, m_tce.p, m_tci.p, m_active.p, m_out.p);
  SLPX_HIP_CHECK(hipGetLastError());
  download_out(4, met);
}

void BatchIpmDevice::soc_step(std::vector<double>& sd) {
  DeviceNlp& dev = sys.device();
  hipStream_t st = dev.stream();
  BatchSocArgs A{};
  A.V = m_Vcur.p;
  A.v_stride = nV;
  A.cur = m_cur;
  A.ts = m_ts.p;
  A.tce = m_tce.p;
  A.tci = m_tci.p;
  A.alpha_soc = m_alpha_soc.p;
  A.mu = m_mu.p;
  A.first = m_first.p;
  A.sce = m_sce.p;
  A.scims = m_scims.p;
  A.t = m_t.p;
  A.rhs = dev.d_rhs();
  hipLaunchKernelGGL(batch_soc_rhs_kernel, dim3(B), dim3(kBatchThreads), 0, st, dev.kdev(), A, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
  dev.solve();  // (every instance's factor; the slices of the others are not read)
  hipLaunchKernelGGL(batch_soc_direction_kernel, dim3(B), dim3(kBatchThreads), 0, st, dev.kdev(), m_Vcur.p, nV, dev.ldlt().d_p(),
                     m_cur, m_scims.p, m_mu.p, m_tau.p, BatchIter{m_sx.p, m_ss.p, m_sy.p, m_sz.p},
                     m_active.p, m_out.p);
  SLPX_HIP_CHECK(hipGetLastError());
  download_out(2, sd);
}

void BatchIpmDevice::kkt_fallback(std::vector<double>& err_cur, std::vector<double>& err_trial) {
  DeviceNlp& dev = sys.device();
  // the full step's s is s + alpha_max p_s, never the trial c_i (:697)
  std::fill(s_from_ci.begin(), s_from_ci.end(), uint8_t{0});
  upload();
  errors(m_Vcur.p, false, err_cur);
  launch_trial(1);
  dev.sweep_full();
  scale_V(nV);
  errors(dev.d_V(), true, err_trial);
}

void BatchIpmDevice::commit() {
  DeviceNlp& dev = sys.device();
  hipLaunchKernelGGL(batch_commit_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(),
                     m_trial, m_cur, m_mu.p, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

// ---- BatchEqDevice (eq_batch.hpp) ----

BatchEqDevice::BatchEqDevice(NewtonSystem& sys_) : BatchDevice(sys_) {
  if (m_i != 0) throw std::runtime_error("BatchEqDevice: a model without inequality constraints only");
  m_px.alloc(at_least_1(static_cast<size_t>(B) * n));
  m_py.alloc(at_least_1(static_cast<size_t>(B) * m_e));
  m_zero.upload(std::vector<double>(B, 0.0));  // (the barrier parameter batch_errors_kernel reads: none here)
  m_none.alloc(1);                             // (s, z of an iterate without inequality rows: never read)
  m_cur = BatchIter{m_x.p, m_none.p, m_y.p, m_none.p};
  m_trial = BatchIter{m_tx.p, m_none.p, m_ty.p, m_none.p};
  m_mu_of_errors = m_zero.p;
}

void BatchEqDevice::direction(std::vector<double>& dphi) {
  DeviceNlp& dev = sys.device();
  hipLaunchKernelGGL(eq_direction_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(), m_Vcur.p, nV, dev.ldlt().d_p(),
                     EqIter{m_px.p, m_py.p}, m_active.p, m_out.p);
  SLPX_HIP_CHECK(hipGetLastError());
  download_out(1, dphi);
}

void BatchEqDevice::launch_trial(int with_duals) {
  DeviceNlp& dev = sys.device();
  EqTrialArgs A{};
  A.cur = EqIter{m_x.p, m_y.p};
  A.trial = EqIter{m_tx.p, m_ty.p};
  A.newton = EqIter{m_px.p, m_py.p};
  A.soc = EqIter{m_sx.p, m_sy.p};
  A.mode = m_mode.p;
  A.alpha = m_alpha.p;
  A.in = dev.d_x();
  A.in_stride = sys.structure().n_inputs();
  A.S = m_scales.p;
  A.ns = ns;
  A.with_duals = with_duals;
  hipLaunchKernelGGL(eq_trial_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(), A, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

void BatchEqDevice::trial_values(std::vector<double>& met) {
  DeviceNlp& dev = sys.device();
  launch_trial(0);
  dev.sweep_values();
  scale_V(sys.structure().off_g);
  hipLaunchKernelGGL(eq_trial_metrics_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(), dev.d_V(), nV,
                     m_tce.p, m_active.p, m_out.p);
  SLPX_HIP_CHECK(hipGetLastError());
  download_out(3, met);
}

void BatchEqDevice::soc_step() {
  DeviceNlp& dev = sys.device();
  hipStream_t st = dev.stream();
  EqSocArgs A{};
  A.V = m_Vcur.p;
  A.v_stride = nV;
  A.y = m_y.p;
  A.tce = m_tce.p;
  A.alpha_soc = m_alpha_soc.p;
  A.first = m_first.p;
  A.sce = m_sce.p;
  A.rhs = dev.d_rhs();
  hipLaunchKernelGGL(eq_soc_rhs_kernel, dim3(B), dim3(kBatchThreads), 0, st, dev.kdev(), A, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
  dev.solve();  // (every instance's factor; the slices of the others are not read)
  hipLaunchKernelGGL(eq_direction_kernel, dim3(B), dim3(kBatchThreads), 0, st, dev.kdev(), m_Vcur.p, nV, dev.ldlt().d_p(),
                     EqIter{m_sx.p, m_sy.p}, m_active.p, static_cast<double*>(nullptr));
  SLPX_HIP_CHECK(hipGetLastError());
}

void BatchEqDevice::kkt_fallback(std::vector<double>& err_cur, std::vector<double>& err_trial) {
  DeviceNlp& dev = sys.device();
  errors(m_Vcur.p, false, err_cur);
  launch_trial(1);
  dev.sweep_full();
  scale_V(nV);
  errors(dev.d_V(), true, err_trial);
}

void BatchEqDevice::commit() {
  DeviceNlp& dev = sys.device();
  hipLaunchKernelGGL(eq_commit_kernel, dim3(B), dim3(kBatchThreads), 0, dev.stream(), dev.kdev(), EqIter{m_tx.p, m_ty.p},
                     EqIter{m_x.p, m_y.p}, m_active.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

}  // namespace slpx
