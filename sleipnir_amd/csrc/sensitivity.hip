// The kernels of the solution sensitivities and their driver (sensitivity.hpp).  Opt-in: nothing on the path of a
// solve comes here.
//
// Four kernels, all row-local gathers — one lane computes one output entry with the row formulas of sens_rows.h, the
// bodies the host executor (sens_plan.cpp) runs — so an entry's bits do not depend on the launch geometry:
//   sens_rhs_kernel      V' (extended sweep), V, s, z -> every column of M and of R in one launch, grid (rows, n_p)
//   sens_combine_kernel  R dp and (dc_i/dp) dp for the jvp
//   sens_expand_kernel   [dx; -dy] -> dx, ds = A_i dx + r_i, dy, dz = -Sigma ds, grid (entries, columns)
//   sens_vjp_kernel      w^T R[:, q], one workgroup per parameter, lanes and fold in the fixed order of sens_rows.h
// Plain vector loads and stores only.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>

#include "sens_rows.h"
#include "sensitivity.hpp"

namespace slpx {

constexpr int kSensThreads = 256;

__global__ __launch_bounds__(kSensThreads) void sens_rhs_kernel(SensDev d, const double* __restrict__ Vx, const double* __restrict__ V,
                                                               const double* __restrict__ s, const double* __restrict__ z,
                                                               double* __restrict__ M, double* __restrict__ R) {
  const int row = static_cast<int>(blockIdx.x) * kSensThreads + static_cast<int>(threadIdx.x);
  const int q = static_cast<int>(blockIdx.y);
  if (row >= d.dimM || q >= d.n_p) return;
  const int64_t k = static_cast<int64_t>(q) * d.dimM + row;
  const double m = sens_m_entry(d.m_ptr, d.m_src, Vx, k);
  M[k] = m;
  if (row < d.dim)
    R[static_cast<int64_t>(q) * d.dim + row] =
        sens_reduced_entry(d.n, d.m_e, d.dimM, d.m_ptr, d.m_src, d.red_ptr, d.red_src, d.red_row, Vx, V, s, z, q, row, m);
}

__global__ __launch_bounds__(kSensThreads) void sens_combine_kernel(SensDev d, const double* __restrict__ M, const double* __restrict__ R,
                                                                   const double* __restrict__ dp, double* __restrict__ rhs,
                                                                   double* __restrict__ r_i) {
  const int row = static_cast<int>(blockIdx.x) * kSensThreads + static_cast<int>(threadIdx.x);
  if (row >= d.dimM) return;
  if (row < d.dim) rhs[row] = sens_combine_entry(d.n_p, R, d.dim, 0, row, dp);
  else r_i[row - d.dim] = sens_combine_entry(d.n_p, M, d.dimM, d.dim, row - d.dim, dp);
}

// column c: sol + c * dim -> out + c * dimOut, laid out [dx (n) | ds (m_i) | dy (m_e) | dz (m_i)]; r_i of the column at
// r_i + c * r_i_stride
__global__ __launch_bounds__(kSensThreads) void sens_expand_kernel(SensDev d, int columns, const double* __restrict__ V,
                                                                  const double* __restrict__ s, const double* __restrict__ z,
                                                                  const double* __restrict__ sol, const double* __restrict__ r_i,
                                                                  long long r_i_stride, double* __restrict__ out) {
  const int e = static_cast<int>(blockIdx.x) * kSensThreads + static_cast<int>(threadIdx.x);
  const int c = static_cast<int>(blockIdx.y);
  if (e >= d.dimM || c >= columns) return;
  const double* p = sol + static_cast<int64_t>(c) * d.dim;
  double* o = out + static_cast<int64_t>(c) * (d.dimM + d.m_i);
  if (e < d.n) {
    o[e] = p[e];
  } else if (e < d.dim) {
    o[d.n + d.m_i + (e - d.n)] = -p[e];
  } else {
    const int j = e - d.dim;
    const double ds = sens_ds_entry(d.ai_rowptr, d.ai_col, d.ai_src, V, p, r_i + static_cast<int64_t>(c) * r_i_stride, j);
    o[d.n + j] = ds;
    o[d.n + d.m_i + d.m_e + j] = sens_dz_entry(s[j], z[j], ds);
  }
}

__global__ __launch_bounds__(kSensVjpThreads) void sens_vjp_kernel(SensDev d, const double* __restrict__ R, const double* __restrict__ w,
                                                                  double* __restrict__ grad) {
  __shared__ double part[kSensVjpThreads];
  const int q = static_cast<int>(blockIdx.x);
  const int t = static_cast<int>(threadIdx.x);
  part[t] = sens_vjp_partial(d.dim, R + static_cast<int64_t>(q) * d.dim, w, t);
  __syncthreads();
  for (int width = kSensVjpThreads / 2; width > 0; width >>= 1) {
    if (t < width) part[t] = part[t] + part[t + width];
    __syncthreads();
  }
  if (t == 0) grad[q] = part[0];
}

namespace {
using clk = std::chrono::steady_clock;
double seconds_since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }
int blocks_for(int count) { return std::max(1, (count + kSensThreads - 1) / kSensThreads); }
}  // namespace

Sensitivity::Sensitivity(NewtonSystem& model, NodeId f) : m_model(model) {
  const auto t0 = clk::now();
  if (!model.has_device()) throw std::runtime_error("slpx: sensitivity: the model's system has no device");
  if (model.batch() != 1) throw std::runtime_error("slpx: sensitivity: the model's system must be a single problem");
  const std::vector<NodeId> params = model.structure().parameter_nodes();
  if (params.empty()) throw std::runtime_error("slpx: sensitivity: the model reaches no parameter");
  if (params.size() > 65535) throw std::runtime_error("slpx: sensitivity: more than 65535 parameters (one grid row each)");
  // x' = [x ; p]: the parameters behind the decision variables, in the order of every parameter vector
  std::vector<NodeId> xp = model.x_nodes();
  xp.insert(xp.end(), params.begin(), params.end());
  NewtonOptions opt;
  opt.tape = model.options().tape;
  opt.device = model.options().device;
  m_ext = std::make_unique<NewtonSystem>(model.graph(), xp, f, model.c_e_nodes(), model.c_i_nodes(), opt);
  m_ext->device().set_scaling(std::vector<double>(m_ext->structure().n_scales(), 1.0));
  m_plan = build_sens_plan(model.structure(), m_ext->structure());
  const SensPlan& p = m_plan;
  m_m_ptr.upload(p.m_ptr);
  m_m_src.upload(p.m_src);
  m_red_ptr.upload(p.red_ptr);
  m_red_src.upload(p.red_src);
  m_red_row.upload(p.red_row);
  m_ai_rowptr.upload(p.ai_rowptr);
  m_ai_col.upload(p.ai_col);
  m_ai_src.upload(p.ai_src);
  const size_t n_p = static_cast<size_t>(p.n_p);
  m_M.alloc(n_p * p.dimM);
  m_R.alloc(n_p * p.dim);
  m_V.alloc(static_cast<size_t>(p.nV));
  m_s.alloc(static_cast<size_t>(std::max(1, p.m_i)));
  m_z.alloc(static_cast<size_t>(std::max(1, p.m_i)));
  m_vec.alloc(static_cast<size_t>(std::max(p.n_p, p.dim)));
  m_rhs1.alloc(static_cast<size_t>(p.dim));
  m_ri1.alloc(static_cast<size_t>(std::max(1, p.m_i)));
  m_sol.alloc(n_p * p.dim);
  m_out.alloc(n_p * (static_cast<size_t>(p.dimM) + p.m_i));
  m_grad.alloc(n_p);
  m_compile_seconds = seconds_since(t0);
}

Sensitivity::~Sensitivity() = default;

SensDev Sensitivity::view() const {
  const SensPlan& p = m_plan;
  return SensDev{p.n, p.n_p, p.m_e, p.m_i, p.dim, p.dimM, m_m_ptr.p, m_m_src.p, m_red_ptr.p, m_red_src.p, m_red_row.p,
                 m_ai_rowptr.p, m_ai_col.p, m_ai_src.p};
}

// Both systems at the iterate, unit scales, the user's units: V' and V swept, M and R written, the model's lhs
// assembled (and a right-hand side of its own built: the factorization carries one along).
void Sensitivity::evaluate(const Point& at) {
  if (m_evaluated) return;
  const SensPlan& p = m_plan;
  const size_t n = p.n, n_p = p.n_p, m_e = p.m_e, m_i = p.m_i;
  if (at.x->size() != n || at.s->size() != m_i || at.y->size() != m_e || at.z->size() != m_i || at.parameters->size() != n_p)
    throw std::runtime_error("slpx: sensitivity: the iterate does not have the model's sizes");
  DeviceNlp& dev = m_model.device();
  DeviceNlp& ext = m_ext->device();
  m_factored = false;
  // (upload_duals reads all three arrays whatever the sizes)
  const std::vector<double> pad(1, 1.0);
  const double* s = m_i ? at.s->data() : pad.data();
  const double* z = m_i ? at.z->data() : pad.data();
  const double* y = m_e ? at.y->data() : pad.data();
  std::vector<double> xp(*at.x);
  xp.insert(xp.end(), at.parameters->begin(), at.parameters->end());
  ext.upload_x(xp.data());
  ext.upload_duals(s, y, z);
  ext.sweep_full();
  SLPX_HIP_CHECK(hipStreamSynchronize(ext.stream()));  // (the two systems may run on different streams)
  SLPX_HIP_CHECK(hipStreamSynchronize(dev.stream()));
  dev.set_scaling(std::vector<double>(m_model.structure().n_scales(), 1.0));
  dev.upload_x(at.x->data());
  dev.upload_duals(s, y, z);
  dev.upload_mu(&at.mu);
  dev.sweep_full();
  const hipStream_t st = dev.stream();
  SLPX_HIP_CHECK(hipMemcpyAsync(m_V.p, dev.d_V(), static_cast<size_t>(p.nV) * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (m_i) {
    SLPX_HIP_CHECK(hipMemcpyAsync(m_s.p, dev.d_s(), m_i * sizeof(double), hipMemcpyDeviceToDevice, st));
    SLPX_HIP_CHECK(hipMemcpyAsync(m_z.p, dev.d_z(), m_i * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  hipLaunchKernelGGL(sens_rhs_kernel, dim3(blocks_for(p.dimM), p.n_p), dim3(kSensThreads), 0, st, view(), ext.d_V(), m_V.p, m_s.p, m_z.p,
                     m_M.p, m_R.p);
  SLPX_HIP_CHECK(hipGetLastError());
  dev.assemble();
  dev.build_rhs();
  // (what is in memory IS the system now: a request the last solve left for a step that never came is void)
  dev.system_written_by_caller(/*lhs=*/true, /*rhs=*/true);
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (`at` is the caller's)
  m_evaluated = true;
}

// NewtonSystem::compute() on the lhs evaluate() left: the ordinary policy loop from a cleared memory, the system's own
// memory and the caller's scaling put back afterwards.
void Sensitivity::factor(const Point& at, SensitivityInfo& info) {
  evaluate(at);
  if (!m_factored) {
    const auto t0 = clk::now();
    DeviceNlp& dev = m_model.device();
    const NewtonSystem::RegularizationState saved = m_model.regularization_state();
    m_model.reset_regularization();
    std::vector<FactorInfo> res;
    try {
      res = m_model.compute();
    } catch (...) {
      m_model.set_regularization_state(saved);
      throw;
    }
    m_delta = m_model.hessian_regularization()[0];
    m_gamma = m_model.constraint_jacobian_regularization()[0];
    info.factorizations += m_model.last_factorizations();
    m_model.set_regularization_state(saved);
    std::vector<LdltStats> stats;
    dev.read_stats(stats);
    m_n_pos = stats[0].n_pos;
    m_n_neg = stats[0].n_neg;
    m_n_zero = stats[0].n_zero;
    // (V of the model system is its own copy here; the lhs in memory stays the one that was factored)
    if (at.scales_after != nullptr && static_cast<int>(at.scales_after->size()) == m_model.structure().n_scales())
      dev.set_scaling(*at.scales_after);
    if (res[0] != FactorInfo::Success)
      throw std::runtime_error("slpx: sensitivity: the KKT system at the iterate could not be factored (delta " + std::to_string(m_delta) +
                               ", gamma " + std::to_string(m_gamma) + ")");
    m_factored = true;
    info.t_factor += seconds_since(t0);
  }
  info.n_pos = m_n_pos;
  info.n_neg = m_n_neg;
  info.n_zero = m_n_zero;
  info.delta = m_delta;
  info.gamma = m_gamma;
}

void Sensitivity::solve_one(const double* rhs, double* sol, SensitivityInfo& info) {
  DeviceNlp& dev = m_model.device();
  const size_t bytes = static_cast<size_t>(m_plan.dim) * sizeof(double);
  const hipStream_t st = dev.stream();
  SLPX_HIP_CHECK(hipMemcpyAsync(dev.rhs_raw(), rhs, bytes, hipMemcpyDeviceToDevice, st));
  dev.system_written_by_caller(/*lhs=*/false, /*rhs=*/true);
  dev.solve();
  ++info.solves;
  const NewtonSystem::Refinement ref = m_model.refine(2);
  info.refine_steps += ref.accepted[0];
  info.solves += ref.accepted[0];
  const double berr = m_model.error_bounds(nullptr, /*want_ferr=*/false).berr[0];
  if (!(berr <= info.berr_max)) info.berr_max = berr;  // (a NaN shows)
  SLPX_HIP_CHECK(hipMemcpyAsync(sol, dev.d_p(), bytes, hipMemcpyDeviceToDevice, st));
}

void Sensitivity::expand_and_download(int columns, const double* r_i, long long r_i_stride, double* dx, double* ds, double* dy,
                                      double* dz) {
  const SensPlan& p = m_plan;
  DeviceNlp& dev = m_model.device();
  const hipStream_t st = dev.stream();
  hipLaunchKernelGGL(sens_expand_kernel, dim3(blocks_for(p.dimM), columns), dim3(kSensThreads), 0, st, view(), columns, m_V.p, m_s.p, m_z.p,
                     m_sol.p, r_i, r_i_stride, m_out.p);
  SLPX_HIP_CHECK(hipGetLastError());
  const size_t stride = static_cast<size_t>(p.dimM) + p.m_i;
  std::vector<double> out(static_cast<size_t>(columns) * stride);
  dev.download(m_out.p, out.data(), out.size());
  for (int c = 0; c < columns; ++c) {
    const double* o = out.data() + c * stride;
    if (dx) std::copy(o, o + p.n, dx + static_cast<size_t>(c) * p.n);
    if (ds) std::copy(o + p.n, o + p.n + p.m_i, ds + static_cast<size_t>(c) * p.m_i);
    if (dy) std::copy(o + p.n + p.m_i, o + p.n + p.m_i + p.m_e, dy + static_cast<size_t>(c) * p.m_e);
    if (dz) std::copy(o + p.n + p.m_i + p.m_e, o + stride, dz + static_cast<size_t>(c) * p.m_i);
  }
}

void Sensitivity::jacobian(const Point& at, double* dx, double* ds, double* dy, double* dz, SensitivityInfo& info) {
  const auto t0 = clk::now();
  const SensPlan& p = m_plan;
  info.n_p = p.n_p;
  info.t_compile = take_compile_seconds();
  factor(at, info);
  for (int q = 0; q < p.n_p; ++q) solve_one(m_R.p + static_cast<size_t>(q) * p.dim, m_sol.p + static_cast<size_t>(q) * p.dim, info);
  expand_and_download(p.n_p, m_M.p + p.dim, p.dimM, dx, ds, dy, dz);
  info.t_total = seconds_since(t0) + info.t_compile;
}

void Sensitivity::jvp(const Point& at, const double* dp, double* dx, double* ds, double* dy, double* dz, SensitivityInfo& info) {
  const auto t0 = clk::now();
  const SensPlan& p = m_plan;
  if (dp == nullptr) throw std::runtime_error("slpx: sensitivity jvp: dp is null");
  info.n_p = p.n_p;
  info.t_compile = take_compile_seconds();
  factor(at, info);
  DeviceNlp& dev = m_model.device();
  const hipStream_t st = dev.stream();
  SLPX_HIP_CHECK(hipMemcpyAsync(m_vec.p, dp, static_cast<size_t>(p.n_p) * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(sens_combine_kernel, dim3(blocks_for(p.dimM)), dim3(kSensThreads), 0, st, view(), m_M.p, m_R.p, m_vec.p, m_rhs1.p,
                     m_ri1.p);
  SLPX_HIP_CHECK(hipGetLastError());
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (dp is the caller's)
  solve_one(m_rhs1.p, m_sol.p, info);
  expand_and_download(1, m_ri1.p, 0, dx, ds, dy, dz);
  info.t_total = seconds_since(t0) + info.t_compile;
}

void Sensitivity::vjp(const Point& at, const double* vx, double* grad, SensitivityInfo& info) {
  const auto t0 = clk::now();
  const SensPlan& p = m_plan;
  if (vx == nullptr) throw std::runtime_error("slpx: sensitivity vjp: vx is null");
  info.n_p = p.n_p;
  info.t_compile = take_compile_seconds();
  factor(at, info);
  DeviceNlp& dev = m_model.device();
  const hipStream_t st = dev.stream();
  std::vector<double> rhs(static_cast<size_t>(p.dim), 0.0);  // [vx; 0]
  std::copy(vx, vx + p.n, rhs.begin());
  SLPX_HIP_CHECK(hipMemcpyAsync(m_rhs1.p, rhs.data(), rhs.size() * sizeof(double), hipMemcpyHostToDevice, st));
  SLPX_HIP_CHECK(hipStreamSynchronize(st));
  solve_one(m_rhs1.p, m_sol.p, info);
  hipLaunchKernelGGL(sens_vjp_kernel, dim3(p.n_p), dim3(kSensVjpThreads), 0, st, view(), m_R.p, m_sol.p, m_grad.p);
  SLPX_HIP_CHECK(hipGetLastError());
  std::vector<double> g(static_cast<size_t>(p.n_p));
  dev.download(m_grad.p, g.data(), g.size());
  if (grad) std::copy(g.begin(), g.end(), grad);
  info.t_total = seconds_since(t0) + info.t_compile;
}

void Sensitivity::unreduced(const Point& at, double* M) {
  evaluate(at);
  // (evaluate() installed unit scales on the model system: the caller's back, as after a factorization)
  if (at.scales_after != nullptr && static_cast<int>(at.scales_after->size()) == m_model.structure().n_scales() && !m_factored)
    m_model.device().set_scaling(*at.scales_after);
  if (M) m_model.device().download(m_M.p, M, static_cast<size_t>(m_plan.n_p) * m_plan.dimM);
}

}  // namespace slpx
