// The kernels of the solution sensitivities, the layer that launches them, and the two drivers on top of it
// (sensitivity.hpp): one problem (Sensitivity) and B instances at once (BatchSensitivity).  Opt-in: nothing on the path
// of a solve comes here.
//
// Six kernels, all row-local gathers — one lane computes one output entry with the row formulas of sens_rows.h, the
// bodies the host executor (sens_plan.cpp) runs — so an entry's bits do not depend on the launch geometry, on the batch
// size, on the instance's position or on its neighbours:
//   sens_rhs_kernel      V' (extended sweep), V, s, z -> every column of M and of R in one launch
//   sens_combine_kernel  R dp and (dc_i/dp) dp for the jvp
//   sens_expand_kernel   [dx; -dy] -> dx, ds = A_i dx + r_i, dy, dz = -Sigma ds, straight into the caller's layout
//   sens_vjp_kernel      w^T R[:, q], one workgroup per parameter, lanes and fold in the fixed order of sens_rows.h
//   sens_adjoint_rhs_kernel  the full vjp's right-hand side [vx + A_i^T t + vcost g; -vy], t = vs - Sigma o vz (sens_plan.hpp)
//   sens_vjp_full_kernel     w^T R[:, q] + t . r_i[:, q] + vcost f_p[q]: two dot products in sens_vjp_kernel's order, side by side
// THE GRID.  blockIdx.y is the instance (at most 65535 of them: one grid slice each) and every buffer has an instance
// stride.  blockIdx.x runs over the entries of ONE instance with the columns folded in — (parameter, row) for rhs and
// expand.  Each kernel is launched in ONE place, a stage of the layer below, for a SensState of B instances: a grid of
// (blocks, B), the real instance strides — with B = 1 they multiply blockIdx.y = 0 — and the state's launch width.  A
// batch system's state has workgroups of one wave (kSensBatchThreads): the models the batch serves have n_p * dimM of a
// few dozen to a few thousand, so a 256-lane workgroup per (instance, column) would be mostly idle lanes, and it is the
// instance axis that fills the machine.  The state of the problem's own system keeps 256 lanes (kSensThreads), the
// geometry profiles/sensitivity.txt was measured with; the kernels take the workgroup size from the launch.  Plain
// vector loads and stores only; no LDS beyond the fold of the vjp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

#include "sens_rows.h"
#include "sensitivity.hpp"

namespace slpx {

constexpr int kSensThreads = 256;      // the problem's own system
constexpr int kSensBatchThreads = 64;  // a batch system: one wave

// entry e = q * dimM + row of instance blockIdx.y
__global__ __launch_bounds__(kSensThreads) void sens_rhs_kernel(SensDev d, const double* __restrict__ Vx, long long Vx_stride,
                                                               const double* __restrict__ V, long long V_stride,
                                                               const double* __restrict__ s, const double* __restrict__ z,
                                                               long long sz_stride, double* __restrict__ M, double* __restrict__ R) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= static_cast<int64_t>(d.n_p) * d.dimM) return;
  const int64_t b = blockIdx.y;
  const int q = static_cast<int>(e / d.dimM), row = static_cast<int>(e - static_cast<int64_t>(q) * d.dimM);
  Vx += b * Vx_stride;
  const double m = sens_m_entry(d.m_ptr, d.m_src, Vx, e);
  M[b * d.n_p * d.dimM + e] = m;
  if (row < d.dim)
    R[b * d.n_p * d.dim + static_cast<int64_t>(q) * d.dim + row] =
        sens_reduced_entry(d.n, d.m_e, d.dimM, d.m_ptr, d.m_src, d.red_ptr, d.red_src, d.red_row, Vx, V + b * V_stride, s + b * sz_stride,
                           z + b * sz_stride, q, row, m);
}

// instance blockIdx.y: M [n_p][dimM], R [n_p][dim], dp [n_p] -> rhs [dim], r_i [m_i], every one dense per instance
__global__ __launch_bounds__(kSensThreads) void sens_combine_kernel(SensDev d, const double* __restrict__ M, const double* __restrict__ R,
                                                                   const double* __restrict__ dp, double* __restrict__ rhs,
                                                                   double* __restrict__ r_i) {
  const int row = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= d.dimM) return;
  const int64_t b = blockIdx.y;
  M += b * d.n_p * d.dimM;
  R += b * d.n_p * d.dim;
  dp += b * d.n_p;
  if (row < d.dim) rhs[b * d.dim + row] = sens_combine_entry(d.n_p, R, d.dim, 0, row, dp);
  else r_i[b * d.m_i + row - d.dim] = sens_combine_entry(d.n_p, M, d.dimM, d.dim, row - d.dim, dp);
}

// entry e = c * dimM + i of instance b = blockIdx.y: column c of its `columns` solutions, sol + (b * columns + c) * dim,
// into row b * columns + c of dx [.][n], ds [.][m_i], dy [.][m_e], dz [.][m_i]; r_i of the column at
// r_i + b * r_i_instance + c * r_i_column
__global__ __launch_bounds__(kSensThreads) void sens_expand_kernel(SensDev d, int columns, const double* __restrict__ V, long long V_stride,
                                                                  const double* __restrict__ s, const double* __restrict__ z,
                                                                  long long sz_stride, const double* __restrict__ sol,
                                                                  const double* __restrict__ r_i, long long r_i_column,
                                                                  long long r_i_instance, double* __restrict__ dx, double* __restrict__ ds,
                                                                  double* __restrict__ dy, double* __restrict__ dz) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= static_cast<int64_t>(columns) * d.dimM) return;
  const int64_t b = blockIdx.y;
  const int c = static_cast<int>(e / d.dimM), i = static_cast<int>(e - static_cast<int64_t>(c) * d.dimM);
  const int64_t out = b * columns + c;
  const double* p = sol + out * d.dim;
  if (i < d.n) {
    dx[out * d.n + i] = p[i];
  } else if (i < d.dim) {
    dy[out * d.m_e + (i - d.n)] = -p[i];
  } else {
    const int j = i - d.dim;
    const double v = sens_ds_entry(d.ai_rowptr, d.ai_col, d.ai_src, V + b * V_stride, p, r_i + b * r_i_instance + c * r_i_column, j);
    ds[out * d.m_i + j] = v;
    dz[out * d.m_i + j] = sens_dz_entry(s[b * sz_stride + j], z[b * sz_stride + j], v);
  }
}

// workgroup (q, b): grad [b][q] = w[b]^T R[b][:, q]
__global__ __launch_bounds__(kSensVjpThreads) void sens_vjp_kernel(SensDev d, const double* __restrict__ R, const double* __restrict__ w,
                                                                  double* __restrict__ grad) {
  __shared__ double part[kSensVjpThreads];
  const int q = static_cast<int>(blockIdx.x);
  const int64_t b = blockIdx.y;
  const int t = static_cast<int>(threadIdx.x);
  part[t] = sens_vjp_partial(d.dim, R + (b * d.n_p + q) * d.dim, w + b * d.dim, t);
  __syncthreads();
  for (int width = kSensVjpThreads / 2; width > 0; width >>= 1) {
    if (t < width) part[t] = part[t] + part[t + width];
    __syncthreads();
  }
  if (t == 0) grad[b * d.n_p + q] = part[0];
}

// v: the cotangents of the call on the device (null: absent), instance b's rows at vx + b * n, vs + b * m_i, vy + b * m_e,
// vz + b * m_i, vcost + b.  Row `row` < dim of instance blockIdx.y: rhs [b][dim], the buffer the solve is given.
__global__ __launch_bounds__(kSensThreads) void sens_adjoint_rhs_kernel(SensDev d, const double* __restrict__ V, long long V_stride,
                                                                       const double* __restrict__ s, const double* __restrict__ z,
                                                                       long long sz_stride, SensCotangent v, double* __restrict__ rhs) {
  const int row = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= d.dim) return;
  const int64_t b = blockIdx.y;
  rhs[b * d.dim + row] = sens_adjoint_rhs_entry(d.n, d.red_ptr, d.red_src, d.red_row, d.g_src, V + b * V_stride, s + b * sz_stride,
                                                z + b * sz_stride, v.vx ? v.vx + b * d.n : nullptr, v.vs ? v.vs + b * d.m_i : nullptr,
                                                v.vy ? v.vy + b * d.m_e : nullptr, v.vz ? v.vz + b * d.m_i : nullptr,
                                                v.vcost ? v.vcost + b : nullptr, row);
}

// workgroup (q, b): grad [b][q] = w[b]^T R[b][:, q] + t[b] . r_i[b][:, q] + vcost[b] f_p[b][q]
__global__ __launch_bounds__(kSensVjpThreads) void sens_vjp_full_kernel(SensDev d, const double* __restrict__ M, const double* __restrict__ R,
                                                                       const double* __restrict__ w, const double* __restrict__ Vx,
                                                                       long long Vx_stride, const double* __restrict__ s,
                                                                       const double* __restrict__ z, long long sz_stride, SensCotangent v,
                                                                       double* __restrict__ grad) {
  __shared__ double part[kSensVjpThreads], part_t[kSensVjpThreads];
  const int q = static_cast<int>(blockIdx.x);
  const int64_t b = blockIdx.y;
  const int t = static_cast<int>(threadIdx.x);
  const double* vs = v.vs ? v.vs + b * d.m_i : nullptr;
  const double* vz = v.vz ? v.vz + b * d.m_i : nullptr;
  const bool direct = sens_adjoint_has_t(d.m_i, vs, vz);  // (uniform over the workgroup)
  part[t] = sens_vjp_partial(d.dim, R + (b * d.n_p + q) * d.dim, w + b * d.dim, t);
  part_t[t] = direct ? sens_adjoint_direct_partial(d.m_i, M + (b * d.n_p + q) * d.dimM + d.dim, s + b * sz_stride, z + b * sz_stride, vs, vz, t)
                     : 0.0;
  __syncthreads();
  for (int width = kSensVjpThreads / 2; width > 0; width >>= 1) {
    if (t < width) {
      part[t] = part[t] + part[t + width];
      part_t[t] = part_t[t] + part_t[t + width];
    }
    __syncthreads();
  }
  if (t == 0) grad[b * d.n_p + q] = sens_vjp_full_sum(part[0], direct, part_t[0], v.vcost ? v.vcost + b : nullptr, d.fp_src[q], Vx + b * Vx_stride);
}

// ---- the layer under both drivers: every stage once, for a state of B instances ----

void SensPlanDev::build(const NlpStructure& model, const NlpStructure& extended) {
  plan = build_sens_plan(model, extended);
  m_ptr.upload(plan.m_ptr);
  m_src.upload(plan.m_src);
  red_ptr.upload(plan.red_ptr);
  red_src.upload(plan.red_src);
  red_row.upload(plan.red_row);
  ai_rowptr.upload(plan.ai_rowptr);
  ai_col.upload(plan.ai_col);
  ai_src.upload(plan.ai_src);
  g_src.upload(plan.g_src);
  fp_src.upload(plan.fp_src);
  built = true;
}

SensDev SensPlanDev::view() const {
  const SensPlan& p = plan;
  return SensDev{p.n, p.n_p, p.m_e, p.m_i, p.dim, p.dimM, m_ptr.p, m_src.p, red_ptr.p, red_src.p, red_row.p,
                 ai_rowptr.p, ai_col.p, ai_src.p, g_src.p, fp_src.p};
}

namespace {
using clk = std::chrono::steady_clock;
double seconds_since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }
unsigned blocks_for(int64_t count, int threads) { return static_cast<unsigned>(std::max<int64_t>(1, (count + threads - 1) / threads)); }

// The model over x' = [x ; p], the parameters behind the decision variables in the order of every parameter vector:
// the tape and device options of `model`, `batch` instances, unit scales.
std::unique_ptr<NewtonSystem> extended_system(NewtonSystem& model, NodeId f, int batch) {
  const std::vector<NodeId> params = model.structure().parameter_nodes();
  std::vector<NodeId> xp = model.x_nodes();
  xp.insert(xp.end(), params.begin(), params.end());
  NewtonOptions opt;
  opt.tape = model.options().tape;
  opt.device = model.options().device;
  opt.batch = batch;
  auto ext = std::make_unique<NewtonSystem>(model.graph(), xp, f, model.c_e_nodes(), model.c_i_nodes(), opt);
  ext->device().set_scaling(std::vector<double>(ext->structure().n_scales(), 1.0));
  return ext;
}

// The buffers of a state whose B is set, and room for `columns` solutions per instance and their expansion.
void size_state(SensState& S, const SensPlan& p, int columns) {
  const size_t B = static_cast<size_t>(S.B), n_p = static_cast<size_t>(p.n_p);
  if (S.M.p == nullptr) {
    S.M.alloc(B * n_p * p.dimM);
    S.R.alloc(B * n_p * p.dim);
    S.V.alloc(B * p.nV);
    S.s.alloc(B * std::max(1, p.m_i));
    S.z.alloc(B * std::max(1, p.m_i));
    S.vec.alloc(B * n_p);
    S.rhs1.alloc(B * p.dim);
    S.ri1.alloc(B * std::max(1, p.m_i));
    S.grad.alloc(B * n_p);
    S.cot.alloc(B * static_cast<size_t>(p.n + 2 * p.m_i + p.m_e + 1));
  }
  if (S.columns >= columns) return;
  const size_t rows = B * columns;
  S.sol.alloc(rows * p.dim);
  S.dx.alloc(std::max<size_t>(1, rows * p.n));
  S.ds.alloc(std::max<size_t>(1, rows * p.m_i));
  S.dy.alloc(std::max<size_t>(1, rows * p.m_e));
  S.dz.alloc(std::max<size_t>(1, rows * p.m_i));
  S.columns = columns;
}

// After the sweeps of both systems: V, s, z of the model system (`dev`) into the state's copies, then M and R.
void gather(const SensPlanDev& P, SensState& S, DeviceNlp& dev, hipStream_t st) {
  const SensPlan& p = P.plan;
  const size_t B = static_cast<size_t>(S.B), m_i = static_cast<size_t>(p.m_i);
  SLPX_HIP_CHECK(hipMemcpyAsync(S.V.p, dev.d_V(), B * p.nV * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (m_i) {
    SLPX_HIP_CHECK(hipMemcpyAsync(S.s.p, dev.d_s(), B * m_i * sizeof(double), hipMemcpyDeviceToDevice, st));
    SLPX_HIP_CHECK(hipMemcpyAsync(S.z.p, dev.d_z(), B * m_i * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  hipLaunchKernelGGL(sens_rhs_kernel, dim3(blocks_for(static_cast<int64_t>(p.n_p) * p.dimM, S.threads), S.B), dim3(S.threads), 0, st, P.view(),
                     S.ext->device().d_V(), static_cast<long long>(p.nVx), S.V.p, static_cast<long long>(p.nV), S.s.p, S.z.p,
                     static_cast<long long>(p.m_i), S.M.p, S.R.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

// dp (host, [B][n_p]) -> rhs1 = R dp and ri1 = (dc_i/dp) dp of every instance.  Asynchronous: dp is read until `st` is through.
void combine(const SensPlanDev& P, SensState& S, const double* dp, hipStream_t st) {
  const SensPlan& p = P.plan;
  SLPX_HIP_CHECK(hipMemcpyAsync(S.vec.p, dp, static_cast<size_t>(S.B) * p.n_p * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(sens_combine_kernel, dim3(blocks_for(p.dimM, S.threads), S.B), dim3(S.threads), 0, st, P.view(), S.M.p, S.R.p, S.vec.p,
                     S.rhs1.p, S.ri1.p);
  SLPX_HIP_CHECK(hipGetLastError());
}

// The cotangents of a call as arrays beside the iterate — vx, vs, vy, vz, vcost; one on rows the model does not have is absent.
void cotangent_arrays(const SensCotangent& v, int n, int m_e, int m_i, SensExtraRows out[5]) {
  const SensExtraRows rows[5] = {{n ? v.vx : nullptr, n}, {m_i ? v.vs : nullptr, m_i}, {m_e ? v.vy : nullptr, m_e}, {m_i ? v.vz : nullptr, m_i}, {v.vcost, 1}};
  std::copy(rows, rows + 5, out);
}

// Arrays of B rows each (a null one is absent) behind one another in `packed`, as they will lie on the device; at[k]:
// where array k begins.
void pack_rows(int B, const SensExtraRows* extras, int count, std::vector<double>& packed, std::vector<size_t>& at) {
  at.assign(static_cast<size_t>(count), 0);
  for (int k = 0; k < count; ++k) {
    at[k] = packed.size();
    if (extras[k].rows != nullptr) packed.insert(packed.end(), extras[k].rows, extras[k].rows + static_cast<size_t>(B) * extras[k].width);
  }
}

// The packed cotangents (cotangent_arrays, pack_rows) into `cot`, and the right-hand side of the adjoint solve into rhs1.
// Returns them as the kernels take them; `packed` is free again on return.
SensCotangent adjoint_rhs(const SensPlanDev& P, SensState& S, const SensExtraRows* extras, const std::vector<double>& packed,
                          const std::vector<size_t>& at, hipStream_t st) {
  const SensPlan& p = P.plan;
  SensCotangent v;
  const double** on_device[5] = {&v.vx, &v.vs, &v.vy, &v.vz, &v.vcost};
  for (int k = 0; k < 5; ++k)
    if (extras[k].rows != nullptr) *on_device[k] = S.cot.p + at[k];
  if (!packed.empty()) SLPX_HIP_CHECK(hipMemcpyAsync(S.cot.p, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(sens_adjoint_rhs_kernel, dim3(blocks_for(p.dim, S.threads), S.B), dim3(S.threads), 0, st, P.view(), S.V.p,
                     static_cast<long long>(p.nV), S.s.p, S.z.p, static_cast<long long>(p.m_i), v, S.rhs1.p);
  SLPX_HIP_CHECK(hipGetLastError());
  SLPX_HIP_CHECK(hipStreamSynchronize(st));
  return v;
}

// grad (host, [B][n_p], null: not wanted) from the adjoint solutions in `sol`; ends synchronized.
void vjp_reduce(const SensPlanDev& P, SensState& S, const SensCotangent& v, double* grad, hipStream_t st) {
  const SensPlan& p = P.plan;
  // (w^T R alone — a cotangent on x, or on y — is sens_vjp_kernel's, as before there were others)
  if (!sens_adjoint_has_t(p.m_i, v.vs, v.vz) && v.vcost == nullptr)
    hipLaunchKernelGGL(sens_vjp_kernel, dim3(p.n_p, S.B), dim3(kSensVjpThreads), 0, st, P.view(), S.R.p, S.sol.p, S.grad.p);
  else
    hipLaunchKernelGGL(sens_vjp_full_kernel, dim3(p.n_p, S.B), dim3(kSensVjpThreads), 0, st, P.view(), S.M.p, S.R.p, S.sol.p,
                       S.ext->device().d_V(), static_cast<long long>(p.nVx), S.s.p, S.z.p, static_cast<long long>(p.m_i), v, S.grad.p);
  SLPX_HIP_CHECK(hipGetLastError());
  if (grad) SLPX_HIP_CHECK(hipMemcpyAsync(grad, S.grad.p, static_cast<size_t>(S.B) * p.n_p * sizeof(double), hipMemcpyDeviceToHost, st));
  SLPX_HIP_CHECK(hipStreamSynchronize(st));
}

// `columns` solutions per instance in `sol`, r_i of column c of instance b at r_i + b * r_i_instance + c * r_i_column, into
// the host arrays that are given ([B][columns][.], null: not wanted); ends synchronized.
void expand_and_download(const SensPlanDev& P, SensState& S, int columns, const double* r_i, long long r_i_column, long long r_i_instance,
                         double* dx, double* ds, double* dy, double* dz, hipStream_t st) {
  const SensPlan& p = P.plan;
  hipLaunchKernelGGL(sens_expand_kernel, dim3(blocks_for(static_cast<int64_t>(columns) * p.dimM, S.threads), S.B), dim3(S.threads), 0, st, P.view(),
                     columns, S.V.p, static_cast<long long>(p.nV), S.s.p, S.z.p, static_cast<long long>(p.m_i), S.sol.p, r_i, r_i_column,
                     r_i_instance, S.dx.p, S.ds.p, S.dy.p, S.dz.p);
  SLPX_HIP_CHECK(hipGetLastError());
  // (the kernel wrote the caller's layout: one copy per output array, one wait for all)
  const size_t rows = static_cast<size_t>(S.B) * columns;
  const auto fetch = [&](const DevBuf<double>& from, double* to, int width) {
    const size_t count = rows * width;
    if (to != nullptr && count) SLPX_HIP_CHECK(hipMemcpyAsync(to, from.p, count * sizeof(double), hipMemcpyDeviceToHost, st));
  };
  fetch(S.dx, dx, p.n);
  fetch(S.ds, ds, p.m_i);
  fetch(S.dy, dy, p.m_e);
  fetch(S.dz, dz, p.m_i);
  SLPX_HIP_CHECK(hipStreamSynchronize(st));
}

// NewtonSystem::compute() on the lhs in memory — for the instances of `mask` (null: the unmasked call) — as the ordinary
// policy loop from a CLEARED regularization memory; the memory the system had is put back, also when compute() throws.
struct Factored {
  std::vector<FactorInfo> result;
  std::vector<double> delta, gamma;
  int factorizations = 0;
};
Factored factor_from_cleared_memory(NewtonSystem& model, const std::vector<uint8_t>* mask) {
  const NewtonSystem::RegularizationState saved = model.regularization_state();
  model.reset_regularization();
  Factored out;
  try {
    out.result = mask ? model.compute(/*solve_speculatively=*/false, *mask) : model.compute();
  } catch (...) {
    model.set_regularization_state(saved);
    throw;
  }
  out.delta = model.hessian_regularization();
  out.gamma = model.constraint_jacobian_regularization();
  out.factorizations = model.last_factorizations();
  model.set_regularization_state(saved);
  return out;
}

// One round of solves on the factorization in memory: the right-hand sides in rhs (device, [B] rows `rhs_pitch` doubles
// apart) -> the refined solutions into sol likewise; info [B] of the instances of `mask` (null: all) accounts for it.
void solve_round(NewtonSystem& model, int dim, const double* rhs, size_t rhs_pitch, double* sol, size_t sol_pitch,
                 const std::vector<uint8_t>* mask, SensitivityInfo* info) {
  DeviceNlp& dev = model.device();
  const int B = model.batch();
  const size_t width = static_cast<size_t>(dim) * sizeof(double);
  const hipStream_t st = dev.stream();
  const auto copy_rows = [&](double* to, size_t to_pitch, const double* from, size_t from_pitch) {
    if (B == 1) SLPX_HIP_CHECK(hipMemcpyAsync(to, from, width, hipMemcpyDeviceToDevice, st));
    else SLPX_HIP_CHECK(hipMemcpy2DAsync(to, to_pitch * sizeof(double), from, from_pitch * sizeof(double), width, B, hipMemcpyDeviceToDevice, st));
  };
  copy_rows(dev.rhs_raw(), dim, rhs, rhs_pitch);
  dev.system_written_by_caller(/*lhs=*/false, /*rhs=*/true);
  dev.solve();
  const NewtonSystem::Refinement ref = model.refine(2, mask);
  const NewtonSystem::ErrorBounds eb = model.error_bounds(mask, /*want_ferr=*/false);
  for (int b = 0; b < B; ++b) {
    if (mask != nullptr && !(*mask)[b]) continue;
    info[b].solves += 1 + ref.accepted[b];
    info[b].refine_steps += ref.accepted[b];
    if (!(eb.berr[b] <= info[b].berr_max)) info[b].berr_max = eb.berr[b];  // (a NaN shows)
  }
  copy_rows(sol, sol_pitch, dev.ldlt().d_p(), dim);
}
}  // namespace

// ---- one problem ----

Sensitivity::Sensitivity(NewtonSystem& model, NodeId f) : m_model(model) {
  const auto t0 = clk::now();
  if (!model.has_device()) throw std::runtime_error("slpx: sensitivity: the model's system has no device");
  if (model.batch() != 1) throw std::runtime_error("slpx: sensitivity: the model's system must be a single problem");
  if (model.structure().parameter_nodes().empty()) throw std::runtime_error("slpx: sensitivity: the model reaches no parameter");
  m_state.B = 1;
  m_state.threads = kSensThreads;
  m_state.ext = extended_system(model, f, 1);
  m_plan.build(model.structure(), m_state.ext->structure());
  size_state(m_state, m_plan.plan, m_plan.plan.n_p);
  m_compile_seconds = seconds_since(t0);
}

Sensitivity::~Sensitivity() = default;

// Both systems at the iterate, unit scales, the user's units: V' and V swept, M and R written, the model's lhs
// assembled (and a right-hand side of its own built: the factorization carries one along).
void Sensitivity::evaluate(const Point& at) {
  if (m_evaluated) return;
  const SensPlan& p = m_plan.plan;
  const size_t n = p.n, n_p = p.n_p, m_e = p.m_e, m_i = p.m_i;
  if (at.x->size() != n || at.s->size() != m_i || at.y->size() != m_e || at.z->size() != m_i || at.parameters->size() != n_p)
    throw std::runtime_error("slpx: sensitivity: the iterate does not have the model's sizes");
  DeviceNlp& dev = m_model.device();
  DeviceNlp& ext = m_state.ext->device();
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
  gather(m_plan, m_state, dev, st);
  dev.assemble();
  dev.build_rhs();
  // (what is in memory IS the system now: a request the last solve left for a step that never came is void)
  dev.system_written_by_caller(/*lhs=*/true, /*rhs=*/true);
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (`at` is the caller's)
  m_evaluated = true;
}

// The lhs evaluate() left, factored from a cleared memory; the inertia is read back, the caller's scaling is put back
// afterwards, and a system that cannot be factored throws.
void Sensitivity::factor(const Point& at, SensitivityInfo& info) {
  evaluate(at);
  if (!m_factored) {
    const auto t0 = clk::now();
    DeviceNlp& dev = m_model.device();
    const Factored fac = factor_from_cleared_memory(m_model, nullptr);
    m_delta = fac.delta[0];
    m_gamma = fac.gamma[0];
    info.factorizations += fac.factorizations;
    std::vector<LdltStats> stats;
    dev.ldlt().read_stats(stats);
    m_n_pos = stats[0].n_pos;
    m_n_neg = stats[0].n_neg;
    m_n_zero = stats[0].n_zero;
    // (V of the model system is its own copy here; the lhs in memory stays the one that was factored)
    if (at.scales_after != nullptr && static_cast<int>(at.scales_after->size()) == m_model.structure().n_scales())
      dev.set_scaling(*at.scales_after);
    if (fac.result[0] != FactorInfo::Success)
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

void Sensitivity::jacobian(const Point& at, double* dx, double* ds, double* dy, double* dz, SensitivityInfo& info) {
  const auto t0 = clk::now();
  const SensPlan& p = m_plan.plan;
  SensState& S = m_state;
  info.n_p = p.n_p;
  info.t_compile = take_compile_seconds();
  factor(at, info);
  const size_t pitch = static_cast<size_t>(p.n_p) * p.dim;
  for (int q = 0; q < p.n_p; ++q)
    solve_round(m_model, p.dim, S.R.p + static_cast<size_t>(q) * p.dim, pitch, S.sol.p + static_cast<size_t>(q) * p.dim, pitch, nullptr, &info);
  expand_and_download(m_plan, S, p.n_p, S.M.p + p.dim, p.dimM, static_cast<long long>(p.n_p) * p.dimM, dx, ds, dy, dz, m_model.device().stream());
  info.t_total = seconds_since(t0) + info.t_compile;
}

void Sensitivity::jvp(const Point& at, const double* dp, double* dx, double* ds, double* dy, double* dz, SensitivityInfo& info) {
  const auto t0 = clk::now();
  const SensPlan& p = m_plan.plan;
  SensState& S = m_state;
  if (dp == nullptr) throw std::runtime_error("slpx: sensitivity jvp: dp is null");
  info.n_p = p.n_p;
  info.t_compile = take_compile_seconds();
  factor(at, info);
  const hipStream_t st = m_model.device().stream();
  combine(m_plan, S, dp, st);
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (dp is the caller's)
  solve_round(m_model, p.dim, S.rhs1.p, p.dim, S.sol.p, p.dim, nullptr, &info);
  expand_and_download(m_plan, S, 1, S.ri1.p, 0, p.m_i, dx, ds, dy, dz, st);
  info.t_total = seconds_since(t0) + info.t_compile;
}

void Sensitivity::vjp(const Point& at, const double* vx, double* grad, SensitivityInfo& info) {
  if (vx == nullptr) throw std::runtime_error("slpx: sensitivity vjp: vx is null");
  SensCotangent v;
  v.vx = vx;
  vjp_full(at, v, grad, info);
}

void Sensitivity::vjp_full(const Point& at, const SensCotangent& given, double* grad, SensitivityInfo& info) {
  const auto t0 = clk::now();
  if (!given.vx && !given.vs && !given.vy && !given.vz && !given.vcost) throw std::runtime_error("slpx: sensitivity vjp: no cotangent");
  const SensPlan& p = m_plan.plan;
  SensState& S = m_state;
  info.n_p = p.n_p;
  info.t_compile = take_compile_seconds();
  factor(at, info);
  const hipStream_t st = m_model.device().stream();
  SensExtraRows extras[5];
  cotangent_arrays(given, p.n, p.m_e, p.m_i, extras);
  std::vector<double> packed;
  std::vector<size_t> packed_at;
  pack_rows(1, extras, 5, packed, packed_at);
  const SensCotangent v = adjoint_rhs(m_plan, S, extras, packed, packed_at, st);
  solve_round(m_model, p.dim, S.rhs1.p, p.dim, S.sol.p, p.dim, nullptr, &info);
  vjp_reduce(m_plan, S, v, grad, st);
  info.t_total = seconds_since(t0) + info.t_compile;
}

void Sensitivity::unreduced(const Point& at, double* M) {
  evaluate(at);
  // (evaluate() installed unit scales on the model system: the caller's back, as after a factorization)
  if (at.scales_after != nullptr && static_cast<int>(at.scales_after->size()) == m_model.structure().n_scales() && !m_factored)
    m_model.device().set_scaling(*at.scales_after);
  if (M) m_model.device().download(m_state.M.p, M, static_cast<size_t>(m_plan.plan.n_p) * m_plan.plan.dimM);
}

// ---- B instances at once ----

// One call's bookkeeping.  status: the outcome of every instance IN THIS CALL — that of its rows (PerBatch::base_status),
// or skipped for a dp / cotangent that is not finite; mask: the instances the solves of this call are for.
struct BatchSensitivity::Call {
  PerBatch* pb = nullptr;
  NewtonSystem* model = nullptr;
  Rows at;
  clk::time_point t0;
  std::vector<int32_t> status;
  std::vector<uint8_t> extra_bad, mask;
  std::vector<SensitivityInfo> info;
  std::vector<double> extra;  // dp / the cotangents behind one another (pack_rows), zeros in the rows of the instances left out: no kernel reads a NaN
  std::vector<size_t> extra_at;  // where each of them begins in `extra`
  double t_compile = 0.0, t_factor = 0.0;
  int factorizations = 0;

  void settle() {
    const int B = pb->state.B;
    bool any = false;
    for (int b = 0; b < B; ++b) {
      status[b] = pb->base_status[b] != kSensComputed ? pb->base_status[b] : extra_bad[b] ? kSensSkipped : kSensComputed;
      mask[b] = status[b] == kSensComputed ? 1 : 0;
      any = any || mask[b];
    }
    any_computed = any;
  }
  bool any_computed = false;
};

void BatchSensitivity::forget(int batch) {
  const auto it = m_per_batch.find(batch);
  if (it != m_per_batch.end()) it->second.evaluated = it->second.factored = false;
}
void BatchSensitivity::forget_all() {
  for (auto& [batch, pb] : m_per_batch) pb.evaluated = pb.factored = false;
}

// The state of this batch size (its extended system is made on the first call for it) and, on the very first call, the plan.
BatchSensitivity::PerBatch& BatchSensitivity::per_batch(NewtonSystem& model, NodeId f) {
  const int B = model.batch();
  PerBatch& pb = m_per_batch[B];
  if (pb.state.ext) return pb;
  const auto t0 = clk::now();
  if (!model.has_device()) throw std::runtime_error("slpx: batched sensitivity: no HIP device");
  if (model.structure().parameter_nodes().empty()) throw std::runtime_error("slpx: batched sensitivity: the model reaches no parameter");
  auto ext = extended_system(model, f, B);
  if (!m_plan.built) m_plan.build(model.structure(), ext->structure());
  const SensPlan& p = m_plan.plan;
  if (ext->structure().nV != p.nVx || model.structure().nV != p.nV || model.kkt().dim != p.dim)
    throw std::runtime_error("slpx: batched sensitivity: the batch system does not belong to the plan");
  pb.state.B = B;
  pb.state.threads = kSensBatchThreads;
  pb.state.ext = std::move(ext);
  pb.base_status.assign(static_cast<size_t>(B), kSensSkipped);
  pb.fact.assign(static_cast<size_t>(B), SensitivityInfo{});
  pb.compile_seconds = seconds_since(t0);
  return pb;
}

// The checks every call makes, room for `columns` solutions per instance, the classification of its instances, and
// whether what the last call of this batch size left in memory is still the system of these rows.
void BatchSensitivity::begin(Call& c, NewtonSystem& model, NodeId f, const Rows& at, const SensExtraRows* extras, int n_extras, int columns) {
  c.t0 = clk::now();
  c.model = &model;
  c.at = at;
  const int B = at.B;
  if (B <= 0 || B > 65535) throw std::runtime_error("slpx: batched sensitivity: B must be in 1 .. 65535 (one grid slice per instance)");
  if (model.batch() != B) throw std::runtime_error("slpx: batched sensitivity: the batch system is of another size");
  PerBatch& pb = per_batch(model, f);
  c.pb = &pb;
  c.t_compile = pb.compile_seconds;
  pb.compile_seconds = 0.0;
  const SensPlan& p = m_plan.plan;
  if (at.x == nullptr || at.mu == nullptr || at.params == nullptr || (p.m_i && (at.s == nullptr || at.z == nullptr)) ||
      (p.m_e && at.y == nullptr))
    throw std::runtime_error("slpx: batched sensitivity: a required input is null");
  size_state(pb.state, p, columns);
  const size_t Bz = static_cast<size_t>(B);
  // the rows as one vector: what the kept factorization is the factorization OF
  std::vector<double> key;
  key.reserve(Bz * (p.n + 2 * p.m_i + p.m_e + 1 + p.n_p));
  key.insert(key.end(), at.x, at.x + Bz * p.n);
  if (p.m_i) key.insert(key.end(), at.s, at.s + Bz * p.m_i);
  if (p.m_e) key.insert(key.end(), at.y, at.y + Bz * p.m_e);
  if (p.m_i) key.insert(key.end(), at.z, at.z + Bz * p.m_i);
  key.insert(key.end(), at.mu, at.mu + Bz);
  key.insert(key.end(), at.params, at.params + Bz * p.n_p);
  const bool same = pb.evaluated && key.size() == pb.key.size() && std::memcmp(key.data(), pb.key.data(), key.size() * sizeof(double)) == 0;
  if (!same) {
    pb.evaluated = pb.factored = false;
    pb.key = std::move(key);
    sens_classify_instances(B, p.n, p.m_e, p.m_i, p.n_p, at.x, at.s, at.y, at.z, at.mu, at.params, nullptr, 0, pb.base_status.data());
    pb.fact.assign(Bz, SensitivityInfo{});
  }
  c.status.assign(Bz, kSensComputed);
  c.extra_bad.assign(Bz, 0);
  c.mask.assign(Bz, 0);
  c.info.assign(Bz, SensitivityInfo{});
  if (n_extras > 0) {
    std::vector<int32_t> st(Bz);
    sens_classify_extras(B, extras, n_extras, st.data());
    pack_rows(B, extras, n_extras, c.extra, c.extra_at);
    for (size_t b = 0; b < Bz; ++b)
      if (st[b] != kSensComputed) {
        c.extra_bad[b] = 1;
        for (int k = 0; k < n_extras; ++k)
          if (extras[k].rows != nullptr)
            std::fill_n(c.extra.begin() + c.extra_at[k] + b * extras[k].width, extras[k].width, 0.0);
      }
  }
  c.settle();
}

// Both batch systems at the rows, unit scales, the user's units: V' and V swept, M and R written, the model's lhs
// assembled (and a right-hand side of its own built: the factorization carries one along).  An instance that is left
// out stands in with the rows of the first one that is not: nothing reads a NaN, and nobody reads its results.
void BatchSensitivity::evaluate(Call& c) {
  PerBatch& pb = *c.pb;
  if (pb.evaluated) return;
  const SensPlan& p = m_plan.plan;
  const Rows& at = c.at;
  const size_t B = static_cast<size_t>(pb.state.B), n = p.n, n_p = p.n_p, m_e = p.m_e, m_i = p.m_i;
  pb.factored = false;
  size_t h = B;
  for (size_t b = 0; b < B && h == B; ++b)
    if (pb.base_status[b] == kSensComputed) h = b;
  if (h == B) {  // (nothing to differentiate: every output row is NaN)
    pb.evaluated = true;
    return;
  }
  std::vector<double> xp(B * (n + n_p)), x(B * n), s(B * std::max<size_t>(1, m_i), 1.0), y(B * std::max<size_t>(1, m_e), 0.0),
      z(B * std::max<size_t>(1, m_i), 1.0), mu(B), rows(B * n_p);
  for (size_t b = 0; b < B; ++b) {
    const size_t from = pb.base_status[b] == kSensComputed ? b : h;
    std::copy(at.x + from * n, at.x + (from + 1) * n, x.begin() + b * n);
    std::copy(at.x + from * n, at.x + (from + 1) * n, xp.begin() + b * (n + n_p));
    std::copy(at.params + from * n_p, at.params + (from + 1) * n_p, xp.begin() + b * (n + n_p) + n);
    std::copy(at.params + from * n_p, at.params + (from + 1) * n_p, rows.begin() + b * n_p);
    if (m_i) {
      std::copy(at.s + from * m_i, at.s + (from + 1) * m_i, s.begin() + b * m_i);
      std::copy(at.z + from * m_i, at.z + (from + 1) * m_i, z.begin() + b * m_i);
    }
    if (m_e) std::copy(at.y + from * m_e, at.y + (from + 1) * m_e, y.begin() + b * m_e);
    mu[b] = at.mu[from];
  }
  DeviceNlp& dev = c.model->device();
  DeviceNlp& ext = pb.state.ext->device();
  ext.upload_x(xp.data());
  ext.upload_duals(s.data(), y.data(), z.data());
  ext.sweep_full();
  SLPX_HIP_CHECK(hipStreamSynchronize(ext.stream()));  // (the two systems may run on different streams)
  // instance b's parameter row in a pool of its own on the model's batch system for the sweep; however this ends, the
  // shared pool with the parameters' current values is in force again
  struct SharedPoolAgain {
    NewtonSystem* sys;
    void now() {
      NewtonSystem* s = sys;
      sys = nullptr;
      if (s != nullptr) s->device().refresh_params(s->graph());
    }
    ~SharedPoolAgain() {
      try {
        now();
      } catch (...) {
      }
    }
  } shared_pool_again{c.model};
  dev.set_parameters(rows.data(), /*per_instance=*/true);
  dev.upload_x(x.data());
  dev.upload_duals(s.data(), y.data(), z.data());
  dev.upload_mu(mu.data());
  dev.sweep_full();
  const hipStream_t st = dev.stream();
  gather(m_plan, pb.state, dev, st);
  dev.assemble();
  dev.build_rhs();
  // (what is in memory IS the system now — a request for a step that never came is void; assemble() and build_rhs()
  // said themselves which layout they wrote)
  dev.system_written_by_caller(/*lhs=*/false, /*rhs=*/false);
  SLPX_HIP_CHECK(hipStreamSynchronize(st));  // (the rows are this function's)
  shared_pool_again.now();
  pb.evaluated = true;
}

// The instances that are differentiated, factored from a cleared memory.  An instance whose system cannot be factored
// leaves the call here (kSensNotFactored); one that can reports the accepted inertia.
void BatchSensitivity::factor(Call& c) {
  evaluate(c);
  PerBatch& pb = *c.pb;
  const int B = pb.state.B;
  if (!pb.factored) {
    const auto t0 = clk::now();
    std::vector<uint8_t> mask(B, 0);
    bool any = false;
    for (int b = 0; b < B; ++b) any = (mask[b] = pb.base_status[b] == kSensComputed ? 1 : 0) || any;
    if (any) {
      const Factored fac = factor_from_cleared_memory(*c.model, &mask);
      c.factorizations = fac.factorizations;
      std::vector<LdltStats> stats;
      c.model->device().ldlt().read_stats(stats);
      for (int b = 0; b < B; ++b) {
        if (!mask[b]) continue;
        SensitivityInfo& fi = pb.fact[b];
        fi.delta = fac.delta[b];
        fi.gamma = fac.gamma[b];
        if (fac.result[b] == FactorInfo::Success) {
          // (the counters in memory are those of the LAST launch, which an instance accepted earlier sat out: what the
          // policy accepts has the ideal inertia and nothing else, ldlt_policy.hpp: ldlt_judge)
          fi.n_pos = m_plan.plan.n;
          fi.n_neg = m_plan.plan.m_e;
          fi.n_zero = 0;
        } else {  // (gave up in the last launch it took part in; the counters as they stand)
          fi.n_pos = stats[b].n_pos;
          fi.n_neg = stats[b].n_neg;
          fi.n_zero = stats[b].n_zero;
          pb.base_status[b] = kSensNotFactored;
        }
      }
    }
    pb.factored = true;
    c.t_factor = seconds_since(t0);
  }
  c.settle();
  for (int b = 0; b < B; ++b) {
    if (pb.base_status[b] == kSensSkipped) continue;
    c.info[b] = pb.fact[b];
    c.info[b].factorizations = c.factorizations;
  }
}

namespace {
// rows of `width` entries, one per (instance, column): NaN where the instance was not computed
void nan_rows(double* out, const std::vector<int32_t>& status, size_t per_instance) {
  if (out == nullptr || per_instance == 0) return;
  for (size_t b = 0; b < status.size(); ++b)
    if (status[b] != kSensComputed) std::fill(out + b * per_instance, out + (b + 1) * per_instance, std::numeric_limits<double>::quiet_NaN());
}
}  // namespace

// the expansion for the instances that were computed, NaN rows for the others
void BatchSensitivity::expand(Call& c, int columns, const double* r_i, long long r_i_column, long long r_i_instance, double* dx, double* ds,
                              double* dy, double* dz) {
  const SensPlan& p = m_plan.plan;
  if (c.any_computed)
    expand_and_download(m_plan, c.pb->state, columns, r_i, r_i_column, r_i_instance, dx, ds, dy, dz, c.model->device().stream());
  nan_rows(dx, c.status, static_cast<size_t>(columns) * p.n);
  nan_rows(ds, c.status, static_cast<size_t>(columns) * p.m_i);
  nan_rows(dy, c.status, static_cast<size_t>(columns) * p.m_e);
  nan_rows(dz, c.status, static_cast<size_t>(columns) * p.m_i);
}

void BatchSensitivity::finish(Call& c, int32_t* status, SensitivityInfo* info) {
  const double t_total = seconds_since(c.t0) + c.t_compile;
  if (status) std::copy(c.status.begin(), c.status.end(), status);
  if (info == nullptr) return;
  for (int b = 0; b < c.pb->state.B; ++b) {
    info[b] = c.info[b];
    info[b].n_p = m_plan.plan.n_p;
    info[b].solve_status = 0;  // (the call is not told it)
    info[b].t_compile = c.t_compile;
    info[b].t_factor = c.t_factor;
    info[b].t_total = t_total;
  }
}

void BatchSensitivity::jacobian(NewtonSystem& model, NodeId f, const Rows& at, double* dx, double* ds, double* dy, double* dz,
                                int32_t* status, SensitivityInfo* info) {
  Call c;
  begin(c, model, f, at, nullptr, 0, static_cast<int>(model.structure().parameter_nodes().size()));
  const SensPlan& p = m_plan.plan;
  SensState& S = c.pb->state;
  factor(c);
  // round q: column q of every instance
  const size_t pitch = static_cast<size_t>(p.n_p) * p.dim;
  for (int q = 0; q < p.n_p && c.any_computed; ++q)
    solve_round(model, p.dim, S.R.p + static_cast<size_t>(q) * p.dim, pitch, S.sol.p + static_cast<size_t>(q) * p.dim, pitch, &c.mask, c.info.data());
  expand(c, p.n_p, S.M.p + p.dim, p.dimM, static_cast<long long>(p.n_p) * p.dimM, dx, ds, dy, dz);
  finish(c, status, info);
}

void BatchSensitivity::jvp(NewtonSystem& model, NodeId f, const Rows& at, const double* dp, double* dx, double* ds, double* dy,
                           double* dz, int32_t* status, SensitivityInfo* info) {
  if (dp == nullptr) throw std::runtime_error("slpx: batched sensitivity jvp: dp is null");
  Call c;
  const SensExtraRows extra{dp, static_cast<int>(model.structure().parameter_nodes().size())};
  begin(c, model, f, at, &extra, 1, 1);
  const SensPlan& p = m_plan.plan;
  SensState& S = c.pb->state;
  factor(c);
  if (c.any_computed) {
    combine(m_plan, S, c.extra.data(), model.device().stream());
    solve_round(model, p.dim, S.rhs1.p, p.dim, S.sol.p, p.dim, &c.mask, c.info.data());
  }
  expand(c, 1, S.ri1.p, 0, p.m_i, dx, ds, dy, dz);
  finish(c, status, info);
}

void BatchSensitivity::vjp(NewtonSystem& model, NodeId f, const Rows& at, const double* vx, double* grad, int32_t* status,
                           SensitivityInfo* info) {
  if (vx == nullptr) throw std::runtime_error("slpx: batched sensitivity vjp: vx is null");
  SensCotangent v;
  v.vx = vx;
  vjp_full(model, f, at, v, grad, status, info);
}

void BatchSensitivity::vjp_full(NewtonSystem& model, NodeId f, const Rows& at, const SensCotangent& given, double* grad, int32_t* status,
                                SensitivityInfo* info) {
  if (!given.vx && !given.vs && !given.vy && !given.vz && !given.vcost) throw std::runtime_error("slpx: batched sensitivity vjp: no cotangent");
  const NlpStructure& ms = model.structure();
  SensExtraRows extras[5];
  cotangent_arrays(given, ms.n, ms.m_e, ms.m_i, extras);
  Call c;
  begin(c, model, f, at, extras, 5, 1);
  const SensPlan& p = m_plan.plan;
  SensState& S = c.pb->state;
  factor(c);
  if (c.any_computed) {
    const hipStream_t st = model.device().stream();
    const SensCotangent v = adjoint_rhs(m_plan, S, extras, c.extra, c.extra_at, st);
    solve_round(model, p.dim, S.rhs1.p, p.dim, S.sol.p, p.dim, &c.mask, c.info.data());
    vjp_reduce(m_plan, S, v, grad, st);
  }
  nan_rows(grad, c.status, p.n_p);
  finish(c, status, info);
}

void BatchSensitivity::unreduced(NewtonSystem& model, NodeId f, const Rows& at, double* M, int32_t* status) {
  Call c;
  begin(c, model, f, at, nullptr, 0, 0);
  evaluate(c);
  const size_t per_instance = static_cast<size_t>(m_plan.plan.n_p) * m_plan.plan.dimM;
  // (an instance a kept factorization found singular still has its M: only what was skipped has none)
  std::vector<int32_t> st(c.status);
  bool any = false;
  for (size_t b = 0; b < st.size(); ++b) any = (st[b] = c.pb->base_status[b] == kSensSkipped ? kSensSkipped : kSensComputed) == kSensComputed || any;
  if (M && any) model.device().download(c.pb->state.M.p, M, static_cast<size_t>(c.pb->state.B) * per_instance);
  nan_rows(M, st, per_instance);
  if (status) std::copy(st.begin(), st.end(), status);
}

}  // namespace slpx
