#include "sens_plan.hpp"

#include <stdexcept>
#include <string>
#include <utility>

#include "sens_rows.h"

namespace slpx {

SensPlan build_sens_plan(const NlpStructure& model, const NlpStructure& ext) {
  SensPlan p;
  p.n = model.n;
  p.m_e = model.m_e;
  p.m_i = model.m_i;
  p.n_p = ext.n - model.n;
  if (p.n_p <= 0) throw std::runtime_error("slpx: sensitivity plan: the extended structure has no parameter columns");
  if (ext.m_e != model.m_e || ext.m_i != model.m_i)
    throw std::runtime_error("slpx: sensitivity plan: the extended structure has other constraints than the model");
  for (const CscPattern* pat : {&ext.Ae, &ext.Ai, &ext.Hf, &ext.Hc})
    if (pat->cols != ext.n || static_cast<int>(pat->colptr.size()) != ext.n + 1)
      throw std::runtime_error("slpx: sensitivity plan: a pattern of the extended structure is not over n + n_p columns");
  p.dim = p.n + p.m_e;
  p.dimM = p.n + p.m_e + p.m_i;
  p.nV = model.nV;
  p.nVx = ext.nV;
  const int n = p.n, n_p = p.n_p, m_e = p.m_e, dimM = p.dimM;

  // every source of M, Hessians first (H_f' before H_c'), as f(key = q * dimM + row, position in V')
  auto for_each_source = [&](auto&& f) {
    using Block = std::pair<const CscPattern*, int>;
    for (const auto& [pat, off] : {Block{&ext.Hf, ext.off_Hf}, Block{&ext.Hc, ext.off_Hc}})
      for (int c = 0; c < n; ++c)  // (columns >= n: the p-p block, which no sensitivity reads)
        for (int32_t t = pat->colptr[c]; t < pat->colptr[c + 1]; ++t) {
          const int r = pat->rowidx[t];
          if (r < c) throw std::runtime_error("slpx: sensitivity plan: a Hessian entry above the diagonal");
          if (r >= n) f(static_cast<int64_t>(r - n) * dimM + c, off + t);
        }
    for (int q = 0; q < n_p; ++q) {
      for (int32_t t = ext.Ae.colptr[n + q]; t < ext.Ae.colptr[n + q + 1]; ++t)
        f(static_cast<int64_t>(q) * dimM + n + ext.Ae.rowidx[t], ext.off_Ae + t);
      for (int32_t t = ext.Ai.colptr[n + q]; t < ext.Ai.colptr[n + q + 1]; ++t)
        f(static_cast<int64_t>(q) * dimM + n + m_e + ext.Ai.rowidx[t], ext.off_Ai + t);
    }
  };
  const int64_t cells = static_cast<int64_t>(n_p) * dimM;
  if (cells >= (int64_t{1} << 31)) throw std::runtime_error("slpx: sensitivity plan: n_p (n + m_e + m_i) does not fit 31 bits");
  p.m_ptr.assign(static_cast<size_t>(cells) + 1, 0);
  for_each_source([&](int64_t key, int32_t) { ++p.m_ptr[key + 1]; });
  for (int64_t k = 0; k < cells; ++k) p.m_ptr[k + 1] += p.m_ptr[k];
  p.m_src.assign(static_cast<size_t>(p.m_ptr[cells]), -1);
  {
    std::vector<int32_t> next(p.m_ptr.begin(), p.m_ptr.end() - 1);
    for_each_source([&](int64_t key, int32_t src) { p.m_src[next[key]++] = src; });
  }

  // A_i of the model: by columns for the reduction (pattern order), by rows for the expansion (columns ascending)
  const CscPattern& Ai = model.Ai;
  p.red_ptr.assign(Ai.colptr.begin(), Ai.colptr.end());
  if (static_cast<int>(p.red_ptr.size()) != n + 1) throw std::runtime_error("slpx: sensitivity plan: A_i is not over n columns");
  p.red_src.resize(Ai.nnz());
  p.red_row.assign(Ai.rowidx.begin(), Ai.rowidx.end());
  for (int t = 0; t < Ai.nnz(); ++t) p.red_src[t] = model.off_Ai + t;
  p.ai_rowptr.assign(p.m_i + 1, 0);
  for (int32_t r : Ai.rowidx) ++p.ai_rowptr[r + 1];
  for (int j = 0; j < p.m_i; ++j) p.ai_rowptr[j + 1] += p.ai_rowptr[j];
  p.ai_col.resize(Ai.nnz());
  p.ai_src.resize(Ai.nnz());
  {
    std::vector<int32_t> next(p.ai_rowptr.begin(), p.ai_rowptr.end() - 1);
    for (int c = 0; c < n; ++c)
      for (int32_t t = Ai.colptr[c]; t < Ai.colptr[c + 1]; ++t) {
        const int32_t at = next[Ai.rowidx[t]]++;
        p.ai_col[at] = c;
        p.ai_src[at] = model.off_Ai + t;
      }
  }

  // the cost's gradient over x in V, and its parameter columns in V'
  const auto one_entry = [](const CscPattern& g, int col, int off) -> int32_t {
    const int32_t first = g.colptr[col], count = g.colptr[col + 1] - first;
    if (count > 1) throw std::runtime_error("slpx: sensitivity plan: a column of the cost's gradient has more than one entry");
    return count == 1 ? off + first : -1;
  };
  if (static_cast<int>(model.g_pat.colptr.size()) != n + 1 || static_cast<int>(ext.g_pat.colptr.size()) != ext.n + 1)
    throw std::runtime_error("slpx: sensitivity plan: the pattern of the cost's gradient is not over the variables");
  p.g_src.resize(n);
  p.fp_src.resize(n_p);
  for (int i = 0; i < n; ++i) p.g_src[i] = one_entry(model.g_pat, i, model.off_g);
  for (int q = 0; q < n_p; ++q) p.fp_src[q] = one_entry(ext.g_pat, n + q, ext.off_g);
  return p;
}

void sens_host_rhs(const SensPlan& p, const double* Vx, const double* V, const double* s, const double* z, double* M, double* R) {
  for (int q = 0; q < p.n_p; ++q)
    for (int row = 0; row < p.dimM; ++row) {
      const int64_t k = static_cast<int64_t>(q) * p.dimM + row;
      const double m = sens_m_entry(p.m_ptr.data(), p.m_src.data(), Vx, k);
      M[k] = m;
      if (row < p.dim)
        R[static_cast<int64_t>(q) * p.dim + row] =
            sens_reduced_entry(p.n, p.m_e, p.dimM, p.m_ptr.data(), p.m_src.data(), p.red_ptr.data(), p.red_src.data(),
                               p.red_row.data(), Vx, V, s, z, q, row, m);
    }
}

void sens_host_combine(const SensPlan& p, const double* M, const double* R, const double* dp, double* rhs, double* r_i) {
  for (int row = 0; row < p.dim; ++row) rhs[row] = sens_combine_entry(p.n_p, R, p.dim, 0, row, dp);
  for (int j = 0; j < p.m_i; ++j) r_i[j] = sens_combine_entry(p.n_p, M, p.dimM, p.n + p.m_e, j, dp);
}

void sens_host_expand(const SensPlan& p, const double* V, const double* s, const double* z, const double* sol, const double* r_i,
                      double* dx, double* ds, double* dy, double* dz) {
  for (int i = 0; i < p.n; ++i) dx[i] = sol[i];
  for (int j = 0; j < p.m_e; ++j) dy[j] = -sol[p.n + j];
  for (int j = 0; j < p.m_i; ++j) {
    ds[j] = sens_ds_entry(p.ai_rowptr.data(), p.ai_col.data(), p.ai_src.data(), V, sol, r_i, j);
    dz[j] = sens_dz_entry(s[j], z[j], ds[j]);
  }
}

void sens_host_vjp(const SensPlan& p, const double* R, const double* w, double* grad) {
  for (int q = 0; q < p.n_p; ++q) {
    double part[kSensVjpThreads];
    for (int t = 0; t < kSensVjpThreads; ++t) part[t] = sens_vjp_partial(p.dim, R + static_cast<int64_t>(q) * p.dim, w, t);
    for (int width = kSensVjpThreads / 2; width > 0; width >>= 1)
      for (int t = 0; t < width; ++t) part[t] = part[t] + part[t + width];
    grad[q] = part[0];
  }
}

void sens_host_adjoint_rhs(const SensPlan& p, const double* V, const double* s, const double* z, const SensCotangent& v, double* rhs) {
  for (int row = 0; row < p.dim; ++row)
    rhs[row] = sens_adjoint_rhs_entry(p.n, p.red_ptr.data(), p.red_src.data(), p.red_row.data(), p.g_src.data(), V, s, z, v.vx, v.vs, v.vy,
                                      v.vz, v.vcost, row);
}

void sens_host_vjp_full(const SensPlan& p, const double* Vx, const double* M, const double* R, const double* s, const double* z,
                        const double* w, const SensCotangent& v, double* grad) {
  const auto fold = [](double* part) {
    for (int width = kSensVjpThreads / 2; width > 0; width >>= 1)
      for (int t = 0; t < width; ++t) part[t] = part[t] + part[t + width];
    return part[0];
  };
  const bool direct = sens_adjoint_has_t(p.m_i, v.vs, v.vz);
  for (int q = 0; q < p.n_p; ++q) {
    double part[kSensVjpThreads], part_t[kSensVjpThreads];
    for (int t = 0; t < kSensVjpThreads; ++t) part[t] = sens_vjp_partial(p.dim, R + static_cast<int64_t>(q) * p.dim, w, t);
    const double wR = fold(part);
    double tr = 0.0;
    if (direct) {
      const double* r_i = M + static_cast<int64_t>(q) * p.dimM + p.dim;
      for (int t = 0; t < kSensVjpThreads; ++t) part_t[t] = sens_adjoint_direct_partial(p.m_i, r_i, s, z, v.vs, v.vz, t);
      tr = fold(part_t);
    }
    grad[q] = sens_vjp_full_sum(wR, direct, tr, v.vcost, p.fp_src[q], Vx);
  }
}

void sens_classify_extras(int B, const SensExtraRows* extras, int count, int32_t* status) {
  for (int b = 0; b < B; ++b) {
    bool ok = true;
    for (int k = 0; k < count && ok; ++k) {
      if (extras[k].rows == nullptr) continue;
      const double* row = extras[k].rows + static_cast<int64_t>(b) * extras[k].width;
      for (int i = 0; i < extras[k].width; ++i)
        if (!(row[i] - row[i] == 0.0)) ok = false;
    }
    status[b] = ok ? kSensComputed : kSensSkipped;
  }
}

void sens_classify_instances(int B, int n, int m_e, int m_i, int n_p, const double* x, const double* s, const double* y,
                             const double* z, const double* mu, const double* params, const double* extra, int n_extra,
                             int32_t* status) {
  // (x - x is 0 for a finite x and NaN for a NaN or an Inf)
  const auto finite_row = [](const double* a, int b, int count) {
    if (a == nullptr) return true;
    const double* row = a + static_cast<int64_t>(b) * count;
    for (int i = 0; i < count; ++i)
      if (!(row[i] - row[i] == 0.0)) return false;
    return true;
  };
  for (int b = 0; b < B; ++b) {
    bool ok = finite_row(x, b, n) && finite_row(s, b, m_i) && finite_row(y, b, m_e) && finite_row(z, b, m_i) && finite_row(mu, b, 1) &&
              finite_row(params, b, n_p) && finite_row(extra, b, n_extra);
    if (ok && s != nullptr)
      for (int j = 0; j < m_i; ++j)
        if (!(s[static_cast<int64_t>(b) * m_i + j] > 0.0)) ok = false;
    status[b] = ok ? kSensComputed : kSensSkipped;
  }
}

}  // namespace slpx
