// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// A probe of slpx::BatchFrDevice (fr_batch.hpp): plain C entry points that drive the REAL launch wrappers of libslpx.so
// (fr_batch_launch.hip) one at a time on the NewtonSystem behind an slpx_system handle — the batch system that
// slpx_system_create(problem, B, 0) makes, tape at unit scales — and get / put on every per-instance buffer those kernels
// read or write, the device struct's own and the batch system's.  Nothing of the kernels is compiled here.
// tests/test_restoration_batch_kernels_gpu.py compares what comes back with tests/support/fr_reference.py.
#include "../../sleipnir_amd/csrc/fr_batch.hpp"
#include "probe_common.hpp"

namespace slpx {

struct BatchFrProbe {
  static constexpr const char* kName = "frbatchcheck";
  explicit BatchFrProbe(NewtonSystem& s) : sys(s), bd(s) {}
  NewtonSystem& sys;
  BatchFrDevice bd;

  // the buffers fbc_get / fbc_put reach: device pointer and length (doubles)
  std::pair<double*, size_t> buffer(int which) {
    DeviceNlp& dev = sys.device();
    const size_t B = bd.B, n = bd.n, m_e = bd.m_e, m_i = bd.m_i, dim = bd.dim, nV = bd.nV, M = bd.M, nnz = bd.nnz;
    const size_t nin = sys.structure().n_inputs();
    switch (which) {
      case 0: return {bd.m_x.p, B * n};
      case 1: return {bd.m_s0.p, B * m_i};
      case 2: return {bd.m_y.p, B * m_e};
      case 3: return {bd.m_z0.p, B * m_i};
      case 4: return {bd.m_xr.p, B * n};
      case 5: return {bd.m_w.p, B * n};
      case 6: return {bd.m_g_outer.p, B * n};
      case 7: return {bd.m_s_outer.p, B * m_i};
      case 8: return {bd.m_pn.p, B * M};
      case 9: return {bd.m_sxx.p, B * M};
      case 10: return {bd.m_zx.p, B * M};
      case 11: return {bd.m_p.p, B * dim};
      case 12: return {bd.m_ps0.p, B * m_i};
      case 13: return {bd.m_pz0.p, B * m_i};
      case 14: return {bd.m_dpn.p, B * M};
      case 15: return {bd.m_psx.p, B * M};
      case 16: return {bd.m_pzx.p, B * M};
      case 17: return {bd.m_soc_ce.p, B * m_e};
      case 18: return {bd.m_soc_c0.p, B * m_i};
      case 19: return {bd.m_soc_x.p, B * M};
      case 20: return {bd.m_keep_p.p, B * dim};
      case 21: return {bd.m_keep_ps0.p, B * m_i};
      case 22: return {bd.m_keep_pz0.p, B * m_i};
      case 23: return {bd.m_keep_dpn.p, B * M};
      case 24: return {bd.m_keep_psx.p, B * M};
      case 25: return {bd.m_keep_pzx.p, B * M};
      case 26: return {bd.m_Vcur.p, B * nV};
      case 27: return {bd.m_fr_out.p, B * static_cast<size_t>(kFrBatchErrN)};
      case 28: return {bd.m_vt.p, B * static_cast<size_t>(sys.structure().off_g)};
      case 29: return {dev.d_V(), B * nV};       // the batch system's V (the last sweep's, scaled)
      case 30: return {dev.d_x(), B * nin};      // ... its tape input
      case 31: return {dev.lhs_raw(), B * nnz};  // ... its batch-major lhs / rhs as build() writes them
      case 32: return {dev.rhs_raw(), B * dim};
      case 33: return {dev.d_p(), B * dim};      // ... its solution
      default: throw std::runtime_error("frbatchcheck: bad buffer selector");
    }
  }
};

}  // namespace slpx

using slpx::BatchFrProbe;

using namespace probe;

namespace {

// one launch wrapper, then the stream drained
template <class Call>
int launch(BatchFrProbe* h, Call&& call) {
  return guard([&] {
    check(h);
    call(h->bd);
    sync(h);
  });
}

}  // namespace

extern "C" {

const char* fbc_last_error() { return g_error.c_str(); }

BatchFrProbe* fbc_create(slpx_system* s) { return create<BatchFrProbe>(s); }

void fbc_destroy(BatchFrProbe* h) { delete h; }

// B, n, m_e, m_i, dim, ns, nV, nnz of the lhs, M = 2 m_e + 2 m_i, length of the tape input, doubles of an instance's errors
int fbc_dims(BatchFrProbe* h, int64_t* out) {
  return guard([&] {
    check(h);
    const auto& bd = h->bd;
    const int64_t v[11] = {bd.B, bd.n, bd.m_e, bd.m_i, bd.dim, bd.ns, bd.nV, bd.nnz, bd.M, h->sys.structure().n_inputs(), slpx::kFrBatchErrN};
    std::memcpy(out, v, sizeof(v));
  });
}

int fbc_set_scales(BatchFrProbe* h, const double* scales) {
  return guard([&] {
    check(h);
    h->bd.set_scales(vec(scales, static_cast<size_t>(h->bd.B) * h->bd.ns));
  });
}

int fbc_begin(BatchFrProbe* h, int b, const double* x, const double* s0, const double* y, const double* z0, const double* x_r, const double* w,
              const double* g_outer, const double* s_outer, const double* pn, const double* sx, const double* zx) {
  return launch(h, [&](slpx::BatchFrDevice& bd) { bd.begin(b, x, s0, y, z0, x_r, w, g_outer, s_outer, pn, sx, zx); });
}

// the per-instance parameters of the next launches, then upload()
int fbc_set_params(BatchFrProbe* h, const double* delta, const double* mu, const double* tau, const double* alpha, const double* alpha_soc,
                   const double* alpha_z, const double* mu_outer, const uint8_t* soc, const uint8_t* first, const uint8_t* rhs_only,
                   const uint8_t* active) {
  return guard([&] {
    check(h);
    auto& bd = h->bd;
    const size_t B = bd.B;
    bd.delta = vec(delta, B);
    bd.mu = vec(mu, B);
    bd.tau = vec(tau, B);
    bd.alpha = vec(alpha, B);
    bd.alpha_soc = vec(alpha_soc, B);
    bd.alpha_z = vec(alpha_z, B);
    bd.mu_outer = vec(mu_outer, B);
    bd.soc = vec(soc, B);
    bd.first = vec(first, B);
    bd.rhs_only = vec(rhs_only, B);
    bd.active = vec(active, B);
    bd.upload();
  });
}

int fbc_sweep(BatchFrProbe* h) {
  return launch(h, [](slpx::BatchFrDevice& bd) { bd.sweep(); });
}
int fbc_build(BatchFrProbe* h) {
  return launch(h, [](slpx::BatchFrDevice& bd) { bd.build(); });
}
int fbc_expand(BatchFrProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.expand(v); });
}
int fbc_trial_values(BatchFrProbe* h, int after_expand, double* out) {
  return scalars_out(h, out, [&](auto& bd, auto& v) { bd.trial_values(v, after_expand != 0); });
}
int fbc_soc_accumulate(BatchFrProbe* h) {
  return launch(h, [](slpx::BatchFrDevice& bd) { bd.soc_accumulate(); });
}
int fbc_save_direction(BatchFrProbe* h) {
  return launch(h, [](slpx::BatchFrDevice& bd) { bd.save_direction(); });
}
int fbc_restore_direction(BatchFrProbe* h) {
  return launch(h, [](slpx::BatchFrDevice& bd) { bd.restore_direction(); });
}
int fbc_commit(BatchFrProbe* h) { return commit(h); }
int fbc_errors(BatchFrProbe* h, int check_all_V, double* out) {
  return scalars_out(h, out, [&](auto& bd, auto& v) { bd.errors(check_all_V != 0, v); });
}
// the whole restoration iterate of instance b
int fbc_download_instance(BatchFrProbe* h, int b, double* x, double* s0, double* y, double* z0, double* pn, double* sx, double* zx) {
  return launch(h, [&](slpx::BatchFrDevice& bd) { bd.download_instance(b, x, s0, y, z0, pn, sx, zx); });
}

int64_t fbc_get(BatchFrProbe* h, int which, double* out) { return get(h, which, out); }
int fbc_put(BatchFrProbe* h, int which, const double* in) { return put(h, which, in); }

}  // extern "C"
