// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// A probe of slpx::BatchEqDevice (eq_batch.hpp), as batchcheck.cpp is of BatchIpmDevice: plain C entry points that
// drive the REAL launch wrappers of libslpx.so on the NewtonSystem behind an slpx_system handle (the batch system
// slpx_system_create(problem, B, 0) makes, tape at unit scales) and read back every per-instance buffer.  Nothing of
// the kernels is compiled here.  tests/test_eq_batch_kernels_gpu.py compares what comes back with numpy.
#include "../../sleipnir_amd/csrc/eq_batch.hpp"
#include "probe_common.hpp"

namespace slpx {

struct BatchEqProbe {
  static constexpr const char* kName = "eqbatchcheck";
  explicit BatchEqProbe(NewtonSystem& s) : sys(s), bd(s) {}
  NewtonSystem& sys;
  BatchEqDevice bd;

  // the buffers ebc_get / ebc_put reach: device pointer and length (doubles)
  std::pair<double*, size_t> buffer(int which) {
    DeviceNlp& dev = sys.device();
    const size_t B = bd.B, n = bd.n, m_e = bd.m_e, dim = bd.dim, nV = bd.nV;
    switch (which) {
      case 0: return {bd.m_x.p, B * n};
      case 1: return {bd.m_y.p, B * m_e};
      case 2: return {bd.m_tx.p, B * n};
      case 3: return {bd.m_ty.p, B * m_e};
      case 4: return {bd.m_px.p, B * n};
      case 5: return {bd.m_py.p, B * m_e};
      case 6: return {bd.m_sx.p, B * n};
      case 7: return {bd.m_sy.p, B * m_e};
      case 8: return {bd.m_Vcur.p, B * nV};
      case 9: return {bd.m_tce.p, B * m_e};
      case 10: return {bd.m_sce.p, B * m_e};
      case 11: return {bd.m_out.p, B * kBatchErrN};
      case 12: return {dev.d_V(), B * nV};     // the system's V (the last sweep's, scaled)
      case 13: return {dev.d_rhs(), B * dim};  // the system's rhs
      case 14: return {dev.d_p(), B * dim};    // the system's solution
      case 15: return {dev.d_y(), B * m_e};    // the system's y (what build_rhs reads)
      case 16: return {dev.d_x(), B * static_cast<size_t>(sys.structure().n_inputs())};  // the tape's inputs
      default: throw std::runtime_error("eqbatchcheck: bad buffer selector");
    }
  }
};

}  // namespace slpx

using slpx::BatchEqProbe;

using namespace probe;

extern "C" {

const char* ebc_last_error() { return g_error.c_str(); }

BatchEqProbe* ebc_create(slpx_system* s) { return create<BatchEqProbe>(s); }

void ebc_destroy(BatchEqProbe* h) { delete h; }

// B, n, m_e, dim, ns, nV, n_inputs
int ebc_dims(BatchEqProbe* h, int64_t* out) {
  return guard([&] {
    check(h);
    const auto& bd = h->bd;
    const int64_t v[7] = {bd.B, bd.n, bd.m_e, bd.dim, bd.ns, bd.nV, h->sys.structure().n_inputs()};
    std::memcpy(out, v, sizeof(v));
  });
}

int ebc_set_scales(BatchEqProbe* h, const double* scales) {
  return guard([&] {
    check(h);
    h->bd.set_scales(vec(scales, static_cast<size_t>(h->bd.B) * h->bd.ns));
  });
}

int ebc_set_iterate(BatchEqProbe* h, const double* x, const double* y) {
  return guard([&] {
    check(h);
    const size_t B = h->bd.B;
    h->bd.set_iterate(vec(x, B * h->bd.n), vec(y, B * h->bd.m_e));
  });
}

// the per-instance parameters of the next launches, then upload()
int ebc_set_params(BatchEqProbe* h, const double* alpha, const double* alpha_soc, const int32_t* mode, const uint8_t* first,
                   const uint8_t* active) {
  return guard([&] {
    check(h);
    auto& bd = h->bd;
    const size_t B = bd.B;
    bd.alpha = vec(alpha, B);
    bd.alpha_soc = vec(alpha_soc, B);
    bd.mode = vec(mode, B);
    bd.first = vec(first, B);
    bd.active = vec(active, B);
    bd.upload();
  });
}

// the Newton system of the refreshed iterate as the drivers build and solve it (mu = 0, masked compute); info [B]
int ebc_newton_step(BatchEqProbe* h, int32_t* info) {
  return guard([&] {
    check(h);
    slpx::DeviceNlp& dev = h->sys.device();
    const std::vector<double> mu0(h->bd.B, 0.0);
    h->sys.reset_regularization();
    h->sys.set_gamma_min(1e-10);
    dev.upload_mu(mu0.data());
    dev.assemble();
    dev.build_rhs();
    const auto r = h->sys.compute(true, h->bd.active);
    for (size_t b = 0; b < r.size(); ++b) info[b] = static_cast<int32_t>(r[b]);
    sync(h);
  });
}

int ebc_refresh(BatchEqProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.refresh(v); });
}
int ebc_direction(BatchEqProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.direction(v); });
}
int ebc_trial_values(BatchEqProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.trial_values(v); });
}

int ebc_soc_step(BatchEqProbe* h) {
  return guard([&] {
    check(h);
    h->bd.soc_step();
    sync(h);
  });
}

int ebc_kkt_fallback(BatchEqProbe* h, double* err_cur, double* err_trial) { return kkt_fallback(h, err_cur, err_trial); }
int ebc_commit(BatchEqProbe* h) { return commit(h); }
int64_t ebc_get(BatchEqProbe* h, int which, double* out) { return get(h, which, out); }
int ebc_put(BatchEqProbe* h, int which, const double* in) { return put(h, which, in); }

}  // extern "C"
