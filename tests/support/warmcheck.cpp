// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// A probe of the warm-start launches of slpx::BatchDevice (batch_lockstep.hpp: warm_start, unscaled_iterate): plain C
// entry points that drive the REAL launch wrappers of libslpx.so (ipm_batch_launch.hip) on the NewtonSystem behind an
// slpx_system handle — the batch system slpx_system_create(problem, B, 0) makes — through BatchIpmDevice where the model
// has inequality rows and BatchEqDevice where it has none, as the batched drivers do.  Nothing of the kernels is compiled
// here.  tests/test_warm_start_kernels_gpu.py compares what comes back with numpy.
#include <memory>

#include "../../sleipnir_amd/csrc/eq_batch.hpp"
#include "../../sleipnir_amd/csrc/ipm_batch.hpp"
#include "probe_common.hpp"

namespace slpx {

struct WarmProbe {
  static constexpr const char* kName = "warmcheck";
  explicit WarmProbe(NewtonSystem& s) : sys(s) {
    if (s.structure().m_i > 0) bd = (ipm = std::make_unique<BatchIpmDevice>(s)).get();
    else bd = (eq = std::make_unique<BatchEqDevice>(s)).get();
  }
  NewtonSystem& sys;
  std::unique_ptr<BatchIpmDevice> ipm;
  std::unique_ptr<BatchEqDevice> eq;
  BatchDevice* bd = nullptr;
};

}  // namespace slpx

using slpx::WarmProbe;
using namespace probe;

extern "C" {

const char* wc_last_error() { return g_error.c_str(); }
WarmProbe* wc_create(slpx_system* s) { return create<WarmProbe>(s); }
void wc_destroy(WarmProbe* h) { delete h; }

// B, n, m_e, m_i, ns, nV, off_ci
int wc_dims(WarmProbe* h, int64_t* out) {
  return guard([&] {
    check(h);
    const auto& bd = *h->bd;
    const int64_t v[7] = {bd.B, bd.n, bd.m_e, bd.m_i, bd.ns, bd.nV, h->sys.structure().off_ci};
    std::memcpy(out, v, sizeof(v));
  });
}

int wc_set_scales(WarmProbe* h, const double* scales) {
  return guard([&] {
    check(h);
    h->bd->set_scales(vec(scales, static_cast<size_t>(h->bd->B) * h->bd->ns));
  });
}

int wc_set_iterate(WarmProbe* h, const double* x, const double* s, const double* y, const double* z) {
  return guard([&] {
    check(h);
    const auto& bd = *h->bd;
    const size_t B = bd.B;
    h->bd->set_iterate(vec(x, B * bd.n), vec(s, B * bd.m_i), vec(y, B * bd.m_e), vec(z, B * bd.m_i));
  });
}

int wc_get_iterate(WarmProbe* h, double* x, double* s, double* y, double* z) {
  return guard([&] {
    check(h);
    std::vector<double> X, S, Y, Z;
    h->bd->get_iterate(X, S, Y, Z);
    auto copy = [](const std::vector<double>& v, double* out) {
      if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(double));
    };
    copy(X, x);
    copy(S, s);
    copy(Y, y);
    copy(Z, z);
  });
}

// c_i [B][m_i] into the system's V (what the scaling sweep at unit scales leaves there)
int wc_set_ci(WarmProbe* h, const double* ci) {
  return guard([&] {
    check(h);
    const auto& bd = *h->bd;
    sync(h);
    const size_t off = h->sys.structure().off_ci;
    for (int b = 0; b < bd.B && bd.m_i; ++b)
      SLPX_HIP_CHECK(hipMemcpy(h->sys.device().d_V() + static_cast<size_t>(b) * bd.nV + off, ci + static_cast<size_t>(b) * bd.m_i,
                               bd.m_i * sizeof(double), hipMemcpyHostToDevice));
  });
}

// BatchDevice::warm_start: s0, y0, z0, mu0 may be null; run [B], mu_min [B]; out [B][3]
int wc_warm_start(WarmProbe* h, const double* s0, const double* y0, const double* z0, const double* mu0, const uint8_t* run,
                  const double* mu_min, double* out) {
  return guard([&] {
    check(h);
    const size_t B = h->bd->B;
    std::vector<double> o;
    h->bd->warm_start(slpx::BatchWarmStart{s0, y0, z0, mu0}, vec(run, B), vec(mu_min, B), o);
    std::memcpy(out, o.data(), o.size() * sizeof(double));
  });
}

// BatchDevice::unscaled_iterate: run [B]; s_u [B][m_i], y_u [B][m_e], z_u [B][m_i]
int wc_unscaled_iterate(WarmProbe* h, const uint8_t* run, double* s_u, double* y_u, double* z_u) {
  return guard([&] {
    check(h);
    std::vector<double> S, Y, Z;
    h->bd->unscaled_iterate(vec(run, static_cast<size_t>(h->bd->B)), S, Y, Z);
    sync(h);
    auto copy = [](const std::vector<double>& v, double* out) {
      if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(double));
    };
    copy(S, s_u);
    copy(Y, y_u);
    copy(Z, z_u);
  });
}

}  // extern "C"
