// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// A probe of slpx::BatchIpmDevice (ipm_batch.hpp): plain C entry points that drive the REAL launch wrappers of
// libslpx.so (ipm_batch_launch.hip) on the NewtonSystem behind an slpx_system handle — the batch system that
// slpx_system_create(problem, B, 0) makes, tape at unit scales, as Problem::batch_system does — and read back every
// per-instance buffer.  Nothing of the kernels is compiled here.  tests/test_solve_batch_kernels_gpu.py compares what
// comes back with numpy.
#include "../../sleipnir_amd/csrc/ipm_batch.hpp"
#include "probe_common.hpp"

namespace slpx {

struct BatchIpmProbe {
  static constexpr const char* kName = "batchcheck";
  explicit BatchIpmProbe(NewtonSystem& s) : sys(s), bd(s) {}
  NewtonSystem& sys;
  BatchIpmDevice bd;

  // the buffers bc_get / bc_put reach: device pointer and length (doubles)
  std::pair<double*, size_t> buffer(int which) {
    DeviceNlp& dev = sys.device();
    const size_t B = bd.B, n = bd.n, m_e = bd.m_e, m_i = bd.m_i, dim = bd.dim, nV = bd.nV;
    switch (which) {
      case 0: return {bd.m_x.p, B * n};
      case 1: return {bd.m_s.p, B * m_i};
      case 2: return {bd.m_y.p, B * m_e};
      case 3: return {bd.m_z.p, B * m_i};
      case 4: return {bd.m_tx.p, B * n};
      case 5: return {bd.m_ts.p, B * m_i};
      case 6: return {bd.m_ty.p, B * m_e};
      case 7: return {bd.m_tz.p, B * m_i};
      case 8: return {bd.m_sx.p, B * n};
      case 9: return {bd.m_ss.p, B * m_i};
      case 10: return {bd.m_sy.p, B * m_e};
      case 11: return {bd.m_sz.p, B * m_i};
      case 12: return {bd.m_p.p, B * dim};
      case 13: return {bd.m_ps.p, B * m_i};
      case 14: return {bd.m_pz.p, B * m_i};
      case 15: return {bd.m_Vcur.p, B * nV};
      case 16: return {bd.m_tce.p, B * m_e};
      case 17: return {bd.m_tci.p, B * m_i};
      case 18: return {bd.m_sce.p, B * m_e};
      case 19: return {bd.m_scims.p, B * m_i};
      case 20: return {bd.m_out.p, B * kBatchErrN};
      case 21: return {dev.d_V(), B * nV};    // the system's V (the last sweep's, scaled)
      case 22: return {dev.d_rhs(), B * dim};  // the system's rhs
      case 23: return {dev.d_p(), B * dim};    // the system's solution
      case 24: return {dev.d_s(), B * m_i};    // the system's s, y, z (what assemble / build_rhs read)
      case 25: return {dev.d_y(), B * m_e};
      case 26: return {dev.d_z(), B * m_i};
      case 27: return {dev.d_lhs(), B * static_cast<size_t>(sys.kkt().lhs.nnz())};
      case 28: return {dev.d_ps(), B * m_i};   // the system's p_s, p_z (what newton_direction takes)
      case 29: return {dev.d_pz(), B * m_i};
      default: throw std::runtime_error("batchcheck: bad buffer selector");
    }
  }
};

}  // namespace slpx

using slpx::BatchIpmProbe;

using namespace probe;

extern "C" {

const char* bc_last_error() { return g_error.c_str(); }

BatchIpmProbe* bc_create(slpx_system* s) { return create<BatchIpmProbe>(s); }

void bc_destroy(BatchIpmProbe* h) { delete h; }

// B, n, m_e, m_i, dim, ns, nV, nnz of the lhs
int bc_dims(BatchIpmProbe* h, int64_t* out) {
  return guard([&] {
    check(h);
    const auto& bd = h->bd;
    const int64_t v[8] = {bd.B, bd.n, bd.m_e, bd.m_i, bd.dim, bd.ns, bd.nV, h->sys.kkt().lhs.nnz()};
    std::memcpy(out, v, sizeof(v));
  });
}

int bc_set_scales(BatchIpmProbe* h, const double* scales) {
  return guard([&] {
    check(h);
    h->bd.set_scales(vec(scales, static_cast<size_t>(h->bd.B) * h->bd.ns));
  });
}

int bc_set_iterate(BatchIpmProbe* h, const double* x, const double* s, const double* y, const double* z) {
  return guard([&] {
    check(h);
    const size_t B = h->bd.B;
    h->bd.set_iterate(vec(x, B * h->bd.n), vec(s, B * h->bd.m_i), vec(y, B * h->bd.m_e), vec(z, B * h->bd.m_i));
  });
}

// the per-instance parameters of the next launches, then upload()
int bc_set_params(BatchIpmProbe* h, const double* mu, const double* tau, const double* alpha, const double* alpha_z,
                  const double* alpha_soc, const int32_t* mode, const uint8_t* s_from_ci, const uint8_t* first,
                  const uint8_t* active) {
  return guard([&] {
    check(h);
    auto& bd = h->bd;
    const size_t B = bd.B;
    bd.mu = vec(mu, B);
    bd.tau = vec(tau, B);
    bd.alpha = vec(alpha, B);
    bd.alpha_z = vec(alpha_z, B);
    bd.alpha_soc = vec(alpha_soc, B);
    bd.mode = vec(mode, B);
    bd.s_from_ci = vec(s_from_ci, B);
    bd.first = vec(first, B);
    bd.active = vec(active, B);
    bd.upload();
  });
}

// the host copy of s_from_ci (kkt_fallback clears it)
int bc_get_s_from_ci(BatchIpmProbe* h, uint8_t* out) {
  return guard([&] {
    check(h);
    std::memcpy(out, h->bd.s_from_ci.data(), h->bd.s_from_ci.size());
  });
}

// the Newton system of the refreshed iterate, as the driver builds it: mu, lhs, rhs
int bc_assemble(BatchIpmProbe* h) {
  return guard([&] {
    check(h);
    slpx::DeviceNlp& dev = h->sys.device();
    dev.upload_mu(h->bd.mu.data());
    dev.assemble();
    dev.build_rhs();
    sync(h);
  });
}

int bc_reset_regularization(BatchIpmProbe* h, double gamma_min) {
  return guard([&] {
    check(h);
    h->sys.reset_regularization();
    h->sys.set_gamma_min(gamma_min);
  });
}

// the δ/γ memory of every instance
int bc_set_regularization(BatchIpmProbe* h, const double* delta, const double* gamma) {
  return guard([&] {
    check(h);
    h->sys.set_regularization_state({vec(delta, h->bd.B), vec(gamma, h->bd.B)});
  });
}
int bc_get_regularization(BatchIpmProbe* h, double* delta, double* gamma) {
  return guard([&] {
    check(h);
    const auto st = h->sys.regularization_state();
    std::memcpy(delta, st.first.data(), st.first.size() * sizeof(double));
    std::memcpy(gamma, st.second.data(), st.second.size() * sizeof(double));
  });
}

// NewtonSystem::compute(spec, mask) (mask == nullptr: the unmasked compute(spec)); info [B], factorizations made
int bc_compute(BatchIpmProbe* h, int spec, const uint8_t* mask, int32_t* info, int32_t* factorizations) {
  return guard([&] {
    check(h);
    const auto r = mask ? h->sys.compute(spec != 0, vec(mask, h->bd.B)) : h->sys.compute(spec != 0);
    for (size_t b = 0; b < r.size(); ++b) info[b] = static_cast<int32_t>(r[b]);
    *factorizations = h->sys.last_factorizations();
    sync(h);
  });
}

int bc_refresh(BatchIpmProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.refresh(v); });
}
int bc_newton_direction(BatchIpmProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.newton_direction(v); });
}
int bc_trial_values(BatchIpmProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.trial_values(v); });
}
int bc_soc_step(BatchIpmProbe* h, double* out) {
  return scalars_out(h, out, [](auto& bd, auto& v) { bd.soc_step(v); });
}
int bc_kkt_fallback(BatchIpmProbe* h, double* err_cur, double* err_trial) { return kkt_fallback(h, err_cur, err_trial); }
int bc_commit(BatchIpmProbe* h) { return commit(h); }
int64_t bc_get(BatchIpmProbe* h, int which, double* out) { return get(h, which, out); }
int bc_put(BatchIpmProbe* h, int which, const double* in) { return put(h, which, in); }

}  // extern "C"
