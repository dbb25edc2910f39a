// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// A probe of slpx::FrDevice (restoration.hpp): plain C entry points that drive the REAL launch wrappers of libslpx.so
// (restoration.hip) one at a time on the NewtonSystem behind an slpx_system handle of batch 1, the sweeps the
// restoration driver (ipm_restoration.cpp: restoration_core) runs between them, and get / put on every buffer those kernels read
// or write — the outer system's and the FrDevice's own.  Nothing of the kernels is compiled here.
// tests/test_restoration_kernels_gpu.py compares what comes back with tests/support/fr_reference.py.
#include "../../sleipnir_amd/csrc/restoration.hpp"
#include "probe_common.hpp"

namespace slpx {

struct FrProbe {
  static constexpr const char* kName = "frcheck";
  explicit FrProbe(NewtonSystem& s) : sys(s), fr((s.device().ipm_enable(), s.restoration_device())) {}
  NewtonSystem& sys;
  FrDevice& fr;

  // the buffers fc_get / fc_put reach: device pointer and length (doubles)
  std::pair<double*, size_t> buffer(int which) {
    DeviceNlp& dev = sys.device();
    const NlpStructure& st = sys.structure();
    const size_t n = st.n, m_e = st.m_e, m_i = st.m_i, dim = n + m_e, nV = st.nV, M = 2 * m_e + 2 * m_i;
    const size_t nnz = static_cast<size_t>(sys.kkt().lhs.nnz()), nin = st.n_inputs();
    const FrDevice::View v = fr.view();
    auto own = [](const double* p, size_t count) { return std::pair<double*, size_t>{const_cast<double*>(p), count}; };
    switch (which) {
      case 0: return {dev.d_V(), nV};
      case 1: return {dev.d_V_trial(), nV};
      case 2: return {dev.d_x(), nin};  // [x | y | z_0] as the tape reads it
      case 3: return {dev.d_trial_in(), nin};
      case 4: return {dev.d_s(), m_i};
      case 5: return {dev.d_y(), m_e};
      case 6: return {dev.d_z(), m_i};
      case 7: return {dev.d_p(), dim};
      case 8: return {dev.d_ps(), m_i};
      case 9: return {dev.d_pz(), m_i};
      case 10: return {dev.lhs_raw(), nnz};
      case 11: return {dev.rhs_raw(), dim};
      case 12: return {dev.d_s_ahead(), m_i};
      case 13: return {dev.d_y_ahead(), m_e};
      case 14: return {dev.d_z_ahead(), m_i};
      case 15: return own(fr.second_lhs(), v.second_lhs_count ? nnz : 0);
      case 16: return own(fr.second_rhs(), v.second_rhs_count ? dim : 0);
      case 17: return own(v.soc_ce, m_e);
      case 18: return own(v.soc_c0, m_i);
      case 19: return own(v.soc_x, M);
      case 20: return own(v.keep_p, dim);
      case 21: return own(v.keep_ps0, m_i);
      case 22: return own(v.keep_pz0, m_i);
      case 23: return own(v.keep_dpn, M);
      case 24: return own(v.keep_psx, M);
      case 25: return own(v.keep_pzx, M);
      case 26: return own(v.pn, M);
      case 27: return own(v.sx, M);
      case 28: return own(v.zx, M);
      case 29: return own(v.dpn, M);
      case 30: return own(v.psx, M);
      case 31: return own(v.pzx, M);
      case 32: return own(v.pn_ahead, M);
      case 33: return own(v.sx_ahead, M);
      case 34: return own(v.zx_ahead, M);
      case 35: return own(v.alpha, 4);
      default: throw std::runtime_error("frcheck: bad buffer selector");
    }
  }
};

}  // namespace slpx

using slpx::FrProbe;

using namespace probe;

namespace {

constexpr size_t kHostDoubles = sizeof(slpx::FrHost) / sizeof(double);
static_assert(sizeof(slpx::FrHost) % sizeof(double) == 0 && kHostDoubles == 4 + 4 + 2 * (24 + 5), "FrHost is all doubles: dir, trial, err, err_ahead");

// one launch wrapper, then the stream drained: what it wrote (device buffers and the pinned FrHost) is there to read
template <class Call>
int launch(FrProbe* h, Call&& call) {
  return guard([&] {
    check(h);
    call(*h);
    sync(h);
  });
}

}  // namespace

extern "C" {

const char* fc_last_error() { return g_error.c_str(); }

FrProbe* fc_create(slpx_system* s) { return create<FrProbe>(s); }

void fc_destroy(FrProbe* h) { delete h; }

// n, m_e, m_i, dim, nV, nnz of the lhs, M = 2 m_e + 2 m_i, length of the tape input, separable sums of the tape, doubles of FrHost
int fc_dims(FrProbe* h, int64_t* out) {
  return guard([&] {
    check(h);
    const slpx::NlpStructure& st = h->sys.structure();
    const int64_t v[10] = {st.n, st.m_e, st.m_i, st.n + st.m_e, st.nV, h->sys.kkt().lhs.nnz(), 2 * st.m_e + 2 * st.m_i, st.n_inputs(),
                           h->sys.device().n_reduces(), static_cast<int64_t>(kHostDoubles)};
    std::memcpy(out, v, sizeof(v));
  });
}

// the outer iterate (x, s_0, y, z_0) the way the driver uploads it
int fc_set_outer(FrProbe* h, const double* x, const double* s, const double* y, const double* z) {
  return launch(h, [&](FrProbe& p) {
    p.sys.device().upload_x(x);
    p.sys.device().upload_duals(s, y, z);
  });
}

int fc_begin(FrProbe* h, const double* x_r, const double* w, const double* g_outer, const double* s_outer, double mu_outer, const double* pn,
             const double* sx, const double* zx, const double* err_scales) {
  return launch(h, [&](FrProbe& p) {
    const slpx::NlpStructure& st = p.sys.structure();
    p.fr.begin(x_r, w, g_outer, s_outer, mu_outer, pn, sx, zx, vec(err_scales, static_cast<size_t>(1 + st.m_e + st.m_i)));
  });
}

int fc_build(FrProbe* h, double delta, double mu, int soc, int rhs_only, int second) {
  return launch(h, [&](FrProbe& p) { p.fr.build(delta, mu, soc != 0, rhs_only != 0, second != 0); });
}
int fc_build_pair(FrProbe* h, double delta, double delta_second, double mu) {
  return launch(h, [&](FrProbe& p) { p.fr.build_pair(delta, delta_second, mu); });
}
int fc_expand(FrProbe* h, double delta, double mu, double tau, int soc, int ahead) {
  return launch(h, [&](FrProbe& p) { p.fr.expand(delta, mu, tau, soc != 0, ahead != 0); });
}
int fc_accept_lookahead(FrProbe* h) {
  return launch(h, [&](FrProbe& p) { p.fr.accept_lookahead(); });
}
int fc_trial_point(FrProbe* h, double alpha) {
  return launch(h, [&](FrProbe& p) { p.fr.trial_point(alpha); });
}
int fc_trial_metrics(FrProbe* h, double alpha, double mu) {
  return launch(h, [&](FrProbe& p) { p.fr.trial_metrics(alpha, mu); });
}
int fc_commit(FrProbe* h, double alpha, double alpha_z, double mu) {
  return launch(h, [&](FrProbe& p) { p.fr.commit(alpha, alpha_z, mu); });
}
int fc_errors(FrProbe* h, int check_all_V, double mu, int ahead, int sums_ride) {
  return launch(h, [&](FrProbe& p) { p.fr.errors(check_all_V != 0, mu, ahead != 0, sums_ride != 0); });
}
int fc_soc_accumulate(FrProbe* h, double alpha, int first) {
  return launch(h, [&](FrProbe& p) { p.fr.soc_accumulate(alpha, first != 0); });
}
int fc_save_direction(FrProbe* h) {
  return launch(h, [&](FrProbe& p) { p.fr.save_direction(); });
}
int fc_restore_direction(FrProbe* h) {
  return launch(h, [&](FrProbe& p) { p.fr.restore_direction(); });
}
int fc_wait_published(FrProbe* h) {
  return launch(h, [&](FrProbe& p) { p.fr.wait_published(); });
}

// the sweeps of the driver between those launches
int fc_sweep_full(FrProbe* h, int with_reduce) {
  return launch(h, [&](FrProbe& p) { p.sys.device().sweep_full(with_reduce != 0); });
}
int fc_sweep_values_trial(FrProbe* h) {
  return launch(h, [&](FrProbe& p) { p.sys.device().sweep_values_trial(); });
}
int fc_sweep_full_lookahead(FrProbe* h, int with_reduce) {
  return launch(h, [&](FrProbe& p) { p.sys.device().sweep_full_lookahead(with_reduce != 0, /*skippable=*/false); });
}

int fc_download_state(FrProbe* h, double* pn, double* sx, double* zx) {
  return launch(h, [&](FrProbe& p) { p.fr.download_state(pn, sx, zx); });
}
int fc_download_direction(FrProbe* h, double* dpn, double* psx, double* pzx) {
  return launch(h, [&](FrProbe& p) { p.fr.download_direction(dpn, psx, pzx); });
}

// FrHost as doubles: dir (4), trial (4), err (24 + 5), err_ahead (24 + 5)
int fc_host(FrProbe* h, double* out) {
  return launch(h, [&](FrProbe& p) { std::memcpy(out, &p.fr.host(), sizeof(slpx::FrHost)); });
}

int64_t fc_get(FrProbe* h, int which, double* out) { return get(h, which, out); }
int fc_put(FrProbe* h, int which, const double* in) { return put(h, which, in); }

}  // extern "C"
