// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// What the probes of the batched device structs (batchcheck.cpp, eqbatchcheck.cpp) share: the error string behind
// *_last_error, the exception guard of every entry point, and the bodies of get / put / kkt_fallback.  A probe is a
// struct with `sys`, `bd`, `buffer(which)` and `kName`.
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../sleipnir_amd/csrc/capi_internal.hpp"

namespace probe {

static std::string g_error;  // (one per probe library)

template <class F>
int guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return -1;
  } catch (...) {
    g_error = "unknown error";
    return -1;
  }
}

template <class T>
std::vector<T> vec(const T* p, size_t n) {
  return p ? std::vector<T>(p, p + n) : std::vector<T>();
}

template <class Probe>
void check(Probe* h) {
  if (!h) throw std::runtime_error(std::string(Probe::kName) + ": no probe");
}

template <class Probe>
void sync(Probe* h) {
  SLPX_HIP_CHECK(hipStreamSynchronize(h->sys.device().stream()));
}

template <class Probe>
Probe* create(slpx_system* s) {
  Probe* h = nullptr;
  guard([&] {
    if (!s) throw std::runtime_error(std::string(Probe::kName) + ": no system");
    h = new Probe(s->get());
  });
  return h;
}

// length of buffer `which` (Probe::buffer); out != nullptr: its contents
template <class Probe>
int64_t get(Probe* h, int which, double* out) {
  int64_t count = -1;
  const int rc = guard([&] {
    check(h);
    const auto [p, n] = h->buffer(which);
    sync(h);
    if (out && n) SLPX_HIP_CHECK(hipMemcpy(out, p, n * sizeof(double), hipMemcpyDeviceToHost));
    count = static_cast<int64_t>(n);
  });
  return rc == 0 ? count : -1;
}

template <class Probe>
int put(Probe* h, int which, const double* in) {
  return guard([&] {
    check(h);
    const auto [p, n] = h->buffer(which);
    sync(h);
    if (n) SLPX_HIP_CHECK(hipMemcpy(p, in, n * sizeof(double), hipMemcpyHostToDevice));
  });
}

// a launch wrapper of the device struct that fills one vector of per-instance scalars
template <class Probe, class Call>
int scalars_out(Probe* h, double* out, Call&& call) {
  return guard([&] {
    check(h);
    std::vector<double> v;
    call(h->bd, v);
    std::memcpy(out, v.data(), v.size() * sizeof(double));
  });
}

template <class Probe>
int kkt_fallback(Probe* h, double* err_cur, double* err_trial) {
  return guard([&] {
    check(h);
    std::vector<double> c, t;
    h->bd.kkt_fallback(c, t);
    std::memcpy(err_cur, c.data(), c.size() * sizeof(double));
    std::memcpy(err_trial, t.data(), t.size() * sizeof(double));
  });
}

template <class Probe>
int commit(Probe* h) {
  return guard([&] {
    check(h);
    h->bd.commit();
    sync(h);
  });
}

}  // namespace probe
