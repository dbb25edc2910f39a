// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// ldlt_run_batch (csrc/ldlt_policy.hpp) with per-problem extra pivots, driven without a device: the loop
// NewtonSystem::compute_hooked_batch runs, with a launcher that answers every attempt from a scripted inertia RESPONSE
// instead of a factorization — the script format of hostcheck.cpp's hc_reg_policy, whose drivers are the reference here
// (tests/test_batch_restoration_cpu.py).
//   mem: (prev_delta, prev_gamma) per problem, in and out;  mask: which problems take part (or none: all)
//   extra: the smallest eliminated pivot per problem, or none
//   table / table_ptr: problem b's response is rows table_ptr[b] .. table_ptr[b + 1] of 8 doubles
//     {delta below, gamma below, only where gamma == 0, n_pos, n_neg, n_zero, n_bad, min |D|}; the first row that matches
// out: attempts judged, in order {problem, delta, gamma, launch}; info per problem; counts {launches}.
// Returns the attempts (written up to cap), -1: an attempt no row answers, -2: no end in sight.
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../sleipnir_amd/csrc/device.hpp"
#include "../../sleipnir_amd/csrc/ldlt_policy.hpp"

using namespace slpx;

extern "C" int32_t rb_reg_policy_batch(int32_t n, int32_t m_e, int32_t B, double gamma_min, int32_t skip_first, int32_t launch_for_nobody,
                                       double* mem, const uint8_t* mask, const double* extra, const double* table,
                                       const int32_t* table_ptr, double* attempts, int32_t cap, int32_t* info, int32_t* counts) {
  std::vector<LdltPolicy> pol(B);
  std::vector<uint8_t> active(B, 1);
  if (mask) active.assign(mask, mask + B);
  const std::vector<uint8_t> started = active;
  for (int b = 0; b < B; ++b)
    if (active[b]) pol[b].start(n, m_e, mem[2 * b], mem[2 * b + 1], gamma_min, skip_first != 0);
  std::vector<double> extras;
  if (extra) extras.assign(extra, extra + B);
  int32_t n_attempts = 0, launches = 0;
  bool unanswered = false;
  std::vector<LdltStats> stats(B);
  try {
    counts[0] = ldlt_run_batch(
        pol, active, launch_for_nobody != 0,
        [&](const std::vector<double>& d, const std::vector<double>& g, const std::vector<uint8_t>& a) {
          for (int b = 0; b < B; ++b) {
            if (!a[b]) continue;
            if (n_attempts < cap) {
              double* o = attempts + 4 * static_cast<size_t>(n_attempts);
              o[0] = b, o[1] = d[b], o[2] = g[b], o[3] = launches;
            }
            if (++n_attempts > 4096) throw std::runtime_error("no end in sight");
            LdltStats st{0, 0, 0, 1, 0};
            bool found = false;
            for (int32_t r = table_ptr[b]; r < table_ptr[b + 1] && !found; ++r) {
              const double* t = table + 8 * static_cast<size_t>(r);
              if (!(d[b] < t[0] && g[b] < t[1]) || (t[2] != 0.0 && g[b] != 0.0)) continue;
              st = LdltStats{static_cast<int32_t>(t[3]), static_cast<int32_t>(t[4]), static_cast<int32_t>(t[5]), static_cast<int32_t>(t[6]), 0};
              std::memcpy(&st.min_abs_bits, &t[7], sizeof(double));
              found = true;
            }
            unanswered = unanswered || !found;
            stats[b] = st;
          }
          ++launches;
          return stats.data();
        },
        extra ? &extras : nullptr);
  } catch (const std::runtime_error&) {
    return -2;
  }
  if (unanswered) return -1;
  for (int b = 0; b < B; ++b) {
    info[b] = static_cast<int32_t>(started[b] ? pol[b].info : FactorInfo::Success);
    if (!started[b]) continue;
    mem[2 * b] = pol[b].prev_delta;
    mem[2 * b + 1] = pol[b].prev_gamma;
  }
  return n_attempts;
}
