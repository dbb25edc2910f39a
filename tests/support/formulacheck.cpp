// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// Stand-alone probe (its own main) of the host instantiation of the interior-point row formulas (ipm_formulas.h) —
// the bodies ipm.cpp runs, and the kernels instantiate for the device.  Built twice by formulacheck.py: plain, and
// with -fsanitize=address,undefined.
//
//   formulacheck IN OUT   IN  = int32 rows, pad; then per row 12 doubles:
//                               acc, tau, p, v,  z, mu, s,  c, p_s,  alpha, prev, trial
//                         OUT = per row 5 doubles: ftb_candidate(acc, tau, p, v), z_reset(z, mu, s),
//                               soc_rhs_multiplier(mu, s, z, c), backsub_pz_sinv(mu, 1 / s, z, p_s),
//                               soc_accumulate(alpha, prev, trial)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sleipnir_amd/csrc/ipm_formulas.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: formulacheck IN OUT\n");
    return 2;
  }
  constexpr int kIn = 12, kOut = 5;
  std::vector<char> data;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    char buf[1 << 14];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
    std::fclose(f);
  }
  int32_t head[2] = {-1, 0};
  if (data.size() >= sizeof head) std::memcpy(head, data.data(), sizeof head);
  const int32_t rows = head[0];
  if (rows < 0 || data.size() != sizeof head + static_cast<size_t>(rows) * kIn * sizeof(double)) {
    std::fprintf(stderr, "formulacheck: bad input\n");
    return 1;
  }
  std::vector<double> in(static_cast<size_t>(rows) * kIn), out(static_cast<size_t>(rows) * kOut);
  if (rows) std::memcpy(in.data(), data.data() + sizeof head, in.size() * sizeof(double));
  for (int32_t i = 0; i < rows; ++i) {
    const double* a = &in[static_cast<size_t>(i) * kIn];
    double* o = &out[static_cast<size_t>(i) * kOut];
    const double acc = a[0], tau = a[1], p = a[2], v = a[3], z = a[4], mu = a[5], s = a[6], c = a[7], p_s = a[8],
                 alpha = a[9], prev = a[10], trial = a[11];
    o[0] = slpx::ftb_candidate(acc, tau, p, v);
    o[1] = slpx::z_reset(z, mu, s);
    o[2] = slpx::soc_rhs_multiplier(mu, s, z, c);
    o[3] = slpx::backsub_pz_sinv(mu, 1.0 / s, z, p_s);
    o[4] = slpx::soc_accumulate(alpha, prev, trial);
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const bool ok = out.empty() || std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  std::fclose(f);
  return ok ? 0 : 1;
}
