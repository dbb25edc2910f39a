// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// Stand-alone probe (its own main) of the host instantiation of the warm-start formulas (warm_start.h) — the bodies
// ipm.cpp runs, and the batched kernels instantiate for the device.  Built twice by warmcheck_host.py: plain, and with
// -fsanitize=address,undefined.
//
//   warmcheck_host IN OUT   IN  = int32 rows, pad; then per row 12 doubles:
//                                 v_u, d_c, d_f,  mu_given, sum, count, mu_min,  given_s, s, c_i,  given_z, z
//                           OUT = per row 13 doubles:
//                                 0 warm_scale_s(v_u, d_c)            1 warm_unscale_s(of 0, d_c)
//                                 2 warm_scale_dual(v_u, d_c, d_f)    3 warm_unscale_dual(of 2, d_c, d_f)
//                                 4 warm_scale_mu(v_u, d_f)           5 warm_unscale_mu(of 4, d_f)
//                                 6 warm_bad(v_u)                     7 warm_counts(s, z)
//                                 8 mu = warm_mu(sum, count, mu_given, d_f, mu_min)
//                                 9 S = warm_slack(given_s, s, c_i, mu)    10 its repair count
//                                11 warm_dual(given_z, z, mu, S)           12 its repair count
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sleipnir_amd/csrc/warm_start.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: warmcheck_host IN OUT\n");
    return 2;
  }
  constexpr int kIn = 12, kOut = 13;
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
    std::fprintf(stderr, "warmcheck_host: bad input\n");
    return 1;
  }
  std::vector<double> in(static_cast<size_t>(rows) * kIn), out(static_cast<size_t>(rows) * kOut);
  if (rows) std::memcpy(in.data(), data.data() + sizeof head, in.size() * sizeof(double));
  for (int32_t i = 0; i < rows; ++i) {
    const double* a = &in[static_cast<size_t>(i) * kIn];
    double* o = &out[static_cast<size_t>(i) * kOut];
    const double v_u = a[0], d_c = a[1], d_f = a[2], mu_given = a[3], sum = a[4], count = a[5], mu_min = a[6];
    const bool given_s = a[7] != 0.0, given_z = a[10] != 0.0;
    const double s = a[8], c_i = a[9], z = a[11];
    o[0] = slpx::warm_scale_s(v_u, d_c);
    o[1] = slpx::warm_unscale_s(o[0], d_c);
    o[2] = slpx::warm_scale_dual(v_u, d_c, d_f);
    o[3] = slpx::warm_unscale_dual(o[2], d_c, d_f);
    o[4] = slpx::warm_scale_mu(v_u, d_f);
    o[5] = slpx::warm_unscale_mu(o[4], d_f);
    o[6] = slpx::warm_bad(v_u) ? 1.0 : 0.0;
    o[7] = slpx::warm_counts(s, z) ? 1.0 : 0.0;
    const double mu = o[8] = slpx::warm_mu(sum, count, mu_given, d_f, mu_min);
    int rep_s = 0, rep_z = 0;
    o[9] = slpx::warm_slack(given_s, s, c_i, mu, &rep_s);
    o[10] = rep_s;
    o[11] = slpx::warm_dual(given_z, z, mu, o[9], &rep_z);
    o[12] = rep_z;
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const bool ok = out.empty() || std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  std::fclose(f);
  return ok ? 0 : 1;
}
