// The formulas of a warm start as plain functions, one source for the single solve's host path (ipm.cpp) and the
// batched kernels (warm_start_batch_kernels.h), in the style of ipm_formulas.h and under its two rules: no `fp contract`
// pragma in these bodies, and THE EXPRESSION TREE IS THE CONTRACT (tests/test_warm_start_cpu.py and
// tests/test_warm_start_kernels_gpu.py pin the bits).
//
// UNITS.  A solve runs on the scaled problem, and its scales d_f, d_ce, d_ci are computed anew at every solve's x0, so a
// scaled iterate does not carry over from one solve to the next.  A warm start crosses the seam in the user's units:
//     s_u = s / d_ci      y_u = y * (d_ce / d_f)      z_u = z * (d_ci / d_f)      mu_u = mu / d_f
// (the un-scaling of the error measure, ipm_host.hpp: kkt_error_impl); y_u, z_u are the multipliers of
// f - y^T c_e - z^T c_i as the user wrote it.  The way in divides by the SAME quotient the way out multiplies with, so
// out(in(v)) is two roundings away from v, and with scales of 1 both directions return their argument's bits.
//
// SAFEGUARD (per instance, scaled space, the scales of the solve at hand; c_i is the scaled constraint value at x0):
//  1. a NaN or Inf in a given entry ends the instance with NONFINITE_INITIAL_GUESS (warm_bad);
//  2. mu: the given one where it is > 0, floored at mu_min; else the mean of s_j z_j over the rows where both are given
//     and positive, within [mu_min, 0.1 d_f]; else 0.1 d_f, the cold start's (warm_mu);
//  3. s_j absent or <= 0: max(c_i_j, mu) (warm_slack);
//  4. z_j absent or <= 0: mu / s_j; then every z_j through z_reset, the clamp every commit applies (warm_dual);
//  5. y absent: 0.
// No absolute floor anywhere: at a solution an active row has s ~ mu / z ~ 1e-9, and that is the iterate to keep.
#pragma once

#include "ipm_formulas.h"

namespace slpx {

// ---- the two conversions, per entry ----
SLPX_FORMULA double warm_scale_s(double s_u, double d_ci) { return d_ci * s_u; }
SLPX_FORMULA double warm_unscale_s(double s, double d_ci) { return s / d_ci; }
// y with d_c = d_ce, z with d_c = d_ci
SLPX_FORMULA double warm_scale_dual(double v_u, double d_c, double d_f) { return v_u / (d_c / d_f); }
SLPX_FORMULA double warm_unscale_dual(double v, double d_c, double d_f) { return v * (d_c / d_f); }
SLPX_FORMULA double warm_scale_mu(double mu_u, double d_f) { return d_f * mu_u; }
SLPX_FORMULA double warm_unscale_mu(double mu, double d_f) { return mu / d_f; }

// a given entry that is NaN or Inf (v - v is 0 for every finite v and NaN otherwise)
SLPX_FORMULA bool warm_bad(double v) { return !(v - v == 0.0); }

// a row that counts for the mean of step 2: both given (the caller's business) and positive
SLPX_FORMULA bool warm_counts(double s, double z) { return s > 0.0 && z > 0.0; }

// The barrier parameter a warm start begins with: `sum`, `count` of s_j z_j over the rows that count, mu_given the
// caller's (unscaled; <= 0: choose).
SLPX_FORMULA double warm_mu(double sum, double count, double mu_given, double d_f, double mu_min) {
  if (mu_given > 0.0) {
    const double mu = warm_scale_mu(mu_given, d_f);
    return mu > mu_min ? mu : mu_min;
  }
  const double mu_cold = 0.1 * d_f;
  if (!(count > 0.0)) return mu_cold;
  double mu = sum / count;
  mu = mu < mu_cold ? mu : mu_cold;
  return mu > mu_min ? mu : mu_min;
}

// step 3; *repaired is counted up where the value was replaced
SLPX_FORMULA double warm_slack(bool given, double s, double c_i, double mu, int* repaired) {
  if (given && s > 0.0) return s;
  ++*repaired;
  return c_i > mu ? c_i : mu;
}

// step 4 (s is the slack AFTER step 3); *repaired is counted up once where the value was replaced or the clamp moved it
SLPX_FORMULA double warm_dual(bool given, double z, double mu, double s, int* repaired) {
  const bool keep = given && z > 0.0;
  const double z0 = keep ? z : mu / s;
  const double z1 = z_reset(z0, mu, s);
  if (!keep || z1 != z0) ++*repaired;
  return z1;
}

}  // namespace slpx
