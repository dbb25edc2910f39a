// The per-row formulas of the interior-point iteration as plain functions, one source for the kernels (ipm_kernels.h,
// ipm_batch_kernels.h, restoration.hip) and the host drivers (ipm.cpp), like ipm_decide.h and kkt_residual.h.  Two rules:
//  * NO `fp contract` / `reassociate` PRAGMA IN THESE BODIES.  Each instantiation keeps the contraction of the code it
//    is inlined into: hipcc fuses on the device, the x86 host does not.  Host and device bits are NOT claimed equal
//    (kkt_kernels.h pins its rounding because there they are compared).
//  * THE EXPRESSION TREE IS THE CONTRACT.  Operand order and association are what the tests pin (DESIGN.md section 4
//    names them); a body changes only together with every test that pins its bits.
// Reference lines: util/fraction_to_the_boundary_rule.hpp:19-43, interior_point.hpp:797-801, :590-600, :611-616,
// :479-480 and :625-630.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SLPX_FORMULA __host__ __device__ inline
#else
#define SLPX_FORMULA inline
#endif

namespace slpx {

// z stays within [mu / (kappa s), kappa mu / s] (interior_point.hpp:797-801)
constexpr double kKappa = 1e10;

// One row's candidate of the fraction-to-the-boundary rule: the largest alpha with v + alpha p >= (1 - tau) v, folded
// into the minimum so far.  (The rule's result is the minimum of its candidates, whatever their order.)
SLPX_FORMULA double ftb_candidate(double acc, double tau, double p, double v) {
  if (p < 0.0) acc = __builtin_fmin(acc, -tau / p * v);
  return acc;
}

// The z reset: std::clamp(z, mu / (kappa s), kappa mu / s) — a NaN z stays NaN; with lo > hi (s <= 0) whichever
// comparison holds first decides.
SLPX_FORMULA double z_reset(double z, double mu, double s) {
  const double lo = 1.0 / kKappa * mu / s, hi = kKappa * mu / s;
  return z < lo ? lo : (z > hi ? hi : z);
}

// What multiplies a row of A_i^T in the right-hand side of a second-order correction: mu / s - z / s * c with
// c = (c_i - s)_soc
SLPX_FORMULA double soc_rhs_multiplier(double mu, double s, double z, double c) {
  const double sinv = 1.0 / s;
  return mu * sinv - (sinv * z) * c;
}

// p_z of the back-substitution from p_s = c + A_i p_x: mu / s - z - z / s * p_s.  sinv = 1.0 / s is the caller's: it
// stands BEFORE p_s in every site, and with the division in here the two correction kernels' register counts moved.
SLPX_FORMULA double backsub_pz_sinv(double mu, double sinv, double z, double p_s) {
  return mu * sinv - z - (sinv * z) * p_s;
}

// The accumulators of the second-order corrections: alpha * (what was accumulated) + the trial point's value
SLPX_FORMULA double soc_accumulate(double alpha, double prev, double trial) { return alpha * prev + trial; }

}  // namespace slpx
