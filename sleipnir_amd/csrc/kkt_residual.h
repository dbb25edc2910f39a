// The residual of a solve, r = b - Kreg p, as plain functions shared by the kernel (kkt_refine.hip) and by the host
// (the CPU tests run the same body): one source for both sides, like ipm_decide.h.
//
// Kreg = K + diag(delta on the first n rows, -gamma on the others) is what the factorization in memory factored
// (sparse_regularized_ldlt.hpp:217-224); K is given by the values of its lower triangle (pattern 5) and reached
// through a ROW MAP (kkt_plan.hpp: KktRowMap): for row i the entries K(i, j), j <= i, of its own row, then the
// entries K(j, i), j > i, of column i — the mirrored half.
//
// The sum is accumulated in double-double: every product exactly (two_prod: one fma), every addition with its
// rounding error (Knuth's two_sum), the errors summed beside the running value and folded in once at the end, then
// ONE rounding to double.  The systems are ill-conditioned by construction (gamma = 1e-10): a residual in plain
// double is mostly the rounding noise of its own cancellation, and a correction solved from it refines nothing.
// Order: b_i first, then the row's entries in map order; the regularization joins as a term of its own right
// behind the diagonal entry (it is not added to the value in double first).  One lane owns one row, so the bits of
// r_i depend on nothing but the row's inputs.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SLPX_RESIDUAL __host__ __device__ inline
#else
#define SLPX_RESIDUAL inline
#endif

namespace slpx {

// The error terms below are differences the compiler must not "simplify": no contraction of a product into the
// addition that follows it (hipcc contracts by default), no reassociation.
struct DoubleDouble {
  double hi = 0.0, lo = 0.0;
};

// s + e = a + b exactly (Knuth: no assumption on the magnitudes)
SLPX_RESIDUAL void two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off) reassociate(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// p + e = a * b exactly
SLPX_RESIDUAL void two_prod(double a, double b, double& p, double& e) {
#pragma clang fp contract(off) reassociate(off)
  p = a * b;
  e = __builtin_fma(a, b, -p);
}

// acc -= a * x
SLPX_RESIDUAL void dd_sub_prod(DoubleDouble& acc, double a, double x) {
#pragma clang fp contract(off) reassociate(off)
  double p, pe, s, se;
  two_prod(a, x, p, pe);
  two_sum(acc.hi, -p, s, se);
  acc.hi = s;
  acc.lo = acc.lo + (se - pe);
}

SLPX_RESIDUAL double dd_round(const DoubleDouble& acc) {
#pragma clang fp contract(off) reassociate(off)
  return acc.hi + acc.lo;
}

// r_i = b_i - sum_j Kreg(i, j) p_j over the row map (rowptr / ent / col), lhs = the values of pattern 5 of this
// instance, p and b its solution and right-hand side; n_dec = the rows that carry +delta (the others -gamma).
SLPX_RESIDUAL double row_residual(int row, const int32_t* rowptr, const int32_t* ent, const int32_t* col, const double* lhs,
                                  const double* p, double b_i, int n_dec, double delta, double gamma) {
  DoubleDouble acc;
  acc.hi = b_i;
  const double reg = row < n_dec ? delta : -gamma;
  for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
    const int32_t j = col[q];
    const double pj = p[j];
    dd_sub_prod(acc, lhs[ent[q]], pj);
    if (j == row) dd_sub_prod(acc, reg, pj);
  }
  return dd_round(acc);
}

// The same sum in plain double, same order (what the double-double accumulation is measured against).
SLPX_RESIDUAL double row_residual_plain(int row, const int32_t* rowptr, const int32_t* ent, const int32_t* col, const double* lhs,
                                        const double* p, double b_i, int n_dec, double delta, double gamma) {
#pragma clang fp contract(off) reassociate(off)
  double acc = b_i;
  const double reg = row < n_dec ? delta : -gamma;
  for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
    const int32_t j = col[q];
    acc = acc - lhs[ent[q]] * p[j];
    if (j == row) acc = acc - reg * p[j];
  }
  return acc;
}

// |x| as an integer: non-negative doubles order like their bit patterns, and every NaN lies above +Inf — a maximum
// taken on these words is independent of the order it is taken in and cannot lose a NaN the way fmax does.
SLPX_RESIDUAL unsigned long long abs_bits(double x) {
  return static_cast<unsigned long long>(__builtin_bit_cast(unsigned long long, x)) & 0x7fffffffffffffffull;
}

}  // namespace slpx
