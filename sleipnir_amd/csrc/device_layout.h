// How the device images are laid out: the constants and `__host__ __device__` helpers the packers
// (device_images.cpp) write by and the kernels read by.  No kernel in here, so host code that only packs or
// checks an image can include it; the kernel headers that own each piece (named at it) carry the reasoning
// and the measurements.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldlt_symbolic.hpp"

namespace slpx {

// ---- inline KKT terms and back-substitution rows (device.hpp: KktFuse, BacksubFuse) ----
// One addend of an lhs / rhs entry that is a sum (kkt_kernels.h: kkt_terms_value); twelve bytes,
// staged into LDS with the task's plan.  kind = b >> 28, row = b & 0x0fffffff:
//   0  direct += V[a]                 1  g = V[a]                  2  aey += V[a] * y[row]
//   3  ait += V[a] * (-(z/s)[row] * V[c] + mu / s[row] + z[row])   4  prod += (V[a] * (z/s)[row]) * V[c]
struct KktTerm {
  int32_t a, b, c;
};
struct BsRow {
  int32_t r;       // row of A_i
  uint32_t terms;  // first term (relative to the task's block) | number of terms << 20
};
struct BsTerm {
  int32_t a;     // V slot of the A_i value
  uint32_t ref;  // the task's own column (local index) or 0x80000000 | permuted column of an ancestor
};

// ---- the re-encoded source word of a sum entry in a multifrontal task image (kkt_kernels.h: kkt_terms_sum_grouped) ----
constexpr uint32_t kMfTermFirstBits = 14, kMfTermABits = 8, kMfTermBBits = 7;  // + 1 bit: the row has a gradient term
__host__ __device__ inline bool mf_term_code_fits(uint32_t first, uint32_t n_a, uint32_t n_b) {
  return first < (1u << kMfTermFirstBits) && n_a < (1u << kMfTermABits) && n_b < (1u << kMfTermBBits);
}
__host__ __device__ inline uint32_t mf_term_code(uint32_t first, uint32_t has_g, uint32_t n_a, uint32_t n_b) {
  return first | (n_a << kMfTermFirstBits) | (n_b << (kMfTermFirstBits + kMfTermABits)) |
         (has_g << (kMfTermFirstBits + kMfTermABits + kMfTermBBits));
}

// ---- update slots handed over through the data (ldlt_kernels.h: slot_take) ----
constexpr unsigned long long kSlotEmpty = 0x7ff8dead0badbeefull;

// ---- batch-interleaved LDLT (ldlt_il_kernels.h) ----
constexpr int kIlWShift = 4;  // (measured: 8-wide rows 0.74 ms per factorization of 512 x N=1000, 16-wide 0.67)
constexpr int kIlW = 1 << kIlWShift;  // problems per interleaved row
constexpr int kIlRowsPerChunk = 64 / kIlW;  // rows groups covering a 64-problem chunk
// number of 16-problem rows groups a batch occupies (padded to whole waves of 64 problems)
__host__ __device__ inline int il_groups(int batch) { return kIlRowsPerChunk * ((batch + 63) / 64); }
constexpr int kIlFactorThreads = 512;  // (ldlt_il_kernels.h has the measurements)
constexpr int kIlSlots = kIlFactorThreads / kIlW;  // entries of a level a factorization workgroup works on at a time

// ---- multifrontal task images (ldlt_mf_kernels.h: mf_step_body) ----
#ifdef SLPX_MF_CLOCKS
constexpr uint32_t kMfClockBytes = 192;  // the 24 slots of g_ldlt_clocks
#else
constexpr uint32_t kMfClockBytes = 0;
#endif
constexpr uint32_t kMfImageGroups = 6144;  // 16-byte groups of a task's image the staging loop requests: 96 KB
// byte offsets of the regions of a task's LDS, in the order listed at mf_step_body; the image is [o_tab, end of the
// KKT terms) followed by the back-substitution rows
struct MfCarve {
  uint32_t o_arena, o_invd, o_x, o_tab, o_lvl, o_ext, o_src, o_flags, o_cent, o_cptr, o_cidx, o_cp, o_anc,
      o_fr, o_cnt, o_terms;
};
__host__ __device__ inline uint32_t mf_align16(uint32_t v) { return (v + 15u) & ~15u; }
__host__ __device__ inline MfCarve mf_carve(const LdltTask& t, const LdltMfTask& m) {
  MfCarve c;
  auto q = [](uint32_t count, uint32_t per16) { return 16u * ((count + per16 - 1u) / per16); };
  c.o_arena = 8u * t.n_ent;
  c.o_invd = c.o_arena + 8u * m.arena;
  c.o_x = c.o_invd + 8u * t.n_col;
  c.o_tab = mf_align16(c.o_x + 8u * (t.n_col + m.n_anc + 1u));
  c.o_lvl = c.o_tab + q(m.n_tab, 8);
  c.o_ext = c.o_lvl + q(t.n_lvl + 1u, 4);
  c.o_src = c.o_ext + q(m.n_ext, 4);
  c.o_flags = c.o_src + q(t.n_ent, 4);
  c.o_cent = c.o_flags + q(t.n_ent, 16);
  c.o_cptr = c.o_cent + q(m.n_cent, 8);
  c.o_cidx = c.o_cptr + q(m.n_cent + 1u, 4);
  c.o_cp = c.o_cidx + q(m.n_contrib_idx, 4);
  c.o_anc = c.o_cp + q(t.n_col, 4);
  c.o_fr = c.o_anc + q(m.n_anc, 4);
  c.o_cnt = c.o_fr + 16u * m.n_front;
  c.o_terms = c.o_cnt + 32u + kMfClockBytes;
  return c;
}

}  // namespace slpx
