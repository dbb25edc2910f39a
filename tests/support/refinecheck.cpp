// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// Stand-alone probe (its own main) of the host side of the residual / refinement path: the row map
// (kkt_plan.cpp: build_kkt_row_map) and the host body of row_residual (kkt_residual.h) — the same
// functions the library uploads and the kernel runs.  Built twice by refinecheck.py: plain, and with
// -fsanitize=address,undefined.
//
//   refinecheck rowmap   IN OUT   IN  = int32 dim, nnz, colptr[dim + 1], rowidx[nnz]  (lower CSC; diagonal entries may be absent:
//                                       they are added as a bare linear-solver system adds them, complete_diagonal)
//                                 OUT = int32 full_nnz, colptr[dim + 1], rowidx[full_nnz] (the completed pattern),
//                                       user_map[nnz], rowptr[dim + 1], count, ent[count], col[count]
//   refinecheck residual IN OUT   IN  = int32 dim, nnz, n_dec, pad; double delta, gamma; int32 colptr[dim + 1],
//                                       rowidx[nnz] (+ one pad word if dim + 1 + nnz is odd); double lhs[nnz], rhs[dim], p[dim]
//                                 OUT = double r[dim] (double-double), r_plain[dim] (plain double, same order)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sleipnir_amd/csrc/kkt_plan.hpp"
#include "../../sleipnir_amd/csrc/kkt_residual.h"

namespace {

std::vector<char> read_file(const char* path) {
  std::vector<char> data;
  if (FILE* f = std::fopen(path, "rb")) {
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
    std::fclose(f);
  }
  return data;
}

struct Reader {
  const std::vector<char>& data;
  size_t at = 0;
  bool ok = true;
  template <class T>
  std::vector<T> take(size_t count) {
    std::vector<T> out(count);
    if (at + count * sizeof(T) > data.size()) {
      ok = false;
      return out;
    }
    if (count) std::memcpy(out.data(), data.data() + at, count * sizeof(T));
    at += count * sizeof(T);
    return out;
  }
};

template <class T>
bool put(FILE* f, const std::vector<T>& v) {
  return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

bool lower_csc(slpx::CscPattern& full, std::vector<int32_t>& user_map, int32_t dim, const std::vector<int32_t>& colptr,
               const std::vector<int32_t>& rowidx) {
  slpx::CscPattern lower;
  if (colptr.empty() || colptr.front() != 0 || colptr.back() != static_cast<int32_t>(rowidx.size())) return false;
  for (int32_t c = 0; c < dim; ++c) {
    if (colptr[c] > colptr[c + 1]) return false;
    for (int32_t q = colptr[c]; q < colptr[c + 1]; ++q)
      if (rowidx[q] < c || rowidx[q] >= dim) return false;
  }
  lower.rows = lower.cols = dim;
  lower.colptr = colptr;
  lower.rowidx = rowidx;
  std::vector<uint8_t> diag_given;
  full = slpx::complete_diagonal(lower, user_map, diag_given);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: refinecheck rowmap|residual IN OUT\n");
    return 2;
  }
  const std::string what = argv[1];
  const std::vector<char> data = read_file(argv[2]);
  Reader in{data};
  FILE* out = std::fopen(argv[3], "wb");
  if (!out) return 2;
  bool ok = false;
  if (what == "rowmap") {
    const std::vector<int32_t> head = in.take<int32_t>(2);
    if (in.ok && head[0] >= 0 && head[1] >= 0) {
      const int32_t dim = head[0], nnz = head[1];
      const std::vector<int32_t> colptr = in.take<int32_t>(static_cast<size_t>(dim) + 1), rowidx = in.take<int32_t>(nnz);
      slpx::CscPattern full;
      std::vector<int32_t> user_map;
      if (in.ok && lower_csc(full, user_map, dim, colptr, rowidx)) {
        const slpx::KktRowMap map = slpx::build_kkt_row_map(full);
        const std::vector<int32_t> full_nnz(1, full.nnz()), count(1, static_cast<int32_t>(map.ent.size()));
        ok = put(out, full_nnz) && put(out, full.colptr) && put(out, full.rowidx) && put(out, user_map) && put(out, map.rowptr) &&
             put(out, count) && put(out, map.ent) && put(out, map.col);
      }
    }
  } else if (what == "residual") {
    const std::vector<int32_t> head = in.take<int32_t>(4);
    const std::vector<double> reg = in.take<double>(2);
    if (in.ok && head[0] >= 0 && head[1] >= 0) {
      const int32_t dim = head[0], nnz = head[1], n_dec = head[2];
      const std::vector<int32_t> colptr = in.take<int32_t>(static_cast<size_t>(dim) + 1), rowidx = in.take<int32_t>(nnz);
      if ((dim + 1 + nnz) % 2) (void)in.take<int32_t>(1);
      const std::vector<double> lhs = in.take<double>(nnz), rhs = in.take<double>(dim), p = in.take<double>(dim);
      slpx::CscPattern full;
      std::vector<int32_t> user_map;
      // (values in the order of the pattern given: it must hold every diagonal entry, like pattern 5 does)
      if (in.ok && lower_csc(full, user_map, dim, colptr, rowidx) && full.nnz() == nnz) {
        const slpx::KktRowMap map = slpx::build_kkt_row_map(full);
        std::vector<double> r(dim), plain(dim);
        for (int32_t i = 0; i < dim; ++i) {
          r[i] = slpx::row_residual(i, map.rowptr.data(), map.ent.data(), map.col.data(), lhs.data(), p.data(), rhs[i], n_dec, reg[0], reg[1]);
          plain[i] = slpx::row_residual_plain(i, map.rowptr.data(), map.ent.data(), map.col.data(), lhs.data(), p.data(), rhs[i], n_dec,
                                              reg[0], reg[1]);
        }
        ok = put(out, r) && put(out, plain);
      }
    }
  }
  std::fclose(out);
  if (!ok) std::fprintf(stderr, "refinecheck %s: bad input\n", what.c_str());
  return ok ? 0 : 1;
}
