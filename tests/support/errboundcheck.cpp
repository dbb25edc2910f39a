// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// Stand-alone probe (its own main) of the host side of the error bounds of a solve: the host bodies of
// kkt_errbound.h (row_abs_sum, berr_term, residual_rounding_bound — the same functions the kernel runs) over the row
// map of kkt_plan.cpp, and the estimator's state machine (NormEstState), the class the driver advances.  Built twice
// by errboundcheck.py: plain, and with -fsanitize=address,undefined.
//
//   errboundcheck rows IN OUT     IN  = int32 dim, nnz, n_dec, pad; double delta, gamma; int32 colptr[dim + 1],
//                                       rowidx[nnz] (+ one pad word if dim + 1 + nnz is odd); double lhs[nnz], rhs[dim], p[dim]
//                                       (refinecheck's `residual` input)
//                                 OUT = double r[dim] (row_residual), w[dim], sum[dim], t[dim], rho[dim], terms[dim]
//   errboundcheck normest DIM     a dialogue on stdin / stdout, one line per round.  The program prints the probe
//                                 "kind j transposed done solves estimate" (estimate as a hex float), then reads the
//                                 scalars of the product "norm1 argmax signs_repeated finite" (norm1 as a hex float)
//                                 and prints "adopt 0|1" (sign(v) becomes the kept sign vector) — until done is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sleipnir_amd/csrc/kkt_errbound.h"
#include "../../sleipnir_amd/csrc/kkt_plan.hpp"

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

// a lower-CSC pattern that holds every diagonal entry, like pattern 5
bool lower_csc(slpx::CscPattern& out, int32_t dim, const std::vector<int32_t>& colptr, const std::vector<int32_t>& rowidx) {
  if (colptr.empty() || colptr.front() != 0 || colptr.back() != static_cast<int32_t>(rowidx.size())) return false;
  for (int32_t c = 0; c < dim; ++c) {
    if (colptr[c] >= colptr[c + 1] || rowidx[colptr[c]] != c) return false;
    for (int32_t q = colptr[c]; q < colptr[c + 1]; ++q) {
      if (rowidx[q] < c || rowidx[q] >= dim) return false;
      if (q > colptr[c] && rowidx[q] <= rowidx[q - 1]) return false;
    }
  }
  out.rows = out.cols = dim;
  out.colptr = colptr;
  out.rowidx = rowidx;
  return true;
}

int rows(const char* in_path, const char* out_path) {
  const std::vector<char> data = read_file(in_path);
  Reader in{data};
  FILE* out = std::fopen(out_path, "wb");
  if (!out) return 2;
  bool ok = false;
  const std::vector<int32_t> head = in.take<int32_t>(4);
  const std::vector<double> reg = in.take<double>(2);
  if (in.ok && head[0] >= 0 && head[1] >= 0) {
    const int32_t dim = head[0], nnz = head[1], n_dec = head[2];
    const std::vector<int32_t> colptr = in.take<int32_t>(static_cast<size_t>(dim) + 1), rowidx = in.take<int32_t>(nnz);
    if ((dim + 1 + nnz) % 2) (void)in.take<int32_t>(1);
    const std::vector<double> lhs = in.take<double>(nnz), rhs = in.take<double>(dim), p = in.take<double>(dim);
    slpx::CscPattern full;
    if (in.ok && lower_csc(full, dim, colptr, rowidx)) {
      const slpx::KktRowMap map = slpx::build_kkt_row_map(full);
      std::vector<double> r(dim), w(dim), sum(dim), t(dim), rho(dim), terms(dim);
      for (int32_t i = 0; i < dim; ++i) {
        r[i] = slpx::row_residual(i, map.rowptr.data(), map.ent.data(), map.col.data(), lhs.data(), p.data(), rhs[i], n_dec, reg[0], reg[1]);
        const slpx::RowAbs ra =
            slpx::row_abs_sum(i, map.rowptr.data(), map.ent.data(), map.col.data(), lhs.data(), p.data(), rhs[i], n_dec, reg[0], reg[1]);
        w[i] = ra.w;
        sum[i] = ra.sum;
        terms[i] = ra.terms;
        t[i] = slpx::berr_term(r[i], ra.w);
        rho[i] = slpx::residual_rounding_bound(r[i], ra.w, ra.terms, ra.exact);
      }
      ok = put(out, r) && put(out, w) && put(out, sum) && put(out, t) && put(out, rho) && put(out, terms);
    }
  }
  std::fclose(out);
  if (!ok) std::fprintf(stderr, "errboundcheck rows: bad input\n");
  return ok ? 0 : 1;
}

int normest(int dim) {
  if (dim < 1) return 2;
  slpx::NormEstState est(dim);
  char line[256];
  for (;;) {
    std::printf("%d %d %d %d %d %a\n", static_cast<int>(est.probe()), est.probe() == slpx::kProbeUnit ? est.unit_index() : -1,
                est.transposed() ? 1 : 0, est.done() ? 1 : 0, est.solves(), est.estimate());
    std::fflush(stdout);
    if (est.done()) return 0;
    if (!std::fgets(line, sizeof line, stdin)) return 1;
    char* at = line;
    const double norm1 = std::strtod(at, &at);
    const long argmax = std::strtol(at, &at, 10), repeated = std::strtol(at, &at, 10), finite = std::strtol(at, &at, 10);
    if (argmax < 0 || argmax >= dim) return 1;
    const bool adopt = est.advance(norm1, static_cast<int>(argmax), repeated != 0, finite != 0);
    std::printf("adopt %d\n", adopt ? 1 : 0);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "rows" && argc == 4) return rows(argv[2], argv[3]);
  if (what == "normest" && argc == 3) return normest(std::atoi(argv[2]));
  std::fprintf(stderr, "usage: errboundcheck rows IN OUT | normest DIM\n");
  return 2;
}
