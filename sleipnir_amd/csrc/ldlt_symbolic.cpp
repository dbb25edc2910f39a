// Symbolic LDLᵀ: the driver (build_ldlt_plan_once: the phases in order), the pattern of L and the elimination tree,
// relaxed supernodes, tasks and rounds, supernodes and levels; the retry wrapper and the dense plan.
#include "ldlt_symbolic.hpp"

#include "ldlt_symbolic_detail.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <stdexcept>
#include <string>

namespace slpx {

namespace ldlt_detail {

// ---- permuted A: per column, strictly-lower rows with their lhs source ------
void permute_matrix(const CscPattern& lower, Elimination& E) {
  const int n = E.n;
  E.Acol.assign(n, {});
  E.diag_src.assign(n, -1);
  for (int c = 0; c < n; ++c)
    for (int p = lower.colptr[c]; p < lower.colptr[c + 1]; ++p) {
      int32_t i = E.iperm[lower.rowidx[p]], j = E.iperm[c];
      if (i == j) E.diag_src[j] = p;
      else E.Acol[std::min(i, j)].emplace_back(std::max(i, j), p);
    }
  for (auto& v : E.Acol) std::sort(v.begin(), v.end());
}

// ---- symbolic factorization: pattern of L and the etree -----------------------
void pattern_and_etree(Elimination& E) {
  const int n = E.n;
  E.Lcol.assign(n, {});
  E.children.assign(n, {});
  E.parent.assign(n, -1);
  std::vector<int32_t> tmp, tmp2;
  for (int j = 0; j < n; ++j) {
    tmp.clear();
    for (auto& [r, src] : E.Acol[j]) tmp.push_back(r);
    for (int32_t c : E.children[j]) {
      tmp2.clear();
      // Lcol[c] \ {j}
      std::set_union(tmp.begin(), tmp.end(), E.Lcol[c].begin() + 1, E.Lcol[c].end(),
                     std::back_inserter(tmp2));
      tmp.swap(tmp2);
    }
    E.Lcol[j] = tmp;
    if (!tmp.empty()) {
      E.parent[j] = tmp[0];
      E.children[tmp[0]].push_back(j);
    }
  }
  // Which diagonal entries receive an update in the EXACT structure of L (before supernodes are relaxed:
  // an explicit zero L(j, k) = 0 "updates" d_j by nothing).  A (2,2)-block diagonal without a
  // source and without such an update is a structurally zero pivot of the unregularized matrix.
  E.diag_updated_exact.assign(n, 0);
  for (int k = 0; k < n; ++k)
    for (int32_t r : E.Lcol[k]) E.diag_updated_exact[r] = 1;
}

namespace {

// the chains of equal-structure columns as they stand: chain c = col[ptr[c] .. ptr[c + 1]), sn[j] = the chain of column j
struct Chains {
  std::vector<int32_t> sn, ptr{0}, col;
  struct View {
    const int32_t *b, *e;
    size_t size() const { return static_cast<size_t>(e - b); }
    int32_t operator[](size_t i) const { return b[i]; }
    int32_t back() const { return e[-1]; }
    const int32_t* begin() const { return b; }
    const int32_t* end() const { return e; }
  };
  size_t size() const { return ptr.size() - 1; }
  View operator[](size_t c) const { return {col.data() + ptr[c], col.data() + ptr[c + 1]}; }
};

Chains exact_chains(const LdltOptions& opt, const Elimination& E) {
  const int n = E.n;
  Chains C;
  C.sn.assign(n, -1);
  C.col.reserve(n);
  for (int j = 0; j < n; ++j) {
    if (C.sn[j] >= 0) continue;
    const int32_t id = static_cast<int32_t>(C.ptr.size()) - 1;
    C.sn[j] = id;
    C.col.push_back(j);
    size_t len = 1;
    int32_t k = j;
    while (len < opt.max_supernode_width) {
      const int32_t p = E.parent[k];
      if (p < 0 || C.sn[p] >= 0 || E.Lcol[k].size() != E.Lcol[p].size() + 1 ||
          len + 1 + E.Lcol[p].size() + 1 > opt.max_front_rows)
        break;
      C.sn[p] = id;
      C.col.push_back(p);
      ++len;
      k = p;
    }
    C.ptr.push_back(static_cast<int32_t>(C.col.size()));
  }
  return C;
}

}  // namespace

// ---- relaxed supernodes (LdltOptions::relax_zeros) -------------------------------------------------
void relax_supernodes(const LdltOptions& opt, Elimination& E) {
  const int n = E.n;
  int relaxed_merges = 0;
  int64_t relaxed_zeros = 0;
  if (opt.supernodal && opt.relax_zeros > 0) {
    for (int round = 0; round < 8; ++round) {
      // the chains as they stand (exact structure), their levels
      const Chains cols = exact_chains(opt, E);
      const std::vector<int32_t>& sn = cols.sn;
      std::vector<int32_t> lvl(cols.size(), 0);
      for (int j = 0; j < n; ++j)
        for (int32_t c : E.children[j])
          if (sn[c] != sn[j]) lvl[sn[j]] = std::max(lvl[sn[j]], lvl[sn[c]] + 1);
      std::vector<int32_t> by_level(cols.size());
      std::iota(by_level.begin(), by_level.end(), 0);
      std::stable_sort(by_level.begin(), by_level.end(), [&](int32_t a, int32_t b) { return lvl[a] < lvl[b]; });
      std::vector<uint8_t> used(cols.size(), 0);
      int merged = 0;
      for (int32_t s : by_level) {
        if (used[s]) continue;
        const Chains::View ch = cols[s];
        const int32_t p = E.parent[ch.back()];
        if (p < 0) continue;
        const int32_t J = sn[p];
        if (used[J] || cols[J][0] != p || lvl[s] + 1 < lvl[J]) continue;  // joins at the head, deepest child only
        const Chains::View cj = cols[J];
        const size_t below = cj.size() + E.Lcol[cj.back()].size();  // rows under the joining columns
        if (ch.size() + cj.size() > opt.max_supernode_width || ch.size() + below + 1 > opt.max_front_rows) continue;
        int64_t zeros = 0;
        for (size_t i = 0; i < ch.size(); ++i)
          zeros += static_cast<int64_t>(ch.size() - 1 - i + below) - static_cast<int64_t>(E.Lcol[ch[i]].size());
        if (zeros > opt.relax_zeros) continue;
        std::vector<int32_t> tail(cj.begin(), cj.end());
        tail.insert(tail.end(), E.Lcol[cj.back()].begin(), E.Lcol[cj.back()].end());
        for (size_t i = 0; i < ch.size(); ++i) {
          std::vector<int32_t> rows(ch.begin() + i + 1, ch.end());
          rows.insert(rows.end(), tail.begin(), tail.end());
          E.Lcol[ch[i]] = std::move(rows);
        }
        used[s] = used[J] = 1;
        ++merged;
        relaxed_zeros += zeros;
      }
      relaxed_merges += merged;
      if (merged == 0) break;
    }
  }
  if (std::getenv("SLPX_LDLT_VERBOSE") && opt.relax_zeros > 0)
    std::fprintf(stderr, "ldlt relaxed supernodes: %d merges, %lld explicit zeros\n", relaxed_merges,
                 static_cast<long long>(relaxed_zeros));
}

int store_pattern(Elimination& E) {
  const int n = E.n;
  E.Lp.assign(n + 1, 0);
  for (int j = 0; j < n; ++j) E.Lp[j + 1] = E.Lp[j] + static_cast<int32_t>(E.Lcol[j].size());
  E.nnzL = E.Lp[n];
  E.Li.reserve(E.nnzL);
  for (int j = 0; j < n; ++j) E.Li.insert(E.Li.end(), E.Lcol[j].begin(), E.Lcol[j].end());
  int height = 0;
  std::vector<int32_t> h(n, 0);
  for (int j = 0; j < n; ++j) {
    for (int32_t c : E.children[j]) h[j] = std::max(h[j], h[c] + 1);
    height = std::max(height, h[j] + 1);
  }
  return height;
}

namespace {

// One partition with tasks of at most `cap` entry-equivalents: round_of, tcols and n_rounds of part.
void partition_with(uint32_t cap, const Elimination& E, Partition& part) {
  const int n = E.n;
  std::vector<int32_t>& round_of = part.round_of;
  std::vector<TaskCols>& tcols = part.tcols;
  std::fill(round_of.begin(), round_of.end(), -1);
  tcols.clear();
  std::vector<uint32_t> w(n), W(n);
  for (int j = 0; j < n; ++j) {
    // LDS cost in "entry equivalents" (~32 B): the column's entries plus the
    // update pairs it generates (8 B each), wherever those end up being stored
    const uint32_t c = static_cast<uint32_t>(E.Lcol[j].size());
    // (+1 entry and +c pairs for the right-hand-side row, see number_entries)
    w[j] = (c + 2) + (c * (c + 1) / 2 + c + 3) / 4;
    if (w[j] > cap)
      throw std::runtime_error("ldlt: a single column exceeds the LDS task budget "
                               "(global-memory supernode path not built yet)");
  }
  int assigned = 0, round = 0;
  while (assigned < n) {
    for (int j = 0; j < n; ++j) {
      if (round_of[j] >= 0) continue;
      W[j] = w[j];
      for (int32_t c : E.children[j])
        if (round_of[c] < 0) W[j] = std::min<uint64_t>(uint64_t(W[j]) + W[c], 0xffffffffu);
    }
    // unit roots: unassigned j with W <= cap whose parent is assigned-later or too heavy
    TaskCols cur;
    cur.round = round;
    std::vector<int32_t> stack;
    std::vector<int32_t> newly;
    for (int j = n - 1; j >= 0; --j) {  // visit roots before descendants
      if (round_of[j] >= 0 || W[j] > cap) continue;
      int32_t p = E.parent[j];
      if (p >= 0 && round_of[p] < 0 && W[p] <= cap) continue;  // inside a bigger unit
      // collect the unassigned subtree of j
      std::vector<int32_t> unit;
      stack.push_back(j);
      while (!stack.empty()) {
        int32_t v = stack.back();
        stack.pop_back();
        unit.push_back(v);
        for (int32_t c : E.children[v])
          if (round_of[c] < 0) stack.push_back(c);
      }
      if (cur.weight + W[j] > cap && !cur.cols.empty()) {
        tcols.push_back(std::move(cur));
        cur = TaskCols{};
        cur.round = round;
      }
      cur.weight += W[j];
      cur.cols.insert(cur.cols.end(), unit.begin(), unit.end());
      newly.insert(newly.end(), unit.begin(), unit.end());
    }
    if (!cur.cols.empty()) tcols.push_back(std::move(cur));
    if (newly.empty()) throw std::runtime_error("ldlt: task partition made no progress");
    for (int32_t v : newly) round_of[v] = round;
    assigned += static_cast<int>(newly.size());
    ++round;
  }
  part.n_rounds = round;
}

}  // namespace

// ---- tasks: subtrees that fit in LDS, grouped in rounds -------------------------
Partition partition_tasks(const Elimination& E, const LdltOptions& asked, LdltOptions& used) {
  used = asked;
  Partition part;
  part.task_of.assign(E.n, -1);
  part.round_of.assign(E.n, -1);
  partition_with(used.task_entries, E, part);
  if (used.single_problem_task_rules) {
    const size_t first_pass = part.tcols.size();
    if (used.chain_from_deepest_child && used.chain_from_deepest_min_round == 0 && first_pass > 250)
      used.chain_from_deepest_min_round = 1;  // (read by form_supernodes: no new partition for it)
    if (used.task_entries == LdltOptions{}.task_entries && first_pass > 400) {
      used.task_entries *= 2;
      partition_with(used.task_entries, E, part);
    }
  }
  for (int t = 0; t < part.ntasks(); ++t)
    for (int32_t j : part.tcols[t].cols) part.task_of[j] = t;
  return part;
}

// ---- supernodes: chains of the etree inside one task whose columns share their structure ----
// (|struct(L_j)| = |struct(L_parent)| + 1 makes the two structures equal up to the parent
// itself, since struct(L_j) \ {parent} is always contained in struct(L_parent).)  A column
// may have any number of other children: they just have to sit in lower levels.
void form_supernodes(const Elimination& E, const LdltOptions& opt, Partition& part, LdltPlan& P) {
  const int n = E.n, ntasks = part.ntasks();
  const std::vector<int32_t>& task_of = part.task_of;
  const std::vector<std::vector<int32_t>>& Lcol = E.Lcol;
  std::vector<int32_t>&sn_of = part.sn_of, &sn_pos = part.sn_pos;
  std::vector<std::vector<int32_t>>& sn_cols = part.sn_cols;
  sn_of.assign(n, -1);
  sn_pos.assign(n, 0);
  // A column joins its parent's chain only from the DEEPEST side (opt.chain_from_deepest_child): a chain is one
  // front, scheduled after every child subtree of all its columns — a child k whose sibling subtree is as deep
  // as its own would otherwise put its pivots on the critical path behind that sibling, where alone it runs a
  // level earlier, beside it (seen at the ends of a dissected transcription: two separators of the same
  // structure in one front of 9, 1.4 us of the round's 6).  From round chain_from_deepest_min_round up: in the
  // leaf tasks, whose levels are full of fronts anyway, more and smaller fronts only cost tables and arena
  // (cart-pole N=5000 no longer fit two workgroups per CU).  depth = columns on the longest path of the
  // elimination tree below and including a column, inside its task.
  std::vector<int32_t> col_depth(n, 1);
  for (int j = 0; j < n; ++j)
    for (int32_t c : E.children[j])
      if (task_of[c] == task_of[j]) col_depth[j] = std::max(col_depth[j], col_depth[c] + 1);
  auto joins_from_deepest_side = [&](int32_t k, int32_t p) {
    if (!opt.chain_from_deepest_child || part.round_of[p] < opt.chain_from_deepest_min_round) return true;
    for (int32_t c : E.children[p])
      if (c != k && task_of[c] == task_of[p] && col_depth[c] >= col_depth[k]) return false;
    return true;
  };
  // column p may follow column k in the chain that starts at j and has `len` columns so far
  auto extends = [&](int32_t j, int32_t k, int32_t p, size_t len) {
    // rows of the trapezoid after adding p: chain + struct(L_p) + rhs row
    return p >= 0 && task_of[p] == task_of[j] && sn_of[p] < 0 && Lcol[k].size() == Lcol[p].size() + 1 &&
           len + 1 + Lcol[p].size() + 1 <= opt.max_front_rows && joins_from_deepest_side(k, p);
  };
  for (int j = 0; j < n; ++j) {
    if (sn_of[j] >= 0 || sn_of[j] == -2) continue;
    std::vector<int32_t> chain{j};
    sn_of[j] = static_cast<int32_t>(sn_cols.size());
    int32_t k = j;
    // A chain longer than the widest supernode is cut into pieces of (nearly) EQUAL width — nine columns
    // as 5 + 4, not 8 + 1: the dense pass of a front costs more than linearly in its width
    // (profiles/r04_microbench_front.txt), and the one-column tail was a level of its own.
    uint32_t cap = opt.max_supernode_width;
    if (opt.supernodal && opt.balance_supernode_cuts) {
      uint32_t len = 1;
      for (int32_t q = j; extends(j, q, E.parent[q], len); q = E.parent[q]) ++len;
      const uint32_t pieces = (len + opt.max_supernode_width - 1) / opt.max_supernode_width;
      cap = (len + pieces - 1) / pieces;
    }
    while (opt.supernodal && chain.size() < cap) {
      const int32_t p = E.parent[k];
      if (!extends(j, k, p, chain.size())) break;
      sn_of[p] = sn_of[j];
      sn_pos[p] = static_cast<int32_t>(chain.size());
      chain.push_back(p);
      k = p;
    }
    if (chain.size() > 1 && static_cast<int>(chain.size()) < opt.min_supernode_width) {
      // not worth a dense pass: back to single columns
      for (size_t i = 1; i < chain.size(); ++i) {
        sn_of[chain[i]] = -2;  // claimed by nobody; gets its own (lone) supernode below
        sn_pos[chain[i]] = 0;
      }
      chain.resize(1);
    }
    sn_cols.push_back(std::move(chain));
  }
  for (int j = 0; j < n; ++j)
    if (sn_of[j] == -2) {
      sn_of[j] = static_cast<int32_t>(sn_cols.size());
      sn_cols.push_back({j});
    }
  P.n_supernodes = static_cast<int>(sn_cols.size());
  for (auto& c : sn_cols) {
    P.widest_supernode = std::max<int>(P.widest_supernode, static_cast<int>(c.size()));
    if (P.sn_width_hist.size() <= c.size()) P.sn_width_hist.resize(c.size() + 1, 0);
    ++P.sn_width_hist[c.size()];
  }
  // level of a supernode = 1 + the deepest supernode among the other children of its columns
  // (columns ascending: a child outside the chain ends its own chain, so that one is final)
  std::vector<int32_t>&tlevel = part.tlevel, &lcol = part.lcol;
  tlevel.assign(n, 0);
  lcol.assign(n, -1);
  {
    std::vector<int32_t> snlevel(sn_cols.size(), 0);
    for (int j = 0; j < n; ++j)
      for (int32_t c : E.children[j])
        if (task_of[c] == task_of[j] && sn_of[c] != sn_of[j])
          snlevel[sn_of[j]] = std::max(snlevel[sn_of[j]], snlevel[sn_of[c]] + 1);
    for (int j = 0; j < n; ++j) tlevel[j] = snlevel[sn_of[j]];
  }
  for (int t = 0; t < ntasks; ++t) {
    auto& cols = part.tcols[t].cols;
    // within a level: supernodes by width (the lanes finishing them run width-specific code),
    // a supernode's columns consecutive and ascending
    std::sort(cols.begin(), cols.end(), [&](int32_t a, int32_t b) {
      if (tlevel[a] != tlevel[b]) return tlevel[a] < tlevel[b];
      if (sn_of[a] != sn_of[b]) {
        const int32_t wa = part.sn_width(a), wb = part.sn_width(b);
        return wa != wb ? wa < wb : sn_cols[sn_of[a]][0] < sn_cols[sn_of[b]][0];
      }
      return a < b;
    });
    for (size_t i = 0; i < cols.size(); ++i) lcol[cols[i]] = static_cast<int32_t>(i);
  }
}

namespace {

// SLPX_LDLT_VERBOSE, per round: tasks, levels, supernodes (w >= 2) per level, rows per level
void print_round_stats(const LdltPlan& P) {
  for (int r = 0; r < P.n_rounds; ++r) {
    std::vector<int> hist(9, 0);
    uint32_t max_sn = 0, max_rows = 0, lvls = 0, ntask = P.round_ptr[r + 1] - P.round_ptr[r];
    double sum_sn = 0, sum_ent = 0;
    for (uint32_t ti = P.round_ptr[r]; ti < P.round_ptr[r + 1]; ++ti) {
      const LdltTask& T = P.tasks[ti];
      for (uint32_t l = 0; l < T.n_lvl; ++l) {
        const uint32_t ns = P.sn_lvl_ptr[T.lvl_off + l + 1] - P.sn_lvl_ptr[T.lvl_off + l];
        uint32_t ni = 0;
        for (uint32_t q = P.sn_lvl_ptr[T.lvl_off + l]; q < P.sn_lvl_ptr[T.lvl_off + l + 1]; ++q) ni += P.sn_desc[T.sn_off + q].nr;
        const uint32_t ne = P.lvl_ptr[T.lvl_off + l + 1] - P.lvl_ptr[T.lvl_off + l];
        max_sn = std::max(max_sn, ns);
        max_rows = std::max(max_rows, ni);
        sum_sn += ns;
        sum_ent += ne;
        ++lvls;
        ++hist[std::min<uint32_t>(8, (ns + 3) / 4)];
      }
    }
    {
      // update blocks for the parents: how many entries per task, how long their pair lists,
      // and how many update slots an entry of this round's tasks takes from its children
      double ext = 0, ext_pairs = 0, own_pairs = 0, own_ent = 0, takes = 0, takers = 0;
      uint32_t ext_max = 0, take_max = 0;
      for (uint32_t ti = P.round_ptr[r]; ti < P.round_ptr[r + 1]; ++ti) {
        const LdltTask& T = P.tasks[ti];
        ext += T.n_ext;
        ext_max = std::max(ext_max, T.n_ext);
        const uint32_t* pp = P.ent_pair_ptr.data() + T.pair_ptr_off;
        ext_pairs += pp[T.n_ent + T.n_ext] - pp[T.n_ent];
        own_pairs += pp[T.n_ent];
        own_ent += T.n_ent;
        const uint32_t* cp = P.ent_contrib_ptr.data() + T.contrib_ptr_off;
        for (uint32_t i = 0; i < T.n_ent; ++i)
          if (cp[i + 1] > cp[i]) {
            takes += cp[i + 1] - cp[i];
            takers += 1;
            take_max = std::max(take_max, cp[i + 1] - cp[i]);
          }
      }
      std::fprintf(stderr,
                   "ldlt round %d: update entries/task avg %.0f max %u, pairs per update entry %.1f, pairs per own entry "
                   "%.1f; entries taking update slots/task %.0f, slots per such entry avg %.1f max %u\n",
                   r, ext / ntask, ext_max, ext > 0 ? ext_pairs / ext : 0.0, own_pairs / std::max(1.0, own_ent),
                   takers / ntask, takers > 0 ? takes / takers : 0.0, take_max);
    }
    std::fprintf(stderr, "ldlt round %d: %u tasks, %.1f levels/task, chains(w>=2)/level avg %.1f max %u, chain rows/level max %u, entries/level avg %.0f; chains/level hist (0,1-4,5-8,...,>=29):",
                 r, ntask, double(lvls) / ntask, sum_sn / lvls, max_sn, max_rows, sum_ent / lvls);
    for (int h : hist) std::fprintf(stderr, " %d", h);
    std::fprintf(stderr, "\n");
  }
}

}  // namespace

}  // namespace ldlt_detail

static LdltPlan build_ldlt_plan_once(const CscPattern& lower, int n_dec, const LdltOptions& opt_in,
                                     const std::vector<int32_t>* user_perm,
                                     const std::vector<uint8_t>* diag_has_source) {
  using namespace ldlt_detail;
  LdltPlan P;
  const int n = lower.cols;
  P.n = n;
  P.n_dec = n_dec;
  Elimination E;
  E.n = n;
  E.has_diag.assign(n, 0);
  for (int i = 0; i < n; ++i)
    E.has_diag[i] = diag_has_source ? (*diag_has_source)[i] : static_cast<uint8_t>(i < n_dec);

  SetupLap lap;
  order_columns(lower, opt_in, user_perm, E, lap);
  lap("  ldlt: ordering (nested dissection)");
  permute_matrix(lower, E);
  pattern_and_etree(E);
  lap("  ldlt: pattern of L, elimination tree");
  relax_supernodes(opt_in, E);
  P.etree_height = store_pattern(E);
  lap("  ldlt: relaxed supernodes");
  LdltOptions opt;  // opt_in, but for what single_problem_task_rules changes after the first task partition
  Partition part = partition_tasks(E, opt_in, opt);
  P.n_rounds = part.n_rounds;
  lap("  ldlt: tasks and rounds");
  form_supernodes(E, opt, part, P);
  lap("  ldlt: supernodes, levels");
  const Entries ent = number_entries(E, part);
  const PairLists pairs = build_pair_lists(E, part, ent);
  P.n_contrib = pairs.n_contrib;
  lap("  ldlt: entries, pair lists");
  const SolveLists solve = build_solve_lists(E, part);
  P.n_scontrib = solve.n_scontrib;
  lap("  ldlt: solve lists");
  sort_tasks_by_round(part, P);
  std::vector<LdltPlan> flat = flatten_tasks(E, part, ent, pairs, solve, n_dec);
  const size_t n_real_pairs = join_tasks(flat, P);
  flat = {};
  lap("  ldlt: flattened plan arrays");
  if (opt.multifrontal) build_fronts(E, part, ent, opt, P);
  lap("  ldlt: fronts and their tables");

  // structural zero pivots of the unregularized matrix: a diagonal of the (2,2)
  // block (no lhs source other than the forced 0) that no earlier column updates
  for (int j = 0; j < n; ++j)
    if (!E.has_diag[E.perm[j]] && !E.diag_updated_exact[j]) P.structurally_singular_unregularized = true;
  if (E.ordering_forced) P.structurally_singular_unregularized = true;
  pad_plan_tails(P, false);  // (the staged kernels read whole 16-byte groups)
  if (std::getenv("SLPX_LDLT_VERBOSE")) print_round_stats(P);
  for (int r = 0; r < P.n_rounds; ++r) {
    uint32_t deepest = 0;
    for (uint32_t ti = P.round_ptr[r]; ti < P.round_ptr[r + 1]; ++ti) deepest = std::max(deepest, P.tasks[ti].n_lvl);
    P.critical_levels += static_cast<int>(deepest);
  }
  if (std::getenv("SLPX_LDLT_VERBOSE")) std::fprintf(stderr, "ldlt LDS: factor %u bytes, solve %u bytes\n", P.factor_lds_bytes, P.solve_lds_bytes);
  if (P.factor_lds_bytes > 160u * 1024u || P.solve_lds_bytes > 160u * 1024u)
    throw std::runtime_error("ldlt: a task's working set exceeds the 160 KB LDS of a CU; lower "
                             "LdltOptions::task_entries");
  P.perm = std::move(E.perm);
  P.iperm = std::move(E.iperm);
  P.parent = std::move(E.parent);
  P.Lp = std::move(E.Lp);
  P.Li = std::move(E.Li);
  P.nnzL = E.nnzL;
  P.flops = 2 * static_cast<int64_t>(n_real_pairs);
  P.factor_bytes = 12LL * lower.nnz() + 16LL * (P.nnzL + n);
  P.solve_bytes = 32LL * P.nnzL + 16LL * n;
  return P;
}

bool ldlt_plan_error_is_too_big(const std::exception& e) {
  const std::string what = e.what();
  return what.find("exceeds the LDS task budget") != std::string::npos || what.find("exceeds the 160 KB LDS") != std::string::npos ||
         what.find("exceeds 16-bit local indexing") != std::string::npos;
}

LdltPlan build_dense_ldlt_plan(const CscPattern& lower, int n_dec) {
  LdltPlan P;
  const int n = lower.cols;
  P.n = n;
  P.n_dec = n_dec;
  P.dense = true;
  P.perm.resize(n);
  std::iota(P.perm.begin(), P.perm.end(), 0);
  P.iperm = P.perm;
  P.parent.assign(n, -1);
  for (int j = 0; j + 1 < n; ++j) P.parent[j] = j + 1;
  P.nnzL = static_cast<int64_t>(n) * (n - 1) / 2;
  P.Lp.assign(n + 1, 0);
  for (int j = 0; j < n; ++j) P.Lp[j + 1] = P.Lp[j] + (n - 1 - j);
  P.Li.reserve(static_cast<size_t>(P.nnzL));
  for (int j = 0; j < n; ++j)
    for (int i = j + 1; i < n; ++i) P.Li.push_back(i);
  P.etree_height = n;
  P.n_rounds = 0;
  P.round_ptr.assign(1, 0);
  P.n_supernodes = n;
  P.critical_levels = n;
  // (the padding the uploads and the staged kernels' 16-byte reads expect of every plan)
  ldlt_detail::pad_plan_tails(P, true);
  ldlt_detail::pad_front_tails(P);
  // the traffic of a dense factorization and of its two triangular solves
  P.factor_bytes = 12LL * lower.nnz() + 16LL * (P.nnzL + n);
  P.solve_bytes = 32LL * P.nnzL + 16LL * n;
  P.flops = static_cast<int64_t>(n) * n * n / 3;
  return P;
}

LdltPlan build_ldlt_plan(const CscPattern& lower, int n_dec, const LdltOptions& opt,
                         const std::vector<int32_t>* user_perm,
                         const std::vector<uint8_t>* diag_has_source) {
  auto too_big = [](const std::runtime_error& e) { return ldlt_plan_error_is_too_big(e); };
  try {
    return build_ldlt_plan_once(lower, n_dec, opt, user_perm, diag_has_source);
  } catch (const std::runtime_error& e) {
    if (!too_big(e)) throw;
  }
  // A column that does not fit a task is usually the work of a few well-connected nodes the
  // default rule did not take for hubs: once more with a sharper rule; then with bigger tasks
  // (a column of c entries needs about c^2 / 8 entry-equivalents: 2048 hold c = 124, 5120 c = 198;
  // beyond that the factor is dense enough for the reference's dense branch).
  LdltOptions sharper = opt;
  if (user_perm == nullptr || user_perm->empty()) {
    sharper.hub_factor = 2.0;
    sharper.hub_floor = 12;
  }
  for (uint32_t entries : {std::max<uint32_t>(opt.task_entries, LdltOptions{}.task_entries), 4096u, 5120u}) {
    if (entries < opt.task_entries) continue;
    sharper.task_entries = entries;
    try {
      return build_ldlt_plan_once(lower, n_dec, sharper, user_perm, diag_has_source);
    } catch (const std::runtime_error& e) {
      if (!too_big(e) || entries == 5120u) throw;
    }
  }
  throw std::runtime_error("ldlt: no plan");  // not reached
}

}  // namespace slpx
