// Symbolic LDLᵀ, the multifrontal plan (LdltFront, ldlt_symbolic.hpp).
// The fronts are an optional accelerator: whatever keeps them from being built — a limit (16-bit reach,
// children per entry) or a structural corner case its consistency checks trip over (MfRefused) — leaves
// P.mf = false and the pair-list plan, which every system has, in charge.
#include "ldlt_symbolic_detail.hpp"

#include "setup_threads.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>

namespace slpx::ldlt_detail {

namespace {

struct MfRefused {
  const char* why;
};

struct Front {
  std::vector<int32_t> cols, R;  // permuted indices, ascending
  int task = 0, level = 0, parent = -1;
  uint32_t nr = 0, n_s = 0, s_base = 0;  // s_base: doubles into the arena
  std::vector<int> kids;
};
struct FrontSet {
  std::vector<Front> fronts;
  std::vector<std::vector<int>> task_fronts;  // per task (partition order): its fronts, level order after level_fronts
};

// what a task's tables are built into before the join
struct TaskOut {
  std::vector<uint32_t> mf_anc, mf_lvl_ptr, mf_ext;
  std::vector<uint16_t> mf_tab;
  std::vector<LdltFront> mf_fronts;
  std::vector<std::pair<uint32_t, uint32_t>> mc_found;  // (receiving entry, global; slot of this task) in slot order
  uint32_t n_slots = 0, n_mfma = 0, max_nch = 0, max_front_rows = 0;
  bool ok = true;
  const char* refused = nullptr;
};
struct Scratch {
  std::vector<uint16_t> cell_vals;  // per front: the children's values of every table cell, `kids` slots a cell
  std::vector<uint8_t> cell_cnt;
  std::vector<uint32_t> to;
};

// the front arrays of the plan: padded behind, emptied when the fronts are refused
template <class F> void for_each_front_array(LdltPlan& P, F&& f) {
  f(P.mf_tab), f(P.mf_ext), f(P.mf_contrib_ptr), f(P.mf_contrib_idx), f(P.mf_cent), f(P.mf_anc), f(P.mf_lvl_ptr), f(P.mf_fronts);
}

// local entry of (row, col) in the task of col; row = -1: the right-hand-side row
uint32_t entry_of(const Elimination& E, const Entries& ent, int32_t row, int32_t col) {
  if (row == col) return ent.diag_ent[col];
  if (row < 0) return ent.bent[col];
  const int32_t* b = E.Li.data() + E.Lp[col];
  const int32_t* e = E.Li.data() + E.Lp[col + 1];
  const int32_t* f = std::lower_bound(b, e, row);
  if (f == e || *f != row) throw MfRefused{"a front's update block has an entry outside the pattern of L"};
  return ent.lent[f - E.Li.data()];
}

// every supernode a front, its parent front inside the task; false: a front beyond what the kernels address
bool collect_fronts(const Elimination& E, const Partition& part, FrontSet& F) {
  const int ntasks = part.ntasks();
  std::vector<Front>& fronts = F.fronts;
  std::vector<int32_t> front_of(E.n, -1);
  F.task_fronts.assign(ntasks, {});
  bool ok = true;
  for (int t = 0; t < ntasks && ok; ++t)
    for (int32_t j : part.tcols[t].cols) {
      if (part.sn_pos[j] != 0) continue;
      Front f;
      f.cols = part.sn_cols[part.sn_of[j]];
      f.R = E.Lcol[f.cols.back()];
      f.task = t;
      f.level = part.tlevel[j];
      f.nr = static_cast<uint32_t>(f.cols.size() + f.R.size() + 1);
      const uint32_t r = static_cast<uint32_t>(f.R.size());
      f.n_s = r * (r + 1) / 2 + r;
      if (f.nr > kSnRowsMax || f.cols.size() > kSnWidthMax || f.n_s > 0xffffu) ok = false;
      for (int32_t c : f.cols) front_of[c] = static_cast<int>(fronts.size());
      F.task_fronts[t].push_back(static_cast<int>(fronts.size()));
      fronts.push_back(std::move(f));
    }
  for (size_t fi = 0; fi < fronts.size() && ok; ++fi) {
    Front& f = fronts[fi];
    const int32_t pc = E.parent[f.cols.back()];
    if (pc >= 0 && part.task_of[pc] == f.task && !f.R.empty()) {
      f.parent = front_of[pc];
      fronts[f.parent].kids.push_back(static_cast<int>(fi));
    }
  }
  return ok;
}

// Levels of the fronts inside their task: 0 .. n_lvl - 1 in step with the column levels, then
// balanced — a level is worked off sixteen fronts at a time (one wave each), and a front whose parent
// sits more than one level up may as well run a level later: fronts with that slack leave levels of
// more than sixteen (cart-pole N=1000: the leaf tasks' passes of sixteen 4..6 -> 4..5) — and inside a
// level the wide fronts first, so that a second pass holds the cheap ones.
void level_fronts(FrontSet& F) {
  std::vector<Front>& fronts = F.fronts;
  for (auto& fl : F.task_fronts) {
    std::vector<int> distinct;
    for (int fi : fl) distinct.push_back(fronts[fi].level);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    const int n_lvl = static_cast<int>(distinct.size());
    for (int fi : fl)
      fronts[fi].level = static_cast<int>(std::lower_bound(distinct.begin(), distinct.end(), fronts[fi].level) - distinct.begin());
    std::vector<int> count(n_lvl, 0);
    for (int fi : fl) ++count[fronts[fi].level];
    for (int l = 0; l + 1 < n_lvl; ++l) {
      if (count[l] <= 16) continue;
      // candidates: cheapest first (they add least to the level they join)
      std::vector<int> cand;
      for (int fi : fl) {
        const Front& f = fronts[fi];
        if (f.level != l) continue;
        const int limit = f.parent >= 0 ? fronts[f.parent].level : n_lvl;  // must stay below
        if (l + 1 < limit) cand.push_back(fi);
      }
      std::sort(cand.begin(), cand.end(), [&](int a, int b) {
        return fronts[a].cols.size() * 64 + fronts[a].R.size() < fronts[b].cols.size() * 64 + fronts[b].R.size();
      });
      for (int fi : cand) {
        if (count[l] <= 16 || count[l + 1] >= 16) break;
        ++fronts[fi].level;
        --count[l];
        ++count[l + 1];
      }
    }
    std::stable_sort(fl.begin(), fl.end(), [&](int a, int b) {
      const Front &fa = fronts[a], &fb = fronts[b];
      if (fa.level != fb.level) return fa.level < fb.level;
      return fa.cols.size() * 64 + fa.R.size() > fb.cols.size() * 64 + fb.R.size();
    });
  }
}

// S blocks of a task's fronts (s_base): a block lives from its front's level to its parent's; first fit over the
// free gaps.  Returns the doubles of the arena: [0] = 0.0, [1] = scratch, the blocks.
uint32_t place_update_blocks(const std::vector<int>& fl, std::vector<Front>& fronts) {
  uint32_t arena = 2;
  struct Blk { uint32_t off, len; int until; };
  std::vector<Blk> live;
  for (int fi : fl) {
    Front& f = fronts[fi];
    if (f.parent < 0 || f.n_s == 0) continue;  // root fronts write to the update slots
    const int lvl = f.level, until = fronts[f.parent].level;
    live.erase(std::remove_if(live.begin(), live.end(), [&](const Blk& b) { return b.until < lvl; }), live.end());
    std::sort(live.begin(), live.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
    uint32_t at = 2;
    for (const Blk& b : live) {
      if (at + f.n_s <= b.off) break;
      at = std::max(at, b.off + b.len);
    }
    f.s_base = at;
    live.push_back({at, f.n_s, until});
    arena = std::max(arena, at + f.n_s);
  }
  return arena;
}

// The tables of the fronts of task t (T, the ti-th of the plan): into O, offsets relative to the task; M: arena, the
// ancestor rows, the counts.  Sets s_base of the task's fronts.  O.ok = false: beyond a limit of the addressing.
void build_task_tables(int t, const LdltTask& T, const Elimination& E, const Partition& part, const Entries& ent,
                       const LdltOptions& opt, FrontSet& F, Scratch& S, LdltMfTask& M, TaskOut& O) {
  std::vector<Front>& fronts = F.fronts;
  const auto& fl = F.task_fronts[t];
  const uint32_t arena = place_update_blocks(fl, fronts);
  M.arena = arena;
  // ---- rows of ancestor tasks the solve reaches
  std::vector<int32_t> anc;
  for (int fi : fl)
    for (int32_t i : fronts[fi].R)
      if (part.task_of[i] != t) anc.push_back(i);
  std::sort(anc.begin(), anc.end());
  anc.erase(std::unique(anc.begin(), anc.end()), anc.end());
  M.anc_off = static_cast<uint32_t>(O.mf_anc.size());
  M.n_anc = static_cast<uint32_t>(anc.size());
  for (int32_t i : anc) O.mf_anc.push_back(static_cast<uint32_t>(i));
  // ---- the 64 KB every table offset must reach
  const uint32_t off_arena = 8u * T.n_ent, off_invd = off_arena + 8u * arena, off_x = off_invd + 8u * T.n_col;
  const uint32_t reach = off_x + 8u * (T.n_col + M.n_anc + 1u);
  if (reach > 0x10000u) {
    O.ok = false;
    return;
  }
  const uint16_t kZero = static_cast<uint16_t>(off_arena), kScratch = static_cast<uint16_t>(off_arena + 8u);
  auto s_addr = [&](const Front& f, uint32_t e) { return static_cast<uint16_t>(off_arena + 8u * (f.s_base + e)); };
  auto u_addr = [&](uint32_t e) { return static_cast<uint16_t>(8u * e); };
  // ---- fronts and their tables
  M.front_off = static_cast<uint32_t>(O.mf_fronts.size());
  M.n_front = static_cast<uint32_t>(fl.size());
  M.tab_off = static_cast<uint32_t>(O.mf_tab.size());
  M.ext_off = static_cast<uint32_t>(O.mf_ext.size());
  int cur_level = -1;
  uint32_t n_ext = 0;
  for (size_t q = 0; q < fl.size(); ++q) {
    const Front& f = fronts[fl[q]];
    if (f.level != cur_level) {
      O.mf_lvl_ptr.push_back(static_cast<uint32_t>(q));
      cur_level = f.level;
    }
    const uint32_t w = static_cast<uint32_t>(f.cols.size()), r = static_cast<uint32_t>(f.R.size()), nr = f.nr;
    const uint32_t base0 = ent.diag_ent[f.cols[0]];
    auto tr = [&](uint32_t c, uint32_t row) { return base0 + c * nr - (c * (c - 1)) / 2 + (row - c); };
    // where the rows of each child land in this front (a child's block has at most one value for a cell:
    // the cells' lists are the children's values in child order)
    const size_t n_kids = f.kids.size(), n_piv = static_cast<size_t>(nr) * w, n_cells = n_piv + f.n_s;
    S.cell_cnt.assign(n_cells, 0);
    if (S.cell_vals.size() < n_cells * n_kids) S.cell_vals.resize(n_cells * n_kids);
    for (int ki : f.kids) {
      const Front& k = fronts[ki];
      const uint32_t rk = static_cast<uint32_t>(k.R.size());
      std::vector<uint32_t>& to = S.to;
      to.resize(rk + 1);
      for (uint32_t a = 0; a < rk; ++a) {
        const int32_t i = k.R[a];
        auto ic = std::lower_bound(f.cols.begin(), f.cols.end(), i);
        if (ic != f.cols.end() && *ic == i) {
          to[a] = static_cast<uint32_t>(ic - f.cols.begin());
        } else {
          auto ir = std::lower_bound(f.R.begin(), f.R.end(), i);
          if (ir == f.R.end() || *ir != i) throw MfRefused{"a child front's row is not in its parent front"};
          to[a] = w + static_cast<uint32_t>(ir - f.R.begin());
        }
      }
      to[rk] = nr - 1;
      for (uint32_t a = 0; a <= rk; ++a)
        for (uint32_t b = 0; b < rk && b <= a; ++b) {
          const uint32_t ta = to[a], tb = to[b];
          const uint16_t src = s_addr(k, a * (a + 1) / 2 + b);
          const size_t cell = tb < w ? static_cast<size_t>(ta) * w + tb : n_piv + (ta - w) * (ta - w + 1) / 2 + (tb - w);
          if (S.cell_cnt[cell] == 255 || S.cell_cnt[cell] >= n_kids) {
            O.ok = false;
            break;
          }
          S.cell_vals[cell * n_kids + S.cell_cnt[cell]++] = src;
        }
    }
    if (!O.ok) break;
    uint32_t nch = 0;
    for (size_t c = 0; c < n_cells; ++c) nch = std::max<uint32_t>(nch, S.cell_cnt[c]);
    auto piv_at = [&](uint32_t row, uint32_t c, uint32_t kk) {
      const size_t cell = static_cast<size_t>(row) * w + c;
      return kk < S.cell_cnt[cell] ? S.cell_vals[cell * n_kids + kk] : kZero;
    };
    auto upd_at = [&](uint32_t e, uint32_t kk) {
      const size_t cell = n_piv + e;
      return kk < S.cell_cnt[cell] ? S.cell_vals[cell * n_kids + kk] : kZero;
    };
    LdltFront D{};
    D.tab = static_cast<uint32_t>(O.mf_tab.size()) - M.tab_off;
    D.base0 = static_cast<uint16_t>(base0);
    D.col0 = static_cast<uint16_t>(part.lcol[f.cols[0]]);
    D.w = static_cast<uint8_t>(w);
    D.nr = static_cast<uint8_t>(nr);
    D.nch = static_cast<uint8_t>(nch);
    D.n_s = static_cast<uint16_t>(f.n_s);
    const bool root = f.parent < 0;
    // the update block on the matrix cores: four pivot columns or more under more entries than two
    // lane-per-entry passes cover (ldlt_mf_kernels.h: mf_update_mfma)
    const bool mfma = w >= 4 && f.n_s > opt.mfma_min_entries;
    D.flags = static_cast<uint8_t>((root ? 1 : 0) | (mfma ? 2 : 0));
    O.n_mfma += mfma;
    D.ext = static_cast<uint16_t>(n_ext);
    if (root && n_ext + f.n_s > 0xffffu) {
      O.ok = false;
      break;
    }
    // pivot table: rows x [k][c]
    for (uint32_t row = 0; row < nr; ++row)
      for (uint32_t k = 0; k <= nch; ++k)
        for (uint32_t c = 0; c < w; ++c) {
          uint16_t v;
          if (k == 0) v = row >= c ? u_addr(tr(c, row)) : kScratch;
          else v = row >= c ? piv_at(row, c, k - 1) : kZero;
          O.mf_tab.push_back(v);
        }
    // update table: out, U(a, 0), U(b, 0), children
    for (uint32_t a = 0; a <= r; ++a)
      for (uint32_t b = 0; b < r && b <= a; ++b) {
        const uint32_t e = a * (a + 1) / 2 + b;
        O.mf_tab.push_back(root ? static_cast<uint16_t>(e) : s_addr(f, e));
        O.mf_tab.push_back(u_addr(tr(0, w + a)));
        O.mf_tab.push_back(u_addr(tr(0, w + b)));
        for (uint32_t k = 0; k < nch; ++k) O.mf_tab.push_back(upd_at(e, k));
        if (root) {
          const int32_t gb = f.R[b], ga = a < r ? f.R[a] : -1;
          const int tj = part.task_of[gb];
          const uint32_t slot = O.n_slots++;
          O.mc_found.emplace_back(ent.task_ent_base[tj] + entry_of(E, ent, ga, gb), slot);
          O.mf_ext.push_back(slot);
          ++n_ext;
        }
      }
    // solve table: x of the rows of R
    for (uint32_t a = 0; a < r; ++a) {
      const int32_t i = f.R[a];
      uint32_t xi;
      if (part.task_of[i] == t) xi = static_cast<uint32_t>(part.lcol[i]);
      else xi = T.n_col + static_cast<uint32_t>(std::lower_bound(anc.begin(), anc.end(), i) - anc.begin());
      O.mf_tab.push_back(static_cast<uint16_t>(off_x + 8u * xi));
    }
    O.mf_fronts.push_back(D);
    O.max_nch = std::max(O.max_nch, nch);
    O.max_front_rows = std::max(O.max_front_rows, nr);
  }
  if (!O.ok) return;
  O.mf_lvl_ptr.push_back(static_cast<uint32_t>(fl.size()));
  if (O.mf_lvl_ptr.size() != T.n_lvl + 1)
    throw MfRefused{"front levels out of step with the column levels"};
  M.n_ext = n_ext;
  M.n_tab = static_cast<uint32_t>(O.mf_tab.size()) - M.tab_off;
}

// The tasks' buffers joined in plan order: offsets, slot numbers and the slots' receiving entries shifted by what came
// before.  Returns (receiving entry, global; slot) in slot order; ok = false at the first task that did not fit (what
// was joined before it stays).
std::vector<std::pair<uint32_t, uint32_t>> join_task_tables(std::vector<TaskOut>& outs, LdltPlan& P, bool& ok) {
  std::vector<std::pair<uint32_t, uint32_t>> mc_found;
  for (size_t ti = 0; ti < P.tasks.size() && ok; ++ti) {
    TaskOut& O = outs[ti];
    if (O.refused != nullptr) throw MfRefused{O.refused};
    if (!O.ok) {
      ok = false;
      break;
    }
    const LdltTask& T = P.tasks[ti];
    LdltMfTask& M = P.mf_tasks[ti];
    M.anc_off = static_cast<uint32_t>(P.mf_anc.size());
    P.mf_anc.insert(P.mf_anc.end(), O.mf_anc.begin(), O.mf_anc.end());
    while (P.mf_anc.size() % 4) P.mf_anc.push_back(0);
    M.front_off = static_cast<uint32_t>(P.mf_fronts.size());
    M.tab_off = static_cast<uint32_t>(P.mf_tab.size());
    M.ext_off = static_cast<uint32_t>(P.mf_ext.size());
    while (P.mf_lvl_ptr.size() < T.lvl_off) P.mf_lvl_ptr.push_back(0);
    P.mf_lvl_ptr.insert(P.mf_lvl_ptr.end(), O.mf_lvl_ptr.begin(), O.mf_lvl_ptr.end());
    if (P.mf_lvl_ptr.size() != T.lvl_off + T.n_lvl + 1) throw MfRefused{"front levels out of step with the column levels"};
    P.mf_fronts.insert(P.mf_fronts.end(), O.mf_fronts.begin(), O.mf_fronts.end());
    P.mf_tab.insert(P.mf_tab.end(), O.mf_tab.begin(), O.mf_tab.end());
    for (uint32_t slot : O.mf_ext) P.mf_ext.push_back(P.mf_n_contrib + slot);
    for (auto& f : O.mc_found) mc_found.emplace_back(f.first, P.mf_n_contrib + f.second);
    P.mf_n_contrib += O.n_slots;
    P.mf_n_mfma += O.n_mfma;
    P.mf_max_nch = std::max(P.mf_max_nch, O.max_nch);
    P.mf_max_front_rows = std::max(P.mf_max_front_rows, O.max_front_rows);
    while (P.mf_tab.size() % 8) P.mf_tab.push_back(0);
    while (P.mf_ext.size() % 4) P.mf_ext.push_back(0);
    O = TaskOut{};
  }
  return mc_found;
}

// update slots per receiving entry (the tasks' entries are numbered in emission order): mf_cent, mf_contrib_ptr,
// mf_contrib_idx of every task
void list_update_slots(const std::vector<std::pair<uint32_t, uint32_t>>& mc_found, const Partition& part, const Entries& ent,
                       bool ok, LdltPlan& P) {
  const uint32_t total_ent = ent.total();
  std::vector<uint32_t> mc_ptr(total_ent + 1, 0), mc(mc_found.size());
  for (auto& f : mc_found) ++mc_ptr[f.first + 1];
  for (uint32_t e = 0; e < total_ent; ++e) mc_ptr[e + 1] += mc_ptr[e];
  {
    std::vector<uint32_t> next(mc_ptr.begin(), mc_ptr.end() - 1);
    for (auto& f : mc_found) mc[next[f.first]++] = f.second;
  }
  for (size_t ti = 0; ti < P.tasks.size() && ok; ++ti) {
    const int t = part.torder[ti];
    LdltMfTask& M = P.mf_tasks[ti];
    while (P.mf_contrib_ptr.size() % 4) P.mf_contrib_ptr.push_back(0);
    while (P.mf_cent.size() % 8) P.mf_cent.push_back(0);
    M.contrib_ptr_off = static_cast<uint32_t>(P.mf_contrib_ptr.size());
    M.contrib_off = static_cast<uint32_t>(P.mf_contrib_idx.size());
    M.cent_off = static_cast<uint32_t>(P.mf_cent.size());
    uint32_t count = 0, n_cent = 0;
    for (uint32_t e = 0; e < ent.task_nent[t]; ++e) {
      const uint32_t ge = ent.task_ent_base[t] + e;
      if (mc_ptr[ge + 1] == mc_ptr[ge]) continue;
      P.mf_cent.push_back(static_cast<uint16_t>(e));
      P.mf_contrib_ptr.push_back(count);
      P.mf_contrib_idx.insert(P.mf_contrib_idx.end(), mc.begin() + mc_ptr[ge], mc.begin() + mc_ptr[ge + 1]);
      count += mc_ptr[ge + 1] - mc_ptr[ge];
      ++n_cent;
    }
    P.mf_contrib_ptr.push_back(count);
    M.n_cent = n_cent;
    M.n_contrib_idx = count;
    while (P.mf_contrib_idx.size() % 4) P.mf_contrib_idx.push_back(0);
  }
}

// SLPX_LDLT_VERBOSE (the front arrays already carry their tail padding)
void print_front_stats(const LdltPlan& P, const std::vector<int32_t>& perm, bool ok) {
  size_t tab = 0, arena = 0;
  for (auto& M : P.mf_tasks) {
    tab = std::max<size_t>(tab, M.n_tab);
    arena = std::max<size_t>(arena, M.arena);
  }
  {
    std::map<std::pair<int, int>, int> hist;
    std::map<int, int> rows;
    for (size_t i = 0; i + 16 < P.mf_fronts.size(); ++i) {
      ++hist[{P.mf_fronts[i].w, P.mf_fronts[i].nch}];
      ++rows[P.mf_fronts[i].nr - P.mf_fronts[i].w - 1];
    }
    std::fprintf(stderr, "ldlt fronts (w, children values per entry): count —");
    for (auto& [k, v] : hist) std::fprintf(stderr, " (%d,%d):%d", k.first, k.second, v);
    std::fprintf(stderr, "\nldlt fronts rows below the pivots: count —");
    for (auto& [k, v] : rows) std::fprintf(stderr, " %d:%d", k, v);
    std::fprintf(stderr, "\n");
  }
  for (int r = 0; r < P.n_rounds && ok; ++r) {
    uint32_t most = 0, over = 0, lv = 0, deepest = 0, most_passes = 0, least_passes = 1u << 30;
    for (uint32_t ti = P.round_ptr[r]; ti < P.round_ptr[r + 1]; ++ti) {
      const LdltTask& T = P.tasks[ti];
      deepest = std::max(deepest, T.n_lvl);
      uint32_t passes = 0;
      for (uint32_t l = 0; l < T.n_lvl; ++l) passes += (P.mf_lvl_ptr[T.lvl_off + l + 1] - P.mf_lvl_ptr[T.lvl_off + l] + 15u) / 16u;
      most_passes = std::max(most_passes, passes);
      least_passes = std::min(least_passes, passes);
      for (uint32_t l = 0; l < T.n_lvl; ++l) {
        const uint32_t nf = P.mf_lvl_ptr[T.lvl_off + l + 1] - P.mf_lvl_ptr[T.lvl_off + l];
        most = std::max(most, nf);
        over += nf > 16;
        ++lv;
      }
    }
    std::fprintf(stderr, "ldlt fronts round %d: deepest task %u levels, most fronts in a level %u, levels with more than 16 fronts %u of %u; passes of 16 waves per task %u..%u\n",
                 r, deepest, most, over, lv, least_passes, most_passes);
  }
  if (const char* lv = std::getenv("SLPX_LDLT_VERBOSE"); lv != nullptr && std::atoi(lv) >= 2) {
    // per task: round, levels, and per level "fronts:widest w" — where the critical path's imbalance sits
    for (size_t ti = 0; ti < P.tasks.size() && ok; ++ti) {
      const LdltTask& T = P.tasks[ti];
      const LdltMfTask& M = P.mf_tasks[ti];
      std::fprintf(stderr, "ldlt task %zu round %u cols %u ents %u anc %u levels %u:", ti, T.round, T.n_col, T.n_ent, M.n_anc, T.n_lvl);
      for (uint32_t l = 0; l < T.n_lvl; ++l) {
        const uint32_t b = P.mf_lvl_ptr[T.lvl_off + l], e = P.mf_lvl_ptr[T.lvl_off + l + 1];
        uint32_t wmax = 0, nchmax = 0, rmax = 0;
        for (uint32_t q = b; q < e; ++q) {
          const LdltFront& F = P.mf_fronts[M.front_off + q];
          wmax = std::max<uint32_t>(wmax, F.w);
          nchmax = std::max<uint32_t>(nchmax, F.nch);
          rmax = std::max<uint32_t>(rmax, F.nr - F.w - 1u);
        }
        std::fprintf(stderr, " %u:w%u,c%u,r%u", e - b, wmax, nchmax, rmax);
      }
      std::fprintf(stderr, "\n");
      if (std::atoi(lv) >= 3 && T.round >= 1)
        for (uint32_t l = 0; l < T.n_lvl; ++l)
          for (uint32_t q = P.mf_lvl_ptr[T.lvl_off + l]; q < P.mf_lvl_ptr[T.lvl_off + l + 1]; ++q) {
            const LdltFront& F = P.mf_fronts[M.front_off + q];
            std::fprintf(stderr, "  level %u front w%u r%u nch%u original columns:", l, F.w, F.nr - F.w - 1u, F.nch);
            for (uint32_t c = 0; c < F.w; ++c) std::fprintf(stderr, " %d", perm[P.col_perm[T.col_off + F.col0 + c]]);
            std::fprintf(stderr, "\n");
          }
    }
  }
  std::fprintf(stderr, "ldlt multifrontal plan: %s, %zu fronts, widest table %zu bytes, largest arena %zu doubles, most children per entry %u, update slots %u (pair plan: %u), fronts on the matrix cores %u\n",
               ok ? "built" : "NOT built", P.mf_fronts.size() - 16, 2 * tab, arena, P.mf_max_nch, P.mf_n_contrib, P.n_contrib, P.mf_n_mfma);
}

}  // namespace

void pad_front_tails(LdltPlan& P) {
  // (the tail padding the staged kernels' 16-byte reads expect)
  for_each_front_array(P, [](auto& v) { v.insert(v.end(), 16, typename std::remove_reference_t<decltype(v)>::value_type{}); });
}

void build_fronts(const Elimination& E, const Partition& part, const Entries& ent, const LdltOptions& opt, LdltPlan& P) {
  try {
    FrontSet F;
    bool ok = collect_fronts(E, part, F);
    if (ok) level_fronts(F);
    // Every task builds its fronts' tables into buffers of its own — the tasks in chunks on the setup threads — and
    // the buffers are joined in plan order afterwards.
    P.mf_tasks.assign(part.ntasks(), LdltMfTask{});
    std::vector<TaskOut> outs(P.tasks.size());
    if (ok)
      parallel_chunks(P.tasks.size(), 4, [&](size_t t_begin, size_t t_end, unsigned) {
        Scratch S;
        for (size_t ti = t_begin; ti < t_end; ++ti) {
          try {
            build_task_tables(part.torder[ti], P.tasks[ti], E, part, ent, opt, F, S, P.mf_tasks[ti], outs[ti]);
          } catch (const MfRefused& r) {
            outs[ti].refused = r.why;
          }
        }
      });
    const auto mc_found = join_task_tables(outs, P, ok);
    list_update_slots(mc_found, part, ent, ok, P);
    P.mf = ok;
    pad_front_tails(P);
    if (std::getenv("SLPX_LDLT_VERBOSE")) print_front_stats(P, E.perm, ok);
  } catch (const MfRefused& refused) {
    // (a consistency check of the fronts tripped: the pair-list plan takes over — a slower step, never a wrong one —
    // and says so once, whatever the verbosity: a defect of the symbolic phase must not hide as a slow-down)
    static std::atomic<bool> warned{false};
    if (!warned.exchange(true) || std::getenv("SLPX_LDLT_VERBOSE"))
      std::fprintf(stderr, "slpx: the multifrontal plan of an order-%d system was refused (%s); the pair-list plan is used\n", E.n, refused.why);
    P.mf = false;
    P.mf_tasks.assign(part.ntasks(), LdltMfTask{});
    P.mf_n_contrib = P.mf_max_nch = P.mf_max_front_rows = P.mf_n_mfma = 0;
    for_each_front_array(P, [](auto& v) { v.clear(); });
    pad_front_tails(P);
  }
}

}  // namespace slpx::ldlt_detail
