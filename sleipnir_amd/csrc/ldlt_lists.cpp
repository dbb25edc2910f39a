// Symbolic LDLᵀ, the lists: entry numbering, pair lists, solve lists, and the per-task arrays of the plan — every
// task's slices first (flatten_tasks), then joined in plan order (join_tasks).
#include "ldlt_symbolic_detail.hpp"

#include "setup_threads.hpp"

#include <algorithm>
#include <atomic>
#include <numeric>
#include <stdexcept>
#include <tuple>

namespace slpx::ldlt_detail {

namespace {

struct SlotTable {  // open addressing, key = receiving entry (global)
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals;
  size_t used = 0, mask = 0;
  SlotTable() { grow(1u << 10); }
  void clear() {
    std::fill(keys.begin(), keys.end(), ~0ull);
    used = 0;
  }
  void grow(size_t cap) {
    std::vector<uint64_t> ok;
    std::vector<uint32_t> ov;
    ok.swap(keys);
    ov.swap(vals);
    keys.assign(cap, ~0ull);
    vals.assign(cap, 0);
    mask = cap - 1;
    for (size_t i = 0; i < ok.size(); ++i)
      if (ok[i] != ~0ull) *find(ok[i]).second = ov[i];
  }
  static uint64_t mix(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return k;
  }
  // (is new, where its value lives)
  std::pair<bool, uint32_t*> find(uint64_t key) {
    size_t i = mix(key) & mask;
    while (keys[i] != ~0ull && keys[i] != key) i = (i + 1) & mask;
    const bool fresh = keys[i] == ~0ull;
    keys[i] = key;
    return {fresh, &vals[i]};
  }
  uint32_t* insert(uint64_t key, bool& fresh) {
    if (2 * (used + 1) > keys.size()) grow(2 * keys.size());
    auto r = find(key);
    fresh = r.first;
    used += fresh;
    return r.second;
  }
};

struct TaskPairs {
  std::vector<std::pair<uint32_t, LdltPair>> own, ext;  // (local entry | local pseudo entry, pair) as found
  std::vector<uint32_t> ext_target;                     // per local pseudo entry: receiving entry (global)
  std::vector<int32_t> ext_made_at;                     // ... and the column whose pair made it
  std::vector<uint32_t> ext_slot;                       // ... and its number (number_pseudo_entries)
};

// Every pair is found by the task of its column k, the columns of a task in ascending order — the order the
// single pass over all columns found them in, restricted to the task: the tasks in chunks on the setup threads.
std::vector<TaskPairs> find_pairs(const Elimination& E, const Partition& part, const Entries& ent) {
  const int n = E.n, ntasks = part.ntasks();
  std::vector<TaskPairs> tp(ntasks);
  std::vector<int32_t> cols_ptr(ntasks + 1, 0), cols_asc(n);  // the columns of a task, ascending
  for (int k = 0; k < n; ++k) ++cols_ptr[part.task_of[k] + 1];
  for (int t = 0; t < ntasks; ++t) cols_ptr[t + 1] += cols_ptr[t];
  {
    std::vector<int32_t> next(cols_ptr.begin(), cols_ptr.end() - 1);
    for (int k = 0; k < n; ++k) cols_asc[next[part.task_of[k]]++] = k;
  }
  std::atomic<bool> inconsistent{false};
  parallel_chunks(static_cast<size_t>(ntasks), 4, [&](size_t t_begin, size_t t_end, unsigned) {
    SlotTable slots;
    for (size_t tt = t_begin; tt < t_end; ++tt) {
      const int tk = static_cast<int>(tt);
      TaskPairs& T = tp[tt];
      slots.clear();
      for (int32_t ck = cols_ptr[tt]; ck < cols_ptr[tt + 1]; ++ck) {
        const int k = cols_asc[ck];
        const int32_t* rows = E.Li.data() + E.Lp[k];
        const int c = E.Lp[k + 1] - E.Lp[k];
        for (int a = 0; a < c; ++a) {
          const int32_t j = rows[a];  // target column
          const int tj = part.task_of[j];
          const uint32_t ent_jk = ent.lent[E.Lp[k] + a];
          // updates between two columns of one supernode are done in registers (ldlt_kernels.h)
          if (part.sn_of[k] == part.sn_of[j]) continue;
          const uint32_t base_j = ent.task_ent_base[tj];
          auto add_pair = [&](uint32_t target, const LdltPair& pr) {
            if (tk == tj) {
              T.own.emplace_back(target, pr);
            } else {
              bool fresh;
              uint32_t* slot = slots.insert(base_j + target, fresh);
              if (fresh) {
                *slot = static_cast<uint32_t>(T.ext_target.size());
                T.ext_target.push_back(base_j + target);
                T.ext_made_at.push_back(k);
              }
              T.ext.emplace_back(*slot, pr);
            }
          };
          // rhs row: U_b(j) -= U_b(k) · U(j,k) / d_k
          add_pair(ent.bent[j], LdltPair{static_cast<uint16_t>(ent.bent[k]), static_cast<uint16_t>(ent_jk),
                                         static_cast<uint16_t>(part.lcol[k]), 0});
          int32_t q = E.Lp[j];  // walk column j's rows
          for (int b = a; b < c; ++b) {
            const int32_t i = rows[b];
            uint32_t target;
            if (b == a) {
              target = ent.diag_ent[j];
            } else {
              while (q < E.Lp[j + 1] && E.Li[q] != i) ++q;
              if (q >= E.Lp[j + 1]) {
                inconsistent = true;
                return;
              }
              target = ent.lent[q];
            }
            add_pair(target, LdltPair{static_cast<uint16_t>(ent.lent[E.Lp[k] + b]),
                                      static_cast<uint16_t>(ent_jk), static_cast<uint16_t>(part.lcol[k]), 0});
          }
        }
      }
    }
  });
  if (inconsistent) throw std::runtime_error("ldlt: fill pattern inconsistency");
  return tp;
}

}  // namespace

// The right-hand side rides along as one extra ROW of the matrix: factorizing
// [[K, b], [bᵀ, ·]] yields, as the last row of L, exactly z = D⁻¹L⁻¹Pb — the result of
// the forward substitution and the diagonal scaling.  Column j therefore gets one more
// entry U_b(j) = b_j − Σ_k U(j,k)·U_b(k)/d_k, computed at column j's level with the same
// pair/contribution machinery as every other entry, and the forward-solve launches
// disappear from the Newton step (they remain for re-solves with a new rhs).
Entries number_entries(const Elimination& E, const Partition& part) {
  const int ntasks = part.ntasks();
  Entries ent;
  ent.diag_ent.resize(E.n);
  ent.lent.resize(E.nnzL);
  ent.bent.resize(E.n);
  ent.task_nent.assign(ntasks, 0);
  for (int t = 0; t < ntasks; ++t) {
    uint32_t e = 0;
    for (int32_t j : part.tcols[t].cols) {
      ent.diag_ent[j] = e++;
      for (int32_t p = E.Lp[j]; p < E.Lp[j + 1]; ++p) ent.lent[p] = e++;
      ent.bent[j] = e++;
    }
    ent.task_nent[t] = e;
    if (e > 65535u) throw std::runtime_error("ldlt: task exceeds 16-bit local indexing");
  }
  // Entries are numbered globally, task by task: ge = task_ent_base[t] + local entry.
  ent.task_ent_base.assign(ntasks + 1, 0);
  for (int t = 0; t < ntasks; ++t) ent.task_ent_base[t + 1] = ent.task_ent_base[t] + ent.task_nent[t];
  return ent;
}

// Pair lists per entry, pseudo entries (update blocks for other tasks) per task, update slots per receiving
// entry — as flat arrays (nested vectors of vectors were most of this pass: a million small allocations at
// N=5000).  A pseudo entry = (source task, receiving entry), numbered in the order of their first pair OVER ALL
// COLUMNS — also their slot in the contribution buffer: the tasks note the column that made each of theirs, the
// numbers are handed out afterwards by one walk over the columns.
PairLists build_pair_lists(const Elimination& E, const Partition& part, const Entries& ent) {
  const int n = E.n, ntasks = part.ntasks();
  const uint32_t total_ent = ent.total();
  PairLists L;
  std::vector<TaskPairs> tp = find_pairs(E, part, ent);
  // the pseudo entries' numbers: in the order of the columns that made them (within a column: the order its task
  // made them in)
  std::vector<uint32_t> ext_task, ext_target;  // by slot: source task, receiving entry (global)
  {
    std::vector<uint32_t> cursor(ntasks, 0);
    for (int t = 0; t < ntasks; ++t) tp[t].ext_slot.resize(tp[t].ext_target.size());
    for (int k = 0; k < n; ++k) {
      const int t = part.task_of[k];
      TaskPairs& T = tp[t];
      uint32_t& cur = cursor[t];
      while (cur < T.ext_made_at.size() && T.ext_made_at[cur] == k) {
        T.ext_slot[cur] = L.n_contrib++;
        ext_task.push_back(static_cast<uint32_t>(t));
        ext_target.push_back(T.ext_target[cur]);
        ++cur;
      }
    }
  }
  // stable counting sorts: the pairs of an entry / of a pseudo entry in the order they were found — entries of a
  // task are consecutive, the pairs of a pseudo entry all its task's: every task writes its own ranges
  L.own_ptr.assign(total_ent + 1, 0);
  L.extp_ptr.assign(L.n_contrib + 1, 0);
  std::vector<uint64_t> own_base(ntasks + 1, 0);
  for (int t = 0; t < ntasks; ++t) own_base[t + 1] = own_base[t] + tp[t].own.size();
  for (int t = 0; t < ntasks; ++t) {
    const TaskPairs& T = tp[t];
    std::vector<uint32_t> cnt(T.ext_target.size(), 0);
    for (auto& f : T.ext) ++cnt[f.first];
    for (size_t x = 0; x < cnt.size(); ++x) L.extp_ptr[T.ext_slot[x] + 1] = cnt[x];
  }
  for (uint32_t d = 0; d < L.n_contrib; ++d) L.extp_ptr[d + 1] += L.extp_ptr[d];
  L.own_pairs.resize(static_cast<size_t>(own_base[ntasks]));
  L.extp.resize(L.extp_ptr[L.n_contrib]);
  parallel_chunks(static_cast<size_t>(ntasks), 4, [&](size_t t_begin, size_t t_end, unsigned) {
    std::vector<uint32_t> next;
    for (size_t tt = t_begin; tt < t_end; ++tt) {
      TaskPairs& T = tp[tt];
      const uint32_t base = ent.task_ent_base[tt], ne = ent.task_nent[tt];
      next.assign(ne + 1, 0);
      for (auto& f : T.own) ++next[f.first + 1];
      for (uint32_t e = 0; e < ne; ++e) next[e + 1] += next[e];
      const uint32_t first = static_cast<uint32_t>(own_base[tt]);
      for (uint32_t e = 0; e < ne; ++e) L.own_ptr[base + e] = first + next[e];
      for (auto& f : T.own) L.own_pairs[first + next[f.first]++] = f.second;
      next.assign(T.ext_target.size(), 0);
      for (size_t x = 0; x < next.size(); ++x) next[x] = L.extp_ptr[T.ext_slot[x]];
      for (auto& f : T.ext) L.extp[next[f.first]++] = f.second;
      T.own = {};
      T.ext = {};
    }
  });
  L.own_ptr[total_ent] = static_cast<uint32_t>(own_base[ntasks]);
  // the pseudo entries of a task (ascending slot = the order they were made in); the slots an entry takes
  L.task_ext_ptr.assign(ntasks + 1, 0);
  L.task_ext.resize(L.n_contrib);
  L.ec_ptr.assign(total_ent + 1, 0);
  L.ec.resize(L.n_contrib);
  for (uint32_t d = 0; d < L.n_contrib; ++d) {
    ++L.task_ext_ptr[ext_task[d] + 1];
    ++L.ec_ptr[ext_target[d] + 1];
  }
  for (int t = 0; t < ntasks; ++t) L.task_ext_ptr[t + 1] += L.task_ext_ptr[t];
  for (uint32_t e = 0; e < total_ent; ++e) L.ec_ptr[e + 1] += L.ec_ptr[e];
  {
    std::vector<uint32_t> tn(L.task_ext_ptr.begin(), L.task_ext_ptr.end() - 1), en(L.ec_ptr.begin(), L.ec_ptr.end() - 1);
    for (uint32_t d = 0; d < L.n_contrib; ++d) {
      L.task_ext[tn[ext_task[d]]++] = d;
      L.ec[en[ext_target[d]]++] = d;
    }
  }
  return L;
}

// Forward items of a column (same-task columns outside its supernode, then its chain), backward items (its
// column of L), the pseudo rows a task computes for rows of other tasks: (source task, row), numbered in the
// order they are first needed — their slot in the solve's contribution buffer.
SolveLists build_solve_lists(const Elimination& E, const Partition& part) {
  const int n = E.n, ntasks = part.ntasks();
  SolveLists S;
  // rows of L (CSR view): for row i the entries (i,k), k ascending
  std::vector<int32_t> Lrow_ptr(n + 1, 0);
  for (int32_t p = 0; p < E.nnzL; ++p) ++Lrow_ptr[E.Li[p] + 1];
  for (int i = 0; i < n; ++i) Lrow_ptr[i + 1] += Lrow_ptr[i];
  std::vector<std::pair<uint32_t, int32_t>> Lrow(static_cast<size_t>(E.nnzL));  // (lpos, k)
  {
    std::vector<int32_t> next(Lrow_ptr.begin(), Lrow_ptr.end() - 1);
    for (int k = 0; k < n; ++k)
      for (int32_t p = E.Lp[k]; p < E.Lp[k + 1]; ++p) Lrow[next[E.Li[p]]++] = {static_cast<uint32_t>(p), k};
  }
  S.fwd_all_ptr.assign(n + 1, 0);
  S.bwd_all_ptr.assign(n + 1, 0);
  S.fwd_all.reserve(static_cast<size_t>(E.nnzL));
  S.bwd_all.reserve(static_cast<size_t>(E.nnzL));
  std::vector<std::pair<uint32_t, LdltSolveItem>> sext_found;
  std::vector<uint32_t> sext_task, sext_row;  // by slot
  SlotTable sslots;
  for (int j = 0; j < n; ++j) {
    const int tj = part.task_of[j];
    for (int32_t q = Lrow_ptr[j]; q < Lrow_ptr[j + 1]; ++q) {
      const uint32_t lpos = Lrow[q].first;
      const int32_t k = Lrow[q].second;
      const int tk = part.task_of[k];
      LdltSolveItem it{lpos, static_cast<uint32_t>(part.lcol[k])};
      if (tk == tj) {
        if (part.sn_of[k] != part.sn_of[j]) S.fwd_all.push_back(it);  // the chain's own columns follow below
      } else {
        bool fresh;
        uint32_t* slot = sslots.insert((static_cast<uint64_t>(tk) << 32) | static_cast<uint32_t>(j), fresh);
        if (fresh) {
          *slot = S.n_scontrib++;
          sext_task.push_back(static_cast<uint32_t>(tk));
          sext_row.push_back(static_cast<uint32_t>(j));
        }
        sext_found.emplace_back(*slot, it);
      }
    }
    // row j against the earlier columns of its own supernode: the LAST sn_pos[j] items, chain order
    for (int c = 0; c < part.sn_pos[j]; ++c) {
      const int32_t k = part.sn_cols[part.sn_of[j]][c];
      const int32_t* b = E.Li.data() + E.Lp[k];
      const int32_t* e = E.Li.data() + E.Lp[k + 1];
      const int32_t* f = std::lower_bound(b, e, j);
      if (f == e || *f != j) throw std::runtime_error("ldlt: supernode column lacks a chain row");
      S.fwd_all.push_back({static_cast<uint32_t>(f - E.Li.data()), static_cast<uint32_t>(part.lcol[k])});
    }
    S.fwd_all_ptr[j + 1] = static_cast<uint32_t>(S.fwd_all.size());
    for (int32_t p = E.Lp[j]; p < E.Lp[j + 1]; ++p) {
      int32_t i = E.Li[p];
      uint32_t ref = part.task_of[i] == tj ? static_cast<uint32_t>(part.lcol[i])
                                           : (0x80000000u | static_cast<uint32_t>(i));
      S.bwd_all.push_back({static_cast<uint32_t>(p), ref});
    }
    S.bwd_all_ptr[j + 1] = static_cast<uint32_t>(S.bwd_all.size());
  }
  S.sext_item_ptr.assign(S.n_scontrib + 1, 0);
  S.sext_item.resize(sext_found.size());
  for (auto& f : sext_found) ++S.sext_item_ptr[f.first + 1];
  for (uint32_t d = 0; d < S.n_scontrib; ++d) S.sext_item_ptr[d + 1] += S.sext_item_ptr[d];
  {
    std::vector<uint32_t> next(S.sext_item_ptr.begin(), S.sext_item_ptr.end() - 1);
    for (auto& f : sext_found) S.sext_item[next[f.first]++] = f.second;
  }
  sext_found = {};
  S.task_sext_ptr.assign(ntasks + 1, 0);
  S.task_sext.resize(S.n_scontrib);
  S.fc_ptr.assign(n + 1, 0);
  S.fc.resize(S.n_scontrib);
  for (uint32_t d = 0; d < S.n_scontrib; ++d) {
    ++S.task_sext_ptr[sext_task[d] + 1];
    ++S.fc_ptr[sext_row[d] + 1];
  }
  for (int t = 0; t < ntasks; ++t) S.task_sext_ptr[t + 1] += S.task_sext_ptr[t];
  for (int j = 0; j < n; ++j) S.fc_ptr[j + 1] += S.fc_ptr[j];
  {
    std::vector<uint32_t> tn(S.task_sext_ptr.begin(), S.task_sext_ptr.end() - 1), jn(S.fc_ptr.begin(), S.fc_ptr.end() - 1);
    for (uint32_t d = 0; d < S.n_scontrib; ++d) {
      S.task_sext[tn[sext_task[d]]++] = d;
      S.fc[jn[sext_row[d]]++] = d;
    }
  }
  return S;
}

void sort_tasks_by_round(Partition& part, LdltPlan& P) {
  const int ntasks = part.ntasks();
  part.torder.resize(ntasks);
  std::iota(part.torder.begin(), part.torder.end(), 0);
  std::stable_sort(part.torder.begin(), part.torder.end(),
                   [&](int a, int b) { return part.tcols[a].round < part.tcols[b].round; });
  P.round_ptr.assign(P.n_rounds + 1, 0);
  for (int t = 0; t < ntasks; ++t) ++P.round_ptr[part.tcols[t].round + 1];
  for (int r = 0; r < P.n_rounds; ++r) P.round_ptr[r + 1] += P.round_ptr[r];
}

namespace {

// One task's slices, into a plan of its own (the same member names; it starts empty, so every offset of T is
// relative to the task's own slice and join_tasks shifts it).
void flatten_task(int t, const Elimination& E, const Partition& part, const Entries& ent, const PairLists& pairs,
                  const SolveLists& solve, int n_dec, LdltPlan& O) {
  LdltTask T{};
  const auto& cols = part.tcols[t].cols;
  T.round = static_cast<uint32_t>(part.tcols[t].round);
  T.n_col = static_cast<uint32_t>(cols.size());
  T.n_ent = ent.task_nent[t];
  T.n_ext = pairs.task_ext_ptr[t + 1] - pairs.task_ext_ptr[t];
  T.n_sext = solve.task_sext_ptr[t + 1] - solve.task_sext_ptr[t];

  int32_t cur_level = -1;
  uint32_t pair_count = 0, contrib_count = 0, fwd_count = 0, bwd_count = 0, sc_count = 0;
  for (size_t ci = 0; ci < cols.size(); ++ci) {
    const int32_t j = cols[ci];
    if (part.tlevel[j] != cur_level) {
      O.lvl_ptr.push_back(ent.diag_ent[j]);
      O.col_lvl_ptr.push_back(static_cast<uint32_t>(ci));
      O.sn_lvl_ptr.push_back(static_cast<uint32_t>(O.sn_desc.size()));
      cur_level = part.tlevel[j];
    }
    O.col_perm.push_back(static_cast<uint32_t>(j));
    const uint32_t w = static_cast<uint32_t>(part.sn_width(j)), pos = static_cast<uint32_t>(part.sn_pos[j]);
    O.col_sn.push_back(pos | (w << 8));
    if (w >= 2 && pos == 0) {
      // rows of the trapezoid: the chain, the common structure below it, the rhs row
      const uint32_t nr = w + static_cast<uint32_t>(E.Lcol[part.sn_cols[part.sn_of[j]].back()].size()) + 1;
      if (nr > kSnRowsMax) throw std::runtime_error("ldlt: supernode has more rows than a wave has lanes");
      O.sn_desc.push_back(LdltSn{ent.diag_ent[j], static_cast<uint16_t>(w), static_cast<uint16_t>(nr),
                                 static_cast<uint16_t>(ci), 0});
    }
    auto emit_entry = [&](uint32_t le, int32_t src, uint8_t flags, uint32_t out) {
      O.ent_src.push_back(src);
      O.ent_flags.push_back(flags);
      O.ent_col.push_back(static_cast<uint16_t>(ci));
      O.ent_out.push_back(out);
      O.ent_pair_ptr.push_back(pair_count);
      O.ent_contrib_ptr.push_back(contrib_count);
      const uint32_t ge = ent.task_ent_base[t] + le;
      O.pairs.insert(O.pairs.end(), pairs.own_pairs.begin() + pairs.own_ptr[ge], pairs.own_pairs.begin() + pairs.own_ptr[ge + 1]);
      pair_count += pairs.own_ptr[ge + 1] - pairs.own_ptr[ge];
      O.contrib_idx.insert(O.contrib_idx.end(), pairs.ec.begin() + pairs.ec_ptr[ge], pairs.ec.begin() + pairs.ec_ptr[ge + 1]);
      contrib_count += pairs.ec_ptr[ge + 1] - pairs.ec_ptr[ge];
    };
    const bool gamma_kind = E.perm[j] >= n_dec;
    // bit 3: entry of the diagonal block of a supernode with w >= 2 — finished (and written
    // out) by the lanes that work on the supernode, not by the generic passes
    const uint8_t in_block = w >= 2 ? 8 : 0;
    emit_entry(ent.diag_ent[j], E.diag_src[j], static_cast<uint8_t>(1 | (gamma_kind ? 2 : 0) | in_block),
               static_cast<uint32_t>(j));
    // off-diagonal entries: A source by merge with Acol[j]
    const auto& Aj = E.Acol[j];
    size_t ap = 0;
    for (int32_t p = E.Lp[j]; p < E.Lp[j + 1]; ++p) {
      int32_t src = -1;
      while (ap < Aj.size() && Aj[ap].first < E.Li[p]) ++ap;
      if (ap < Aj.size() && Aj[ap].first == E.Li[p]) src = Aj[ap].second;
      // the first w - pos - 1 rows of the column are the later columns of its chain
      const bool block_row = static_cast<uint32_t>(p - E.Lp[j]) + pos + 1 < w;
      emit_entry(ent.lent[p], src, block_row ? in_block : 0, static_cast<uint32_t>(p));
    }
    // rhs-row entry: source = rhs[perm[j]], result z_j = U_b(j)/d_j
    emit_entry(ent.bent[j], E.perm[j], 4, static_cast<uint32_t>(j));
    // solve lists
    O.fwd_ptr.push_back(fwd_count);
    O.fwd_items.insert(O.fwd_items.end(), solve.fwd_all.begin() + solve.fwd_all_ptr[j], solve.fwd_all.begin() + solve.fwd_all_ptr[j + 1]);
    fwd_count += solve.fwd_all_ptr[j + 1] - solve.fwd_all_ptr[j];
    O.fwd_contrib_ptr.push_back(sc_count);
    O.scontrib_idx.insert(O.scontrib_idx.end(), solve.fc.begin() + solve.fc_ptr[j], solve.fc.begin() + solve.fc_ptr[j + 1]);
    sc_count += solve.fc_ptr[j + 1] - solve.fc_ptr[j];
    O.bwd_ptr.push_back(bwd_count);
    O.bwd_items.insert(O.bwd_items.end(), solve.bwd_all.begin() + solve.bwd_all_ptr[j], solve.bwd_all.begin() + solve.bwd_all_ptr[j + 1]);
    bwd_count += solve.bwd_all_ptr[j + 1] - solve.bwd_all_ptr[j];
  }
  O.lvl_ptr.push_back(T.n_ent);
  O.col_lvl_ptr.push_back(T.n_col);
  T.n_lvl = static_cast<uint32_t>(O.lvl_ptr.size() - 1);
  T.n_sn = static_cast<uint32_t>(O.sn_desc.size());
  O.sn_lvl_ptr.push_back(T.n_sn);
  if (O.col_sn.size() != O.col_perm.size() || O.sn_lvl_ptr.size() != O.lvl_ptr.size())
    throw std::runtime_error("ldlt: supernode arrays out of step with the column arrays");
  // pseudo entries continue the pair_ptr array
  for (uint32_t q = pairs.task_ext_ptr[t]; q < pairs.task_ext_ptr[t + 1]; ++q) {
    const uint32_t d = pairs.task_ext[q];
    O.ext_dst.push_back(d);
    O.ent_pair_ptr.push_back(pair_count);
    O.pairs.insert(O.pairs.end(), pairs.extp.begin() + pairs.extp_ptr[d], pairs.extp.begin() + pairs.extp_ptr[d + 1]);
    pair_count += pairs.extp_ptr[d + 1] - pairs.extp_ptr[d];
  }
  O.ent_pair_ptr.push_back(pair_count);
  T.n_pairs = pair_count;
  T.n_fwd_items = fwd_count;
  T.n_bwd_items = bwd_count;
  O.ent_contrib_ptr.push_back(contrib_count);
  T.n_contrib_idx = contrib_count;
  while (O.contrib_idx.size() % 4 != 0) O.contrib_idx.push_back(0);  // 16-byte slices: staged into LDS
  O.fwd_ptr.push_back(fwd_count);
  O.fwd_contrib_ptr.push_back(sc_count);
  O.bwd_ptr.push_back(bwd_count);
  uint32_t sitem = 0;
  for (uint32_t q = solve.task_sext_ptr[t]; q < solve.task_sext_ptr[t + 1]; ++q) {
    const uint32_t d = solve.task_sext[q];
    O.sext_dst.push_back(d);
    O.sext_ptr.push_back(sitem);
    O.sext_items.insert(O.sext_items.end(), solve.sext_item.begin() + solve.sext_item_ptr[d], solve.sext_item.begin() + solve.sext_item_ptr[d + 1]);
    sitem += solve.sext_item_ptr[d + 1] - solve.sext_item_ptr[d];
  }
  O.sext_ptr.push_back(sitem);
  O.max_lds_doubles = T.n_ent + T.n_col;
  O.max_solve_lds_doubles = T.n_col;
  // LDS working sets of the staged kernels (see ldlt_kernels.h for the carve-up)
  auto q = [](uint32_t count, uint32_t per16) { return 16u * ((count + per16 - 1) / per16); };
  O.factor_lds_bytes = q(pair_count, 2) + q(T.n_ent + T.n_ext + 1, 4) + q(T.n_lvl + 1, 4) +
                       q(T.n_ent, 4) + q(T.n_ent, 8) + q(T.n_ent, 16) + q(T.n_ent, 4) +
                       q(T.n_ent + 1, 4) + 8 * T.n_ent + 8 * T.n_col + 32 + q(3 * T.n_sn, 4) + q(T.n_lvl + 1, 4) +
                       q(T.n_contrib_idx, 4);
  const uint32_t items = std::max(fwd_count, bwd_count);
  O.solve_lds_bytes = q(items, 2) + 2 * q(T.n_col + 1, 4) + q(T.n_lvl + 1, 4) + q(T.n_col, 4) +
                      8 * items + 8 * (T.n_col + 1) + 32 + q(T.n_col, 4) + q(3 * T.n_sn, 4) + q(T.n_lvl + 1, 4);
  O.tasks.push_back(T);
  O.flops = 2 * static_cast<int64_t>(pair_count);  // (carries the task's pair count to the join)
}

// The per-task arrays of the plan, once: the member, the alignment of a task's slice in elements (16-byte groups: the
// kernels stage the slices into LDS with unrolled 16-byte loads; 1: read from memory), what the padding holds, and the
// offset of LdltTask that names where the slice starts — nullptr: the array runs in step with the one above it and
// shares its offset.
template <class T> struct PlanArray {
  std::vector<T> LdltPlan::*member;
  size_t align;
  T pad;
  uint32_t LdltTask::*offset;
};
template <class T> PlanArray<T> plan_array(std::vector<T> LdltPlan::*member, size_t align, T pad, uint32_t LdltTask::*offset) {
  return {member, align, pad, offset};
}
const auto kPlanArrays = std::make_tuple(
    plan_array(&LdltPlan::ent_src, 16, int32_t{-1}, &LdltTask::ent_off),
    plan_array(&LdltPlan::ent_flags, 16, uint8_t{0}, nullptr),
    plan_array(&LdltPlan::ent_col, 16, uint16_t{0}, nullptr),
    plan_array(&LdltPlan::ent_out, 16, uint32_t{0}, nullptr),
    plan_array(&LdltPlan::pairs, 2, LdltPair{}, &LdltTask::pair_off),
    plan_array(&LdltPlan::ent_pair_ptr, 4, uint32_t{0}, &LdltTask::pair_ptr_off),
    plan_array(&LdltPlan::ent_contrib_ptr, 4, uint32_t{0}, &LdltTask::contrib_ptr_off),
    plan_array(&LdltPlan::lvl_ptr, 4, uint32_t{0}, &LdltTask::lvl_off),
    plan_array(&LdltPlan::col_lvl_ptr, 4, uint32_t{0}, nullptr),
    plan_array(&LdltPlan::sn_lvl_ptr, 4, uint32_t{0}, nullptr),
    plan_array(&LdltPlan::col_perm, 4, uint32_t{0}, &LdltTask::col_off),
    plan_array(&LdltPlan::col_sn, 4, uint32_t{0}, nullptr),
    plan_array(&LdltPlan::sn_desc, 4, LdltSn{}, &LdltTask::sn_off),  // 12-byte records: four of them are three 16-byte groups
    plan_array(&LdltPlan::fwd_ptr, 4, uint32_t{0}, &LdltTask::colptr_off),
    plan_array(&LdltPlan::fwd_contrib_ptr, 4, uint32_t{0}, nullptr),
    plan_array(&LdltPlan::bwd_ptr, 4, uint32_t{0}, nullptr),
    plan_array(&LdltPlan::fwd_items, 2, LdltSolveItem{}, &LdltTask::fwd_item_off),
    plan_array(&LdltPlan::bwd_items, 2, LdltSolveItem{}, &LdltTask::bwd_item_off),
    plan_array(&LdltPlan::ext_dst, 1, uint32_t{0}, &LdltTask::ext_off),
    plan_array(&LdltPlan::contrib_idx, 1, uint32_t{0}, &LdltTask::contrib_off),
    plan_array(&LdltPlan::scontrib_idx, 1, uint32_t{0}, &LdltTask::scontrib_off),
    plan_array(&LdltPlan::sext_dst, 1, uint32_t{0}, &LdltTask::sext_off),
    plan_array(&LdltPlan::sext_ptr, 1, uint32_t{0}, &LdltTask::sext_ptr_off),
    plan_array(&LdltPlan::sext_items, 1, LdltSolveItem{}, &LdltTask::sext_item_off));
constexpr size_t kNumPlanArrays = std::tuple_size_v<decltype(kPlanArrays)>;

template <class F> void for_each_plan_array(F&& f) {
  std::apply([&](const auto&... a) { (f(a), ...); }, kPlanArrays);
}

}  // namespace

std::vector<LdltPlan> flatten_tasks(const Elimination& E, const Partition& part, const Entries& ent, const PairLists& pairs,
                                    const SolveLists& solve, int n_dec) {
  std::vector<LdltPlan> flat(part.tcols.size());
  parallel_chunks(flat.size(), 4, [&](size_t ti_begin, size_t ti_end, unsigned) {
    for (size_t ti = ti_begin; ti < ti_end; ++ti) flatten_task(part.torder[ti], E, part, ent, pairs, solve, n_dec, flat[ti]);
  });
  return flat;
}

// Where every task's slice of every array starts is known from the slices' lengths, so the arrays are sized once and
// the slices copied in, the tasks in chunks on the setup threads.
size_t join_tasks(const std::vector<LdltPlan>& flat, LdltPlan& P) {
  const size_t nt = flat.size();
  std::vector<std::vector<uint32_t>> offs;  // [array, in the order of kPlanArrays][task]
  offs.reserve(kNumPlanArrays);
  for_each_plan_array([&](const auto& a) {
    std::vector<uint32_t> o(nt);
    size_t off = 0;
    for (size_t ti = 0; ti < nt; ++ti) {
      off = (off + a.align - 1) / a.align * a.align;
      o[ti] = static_cast<uint32_t>(off);
      off += (flat[ti].*a.member).size();
    }
    (P.*a.member).assign(off, a.pad);
    if (a.offset == nullptr && o != offs.back())
      throw std::runtime_error("ldlt: supernode arrays out of step with the column arrays");
    offs.push_back(std::move(o));
  });
  P.tasks.resize(nt);
  parallel_chunks(nt, 4, [&](size_t ti_begin, size_t ti_end, unsigned) {
    for (size_t ti = ti_begin; ti < ti_end; ++ti) {
      const LdltPlan& O = flat[ti];
      LdltTask T = O.tasks.at(0);
      size_t k = 0;
      for_each_plan_array([&](const auto& a) {
        const uint32_t off = offs[k++][ti];
        std::copy((O.*a.member).begin(), (O.*a.member).end(), (P.*a.member).begin() + off);
        if (a.offset != nullptr) T.*a.offset += off;
      });
      P.tasks[ti] = T;
    }
  });
  size_t n_pairs = 0;
  for (const LdltPlan& O : flat) {
    P.max_lds_doubles = std::max(P.max_lds_doubles, O.max_lds_doubles);
    P.max_solve_lds_doubles = std::max(P.max_solve_lds_doubles, O.max_solve_lds_doubles);
    P.factor_lds_bytes = std::max(P.factor_lds_bytes, O.factor_lds_bytes);
    P.solve_lds_bytes = std::max(P.solve_lds_bytes, O.solve_lds_bytes);
    n_pairs += static_cast<size_t>(O.flops / 2);
  }
  return n_pairs;
}

void pad_plan_tails(LdltPlan& P, bool all) {
  for_each_plan_array([&](const auto& a) {
    if (all || a.align > 1) (P.*a.member).insert((P.*a.member).end(), 16, a.pad);
  });
}

}  // namespace slpx::ldlt_detail
