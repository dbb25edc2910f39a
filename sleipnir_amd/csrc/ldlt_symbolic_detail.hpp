// Internal to the symbolic LDLᵀ (ldlt_order.cpp, ldlt_symbolic.cpp, ldlt_lists.cpp, ldlt_fronts.cpp; included by
// nothing else): what the phases of build_ldlt_plan hand each other, and the phases themselves.  A phase reads what it
// takes by const reference and fills what it returns or takes by reference — the LdltPlan it is given only as output.
#pragma once

#include <utility>

#include "ldlt_symbolic.hpp"
#include "setup_timing.hpp"

namespace slpx::ldlt_detail {

// ---- the elimination structure: ordering, permuted matrix, pattern of L, elimination tree ------------------------
struct Elimination {
  int n = 0;
  std::vector<uint8_t> has_diag;     // by ORIGINAL index: the unregularized diagonal entry has a source
  std::vector<int32_t> perm, iperm;  // perm[new] = old
  bool ordering_forced = false;      // some zero-diagonal node was eliminated without a partner
  // permuted A: per column the strictly-lower (row, index into lhs), rows ascending; the diagonal's index or -1
  std::vector<std::vector<std::pair<int32_t, int32_t>>> Acol;
  std::vector<int32_t> diag_src;
  std::vector<int32_t> parent;                  // elimination tree
  std::vector<std::vector<int32_t>> children;   // ... its children lists, ascending
  std::vector<std::vector<int32_t>> Lcol;       // strictly-lower rows of every column of L, ascending (relaxed: with explicit zeros)
  std::vector<uint8_t> diag_updated_exact;      // d_j receives an update in the EXACT structure of L
  std::vector<int32_t> Lp, Li;                  // Lcol as CSC (store_pattern)
  int64_t nnzL = 0;
};

// ---- the partition: tasks and rounds, supernodes, levels and local column numbers inside a task --------------------
struct TaskCols {
  std::vector<int32_t> cols;  // as collected; in local order (level, supernode, column) after form_supernodes
  uint32_t weight = 0;
  int round = 0;
};
struct Partition {
  int n_rounds = 0;
  std::vector<int32_t> task_of, round_of;  // per column
  std::vector<TaskCols> tcols;
  // form_supernodes:
  std::vector<int32_t> sn_of, sn_pos;         // per column: its supernode, its position in that chain
  std::vector<std::vector<int32_t>> sn_cols;  // per supernode: its columns, ascending
  std::vector<int32_t> tlevel, lcol;          // per column: level inside its task, local column index
  // sort_tasks_by_round:
  std::vector<int> torder;                    // tasks in plan order (by round, stable)
  int ntasks() const { return static_cast<int>(tcols.size()); }
  int32_t sn_width(int32_t j) const { return static_cast<int32_t>(sn_cols[sn_of[j]].size()); }
};

// ---- the entry numbering: local entry index of every diagonal, every L position and every rhs-row entry ----------
struct Entries {
  std::vector<uint32_t> diag_ent, lent, bent;       // per column, per position of Li, per column
  std::vector<uint32_t> task_nent, task_ent_base;   // global entry = task_ent_base[t] + local entry
  uint32_t total() const { return task_ent_base.back(); }
};

// ---- the pair lists, flat: per global entry, per pseudo entry (= slot of the contribution buffer) ------------------
struct PairLists {
  uint32_t n_contrib = 0;
  std::vector<uint32_t> own_ptr;        // per global entry (+1) into own_pairs
  std::vector<LdltPair> own_pairs;
  std::vector<uint32_t> extp_ptr;       // per slot (+1) into extp
  std::vector<LdltPair> extp;
  std::vector<uint32_t> task_ext_ptr, task_ext;  // the slots a task writes, ascending
  std::vector<uint32_t> ec_ptr, ec;              // the slots a global entry takes
};

// ---- the solve lists, flat: per column, per pseudo row (= slot of the solve's contribution buffer) ------------------
struct SolveLists {
  uint32_t n_scontrib = 0;
  std::vector<uint32_t> fwd_all_ptr, bwd_all_ptr;  // per column (+1)
  std::vector<LdltSolveItem> fwd_all, bwd_all;
  std::vector<uint32_t> sext_item_ptr;             // per slot (+1) into sext_item
  std::vector<LdltSolveItem> sext_item;
  std::vector<uint32_t> task_sext_ptr, task_sext;  // the slots a task writes
  std::vector<uint32_t> fc_ptr, fc;                // the slots a row takes
};

// ---- the phases, in the order build_ldlt_plan_once runs them -----------------------------------------------------
// ldlt_order.cpp: fills perm, iperm and ordering_forced of E from E.n, E.has_diag (laps: adjacency, hubs, dissect)
void order_columns(const CscPattern& lower, const LdltOptions& opt, const std::vector<int32_t>* user_perm, Elimination& E,
                   SetupLap& lap);
// ldlt_symbolic.cpp
void permute_matrix(const CscPattern& lower, Elimination& E);   // Acol, diag_src
void pattern_and_etree(Elimination& E);                         // Lcol, parent, children, diag_updated_exact
void relax_supernodes(const LdltOptions& opt, Elimination& E);  // Lcol with explicit zeros
int store_pattern(Elimination& E);                              // Lp, Li, nnzL; returns the height of the elimination tree
// `used` = `asked`, but for what single_problem_task_rules changes after the first partition
Partition partition_tasks(const Elimination& E, const LdltOptions& asked, LdltOptions& used);
// sn_*, tlevel, lcol, the local order of tcols[t].cols; P: n_supernodes, widest_supernode, sn_width_hist
void form_supernodes(const Elimination& E, const LdltOptions& opt, Partition& part, LdltPlan& P);
// ldlt_lists.cpp
Entries number_entries(const Elimination& E, const Partition& part);
PairLists build_pair_lists(const Elimination& E, const Partition& part, const Entries& ent);
SolveLists build_solve_lists(const Elimination& E, const Partition& part);
void sort_tasks_by_round(Partition& part, LdltPlan& P);  // part.torder; P.round_ptr (from P.n_rounds)
// every task's slices of the per-task arrays in a plan of its own, plan order
std::vector<LdltPlan> flatten_tasks(const Elimination& E, const Partition& part, const Entries& ent, const PairLists& pairs,
                                    const SolveLists& solve, int n_dec);
// the per-task arrays, tasks and LDS sizes of P from `flat`; returns the number of update pairs
size_t join_tasks(const std::vector<LdltPlan>& flat, LdltPlan& P);
// 16 pad elements behind every per-task array the kernels stage with 16-byte reads (`all`: behind every one)
void pad_plan_tails(LdltPlan& P, bool all);
// ldlt_fronts.cpp: the mf_* members of P (P.tasks, the joined per-task arrays and the counts are read); P.mf = false
// where the fronts cannot be built
void build_fronts(const Elimination& E, const Partition& part, const Entries& ent, const LdltOptions& opt, LdltPlan& P);
void pad_front_tails(LdltPlan& P);  // 16 pad elements behind every front array

}  // namespace slpx::ldlt_detail
