// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// csrc/switches.hpp and csrc/system_choice.hpp handed to Python (tests/test_system_choice_cpu.py): the structs as rows
// of integers, named in choicecheck.py.  Nothing is checked here.  The switches are those of the environment at the
// moment of the call, read the way NewtonSystem's constructors read them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>

#include "../../sleipnir_amd/csrc/kkt_plan.hpp"
#include "../../sleipnir_amd/csrc/nlp.hpp"
#include "choicecheck_modes.h"

using namespace slpx;

namespace {
void options_row(const LdltOptions& o, int64_t* out) {
  const int64_t row[] = {o.task_entries, o.supernodal, o.multifrontal, o.min_supernode_width, o.relax_zeros, o.balance_supernode_cuts,
                         o.chain_from_deepest_child, o.chain_from_deepest_min_round, o.single_problem_task_rules, o.mfma_min_entries};
  std::memcpy(out, row, sizeof(row));
}
}  // namespace

extern "C" {

// every member of Switches as (set, value): `set` is 0 only for an empty optional
void cc_switches(int64_t* out) {
  const Switches s = Switches::from_environment();
  auto opt = [](const auto& v, int64_t* o) {
    o[0] = v.has_value();
    o[1] = v ? static_cast<int64_t>(*v) : 0;
  };
  const int64_t plain[] = {s.fuse_launches, s.fuse_kkt, s.fuse_backsub, s.ldlt_mf, s.ldlt_il, s.chain_tape, s.ipm_resident, s.ipm_lookahead,
                           s.ipm_pipeline, s.twin, s.ipm_ride, s.mf_solve, s.fuse_kkt_store, s.il_min_batch};
  int k = 0;
  for (int64_t v : plain) {
    out[k++] = 1;
    out[k++] = v;
  }
  opt(s.dense, out + k), k += 2;
  opt(s.task_entries, out + k), k += 2;
  opt(s.single_launch, out + k), k += 2;
  opt(s.mf_threads, out + k), k += 2;
  opt(s.relax_zeros, out + k), k += 2;
  opt(s.sn_min_width, out + k), k += 2;
  opt(s.mfma_min_entries, out + k), k += 2;
}

int32_t cc_interleaved(int32_t batch) { return interleaved_for(batch, Switches::from_environment()); }

// choose_ldlt_options on default LdltOptions (base_task_entries > 0: with that task size), then pair_list_options of
// the result: two rows of ten (choicecheck.py: OPTIONS)
void cc_options(int32_t batch, int32_t dim, int32_t compiled_model, int32_t base_task_entries, int64_t* out) {
  LdltOptions base;
  if (base_task_entries > 0) base.task_entries = static_cast<uint32_t>(base_task_entries);
  const LdltOptions chosen = choose_ldlt_options(base, batch, dim, compiled_model != 0, Switches::from_environment());
  options_row(chosen, out);
  options_row(pair_list_options(base, chosen), out + 10);
}

// 0: the dense factors of `batch` systems of order `dim` are within the bound; 1: not, and msg is what is thrown
int32_t cc_dense_bound(int32_t batch, int32_t dim, char* msg, int32_t cap) {
  try {
    require_dense_factors_fit(batch, dim);
    return 0;
  } catch (const std::exception& e) {
    std::snprintf(msg, static_cast<size_t>(cap), "%s", e.what());
    return 1;
  }
}

// The plan NewtonSystem gives the compiled model behind (s, k) — hostcheck's NlpStructure and KktPlan — in a batch:
// out = {dense, dense_pivoted, fronts built, fronts asked for}.  -1: the route threw (msg).
int32_t cc_plan(const NlpStructure* s, const KktPlan* k, const int32_t* perm, int32_t perm_len, int32_t batch, int64_t* out, char* msg,
                int32_t cap) {
  try {
    const Switches sw = Switches::from_environment();
    std::vector<uint8_t> diag_has_source(k->dim, 1);
    std::vector<int32_t> up;
    if (perm != nullptr && perm_len > 0) up.assign(perm, perm + perm_len);
    const LdltOptions lopt = choose_ldlt_options(LdltOptions{}, batch, k->dim, true, sw);
    const LdltOptions pair = pair_list_options(LdltOptions{}, lopt);
    const LdltPlan l = choose_ldlt_plan(k->lhs, s->n, k->reference_takes_dense(s->Ae.nnz()), up.empty() ? nullptr : &up, &diag_has_source, batch,
                                        lopt, &pair, sw);
    out[0] = l.dense;
    out[1] = l.dense_pivoted;
    out[2] = l.mf;
    out[3] = lopt.multifrontal;
    return 0;
  } catch (const std::exception& e) {
    std::snprintf(msg, static_cast<size_t>(cap), "%s", e.what());
    return -1;
  }
}

void cc_modes(const int64_t* in, int64_t* out) { choicecheck::run_modes(in, out); }

}  // extern "C"
