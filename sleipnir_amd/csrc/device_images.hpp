// What the kernels read, made from the host plans (NlpStructure, KktPlan, LdltPlan): packed tables and
// per-task LDS images as plain vectors.  Pure functions — no device, no allocation on one: DeviceNlp's
// constructor (kernels.hip) uploads what they return, tests/support/imagecheck.cpp reads the same arrays
// back against the plans on the CPU.  The layouts are those of device_layout.h.
#pragma once

#include <cstdint>
#include <vector>

#include "device_layout.h"
#include "kkt_plan.hpp"
#include "ldlt_symbolic.hpp"
#include "nlp.hpp"
#include "tape_jit.hpp"

namespace slpx {

// The generated tape kernel's tables (TapeDevice::tmpl_*).  inst: per body the family's leaf bindings and
// output destinations, transposed — row r of instance i at [off + r * n_inst + i], rows: leaves | value dst |
// value scale | jacobian dst | jacobian scale.  table[mode] (0: values only, 1: with adjoints): per body
// (first block, instances, off, row-group mode); blocks[mode]: the grid.
struct TemplateTables {
  std::vector<uint32_t> inst, table[2];
  uint32_t blocks[2] = {0, 0};
  uint32_t n_templated_tasks = 0;
};
TemplateTables pack_template_tables(const TapeProgram& p, const std::vector<TapeTemplateGroup>& groups, int batch,
                                    uint32_t block_threads);

// The hot loops' own copies of the level tables (LdltDev::lvl_pack, col_lvl_pack, bwd_range).  Throws where a
// pointer does not fit 16 bits.
struct LdltLevelTables {
  std::vector<uint32_t> lvl_pack;      // lvl_ptr | sn_lvl_ptr << 16
  std::vector<uint32_t> col_lvl_pack;  // col_lvl_ptr | sn_lvl_ptr << 16
  std::vector<uint2> bwd_range;        // per column {first item below its own chain, end}
};
LdltLevelTables pack_ldlt_level_tables(const LdltPlan& l);

// slot hand-over (ldlt_kernels.h: slot_take) needs every update slot to have exactly one reader
bool update_slots_have_one_reader(const LdltPlan& l);

// per column of the decision block: where its diagonal sits in the lhs values (kkt_add_identity_kernel)
std::vector<int32_t> lhs_diagonal_positions(const KktPlan& k);

// Batch-interleaved factorization (ldlt_il_kernels.h): per task the plan slices the kernel keeps in LDS, packed
// back to back, meta_off[task] the first word of
//   [n_cref, n_words | pairs (2 words each) | pair ptr | src | out | flags + column | ext dst | level ptr |
//    kIlSlots + 1 ref pointers | per-slot update-block refs (entry, slot)]
struct IlMeta {
  std::vector<uint32_t> meta, meta_off;
  uint32_t factor_lds = 0, solve_lds = 0;  // dynamic LDS of the factor / solve kernels
};
IlMeta pack_il_meta(const LdltPlan& l);

// The static side of KktFuse: for every entry of the factorization plan what it is made of.  vsrc is
// KktFuse::ent_vsrc, terms / task_terms KktFuse::terms / task_terms.  ok = false (a field too narrow, or more LDS
// than a CU has): the vectors are empty and the stand-alone assembly kernels serve; factor_lds is set either way.
struct InlineKkt {
  std::vector<int32_t> vsrc;
  std::vector<KktTerm> terms;
  std::vector<uint2> task_terms;
  uint32_t factor_lds = 0;  // dynamic LDS of the factorization with the terms staged
  bool ok = false;
};
InlineKkt build_inline_kkt(const NlpStructure& s, const KktPlan& k, const LdltPlan& l);

// The static side of BacksubFuse: every row of A_i goes to the task that owns the deepest of its columns.
// plan / task_plan are BacksubFuse::plan / task_plan; ok = false also where a row's columns are not on one root path.
struct InlineBacksub {
  std::vector<BsRow> plan;  // BsRow and BsTerm are both two 32-bit words: one array
  std::vector<uint4> task_plan;
  uint32_t solve_lds = 0;  // dynamic LDS of the backward solve with the rows staged
  bool ok = false;
};
InlineBacksub build_inline_backsub(const KktPlan& k, const LdltPlan& l);

// The multifrontal step's task images (ldlt_mf_kernels.h): every task's static LDS content in LDS order, in slots of
// one size (stride16 16-byte groups, + one round of padding at the end); desc per task {0, groups up to the end of
// the KKT terms, groups of back-substitution rows, terms groups}; lds: the dynamic LDS the longest task needs.
// declined != nullptr: no images (the pair-list kernels serve), and why.  Throws if a region leaves its slot.
struct MfImages {
  std::vector<uint4> image, desc;
  uint32_t stride16 = 0;
  uint32_t lds = 0;
  const char* declined = nullptr;
};
MfImages build_mf_images(const LdltPlan& l, const InlineKkt& kkt, const InlineBacksub& bs);

}  // namespace slpx
