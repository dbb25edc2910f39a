// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// The packers of csrc/device_images.hpp run on a problem's plans (hostcheck's: hc_plans), every array they return —
// and every plan array the tests compare them with — handed out by name as raw bytes for numpy.  Nothing is checked
// here: tests/test_device_images_cpu.py decodes the images and compares them with the plans and with hostcheck's
// interpreters.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../sleipnir_amd/csrc/device_images.hpp"

using namespace slpx;

struct ic_handle {
  const NlpStructure* s;
  const KktPlan* k;
  const LdltPlan* l;
  InlineKkt kkt;
  InlineBacksub bs;
  std::map<std::string, std::vector<unsigned char>> arrays;
  std::map<std::string, int64_t> scalars;
  template <class T>
  void put(const std::string& name, const std::vector<T>& v) {
    std::vector<unsigned char>& a = arrays[name];
    a.resize(v.size() * sizeof(T));
    if (!v.empty()) std::memcpy(a.data(), v.data(), a.size());
  }
  // one field of an array of structs as an array of its own
  template <class S, class F>
  void field(const std::string& name, const std::vector<S>& v, F S::*member) {
    std::vector<F> col(v.size());
    for (size_t i = 0; i < v.size(); ++i) col[i] = v[i].*member;
    put(name, col);
  }
};

namespace {

void put_plans(ic_handle* h) {
  const NlpStructure& s = *h->s;
  const KktPlan& k = *h->k;
  const LdltPlan& l = *h->l;
  auto scalar = [&](const char* name, int64_t v) { h->scalars[name] = v; };
  scalar("s.nV", s.nV), scalar("s.off_ce", s.off_ce), scalar("s.off_ci", s.off_ci), scalar("s.off_Ae", s.off_Ae);
  scalar("s.off_Ai", s.off_Ai), scalar("k.n", k.n), scalar("k.m_e", k.m_e), scalar("k.m_i", k.m_i), scalar("k.dim", k.dim);
  scalar("l.n", l.n), scalar("l.mf", l.mf), scalar("l.n_contrib", l.n_contrib);
  scalar("l.factor_lds_bytes", l.factor_lds_bytes), scalar("l.solve_lds_bytes", l.solve_lds_bytes);
  h->put("s.Ae.colptr", s.Ae.colptr);
  h->put("s.Ae.rowidx", s.Ae.rowidx);
  h->put("s.Ai.colptr", s.Ai.colptr);
  h->put("s.Ai.rowidx", s.Ai.rowidx);
  h->put("k.dptr", k.dptr);
  h->put("k.dsrc", k.dsrc);
  h->put("k.pptr", k.pptr);
  h->put("k.pa", k.pa);
  h->put("k.pb", k.pb);
  h->put("k.pr", k.pr);
  h->put("k.g_src", k.g_src);
  h->put("k.fast_src", k.fast_src);
  h->put("k.ai_rowptr", k.ai_rowptr);
  h->put("k.ai_col", k.ai_col);
  h->put("k.ai_src", k.ai_src);
  h->put("k.lhs.colptr", k.lhs.colptr);
  h->put("k.lhs.rowidx", k.lhs.rowidx);
  h->put("l.perm", l.perm);
  h->put("l.round_ptr", l.round_ptr);
  h->put("l.ent_src", l.ent_src);
  h->put("l.ent_flags", l.ent_flags);
  h->put("l.ent_col", l.ent_col);
  h->put("l.ent_out", l.ent_out);
  h->put("l.ent_pair_ptr", l.ent_pair_ptr);
  h->put("l.ent_contrib_ptr", l.ent_contrib_ptr);
  h->put("l.contrib_idx", l.contrib_idx);
  h->put("l.ext_dst", l.ext_dst);
  h->put("l.lvl_ptr", l.lvl_ptr);
  h->put("l.pairs", l.pairs);  // uint16 x 4: a, b, k, pad
  h->put("l.col_perm", l.col_perm);
  h->put("l.col_lvl_ptr", l.col_lvl_ptr);
  h->put("l.bwd_ptr", l.bwd_ptr);
  h->put("l.sn_lvl_ptr", l.sn_lvl_ptr);
  h->put("l.col_sn", l.col_sn);
  h->put("l.mf_fronts", l.mf_fronts);  // 16 bytes each
  h->put("l.mf_lvl_ptr", l.mf_lvl_ptr);
  h->put("l.mf_tab", l.mf_tab);
  h->put("l.mf_ext", l.mf_ext);
  h->put("l.mf_contrib_ptr", l.mf_contrib_ptr);
  h->put("l.mf_contrib_idx", l.mf_contrib_idx);
  h->put("l.mf_cent", l.mf_cent);
  h->put("l.mf_anc", l.mf_anc);
#define IC_TASK(f) h->field("l.tasks." #f, l.tasks, &LdltTask::f)
  IC_TASK(n_ent); IC_TASK(n_col); IC_TASK(n_ext); IC_TASK(ent_off); IC_TASK(col_off); IC_TASK(lvl_off); IC_TASK(n_lvl);
  IC_TASK(ext_off); IC_TASK(pair_off); IC_TASK(contrib_off); IC_TASK(round); IC_TASK(pair_ptr_off); IC_TASK(contrib_ptr_off);
  IC_TASK(colptr_off); IC_TASK(n_pairs); IC_TASK(n_bwd_items); IC_TASK(n_contrib_idx);
#undef IC_TASK
#define IC_MF(f) h->field("l.mf_tasks." #f, l.mf_tasks, &LdltMfTask::f)
  IC_MF(front_off); IC_MF(n_front); IC_MF(tab_off); IC_MF(n_tab); IC_MF(ext_off); IC_MF(n_ext); IC_MF(cent_off); IC_MF(n_cent);
  IC_MF(contrib_ptr_off); IC_MF(contrib_off); IC_MF(n_contrib_idx); IC_MF(anc_off); IC_MF(n_anc); IC_MF(arena);
#undef IC_MF
  const TapeProgram& p = s.full;
#define IC_TAPE(f) h->field("tape.tasks." #f, p.tasks, &TapeTask::f)
  IC_TAPE(n_leaf); IC_TAPE(n_node); IC_TAPE(n_slot); IC_TAPE(leaf_off); IC_TAPE(vout_off); IC_TAPE(n_vout); IC_TAPE(jout_off);
  IC_TAPE(n_jout);
#undef IC_TAPE
  h->put("tape.leaf_src", p.leaf_src);
  h->put("tape.vout_dst", p.vout_dst);
  h->put("tape.vout_scale", p.vout_scale);
  h->put("tape.jout_dst", p.jout_dst);
  h->put("tape.jout_scale", p.jout_scale);
  // the layout constants the tests decode by (device_layout.h)
  h->scalars["kIlSlots"] = kIlSlots;
  h->scalars["kIlW"] = kIlW;
  h->scalars["kMfImageGroups"] = kMfImageGroups;
  h->scalars["kMfTermFirstBits"] = kMfTermFirstBits;
  h->scalars["kMfTermABits"] = kMfTermABits;
  h->scalars["kMfTermBBits"] = kMfTermBBits;
}

void put_images(ic_handle* h) {
  const NlpStructure& s = *h->s;
  const KktPlan& k = *h->k;
  const LdltPlan& l = *h->l;
  const LdltLevelTables lt = pack_ldlt_level_tables(l);
  h->put("lvl_pack", lt.lvl_pack);
  h->put("col_lvl_pack", lt.col_lvl_pack);
  h->put("bwd_range", lt.bwd_range);  // uint32 x 2
  h->scalars["one_reader"] = update_slots_have_one_reader(l);
  h->put("diag_pos", lhs_diagonal_positions(k));
  const IlMeta im = pack_il_meta(l);
  h->put("il.meta", im.meta);
  h->put("il.meta_off", im.meta_off);
  h->scalars["il.factor_lds"] = im.factor_lds;
  h->scalars["il.solve_lds"] = im.solve_lds;
  h->kkt = build_inline_kkt(s, k, l);
  h->put("kkt.vsrc", h->kkt.vsrc);
  h->put("kkt.terms", h->kkt.terms);            // int32 x 3
  h->put("kkt.task_terms", h->kkt.task_terms);  // uint32 x 2
  h->scalars["kkt.factor_lds"] = h->kkt.factor_lds;
  h->scalars["kkt.ok"] = h->kkt.ok;
  h->bs = build_inline_backsub(k, l);
  h->put("bs.plan", h->bs.plan);            // uint32 x 2
  h->put("bs.task_plan", h->bs.task_plan);  // uint32 x 4
  h->scalars["bs.solve_lds"] = h->bs.solve_lds;
  h->scalars["bs.ok"] = h->bs.ok;
  if (!l.mf) return;
  const MfImages mf = build_mf_images(l, h->kkt, h->bs);
  h->put("mf.image", mf.image);  // raw 16-byte groups
  h->put("mf.desc", mf.desc);    // uint32 x 4
  h->scalars["mf.stride16"] = mf.stride16;
  h->scalars["mf.lds"] = mf.lds;
  h->scalars["mf.declined"] = mf.declined != nullptr;
  std::vector<uint32_t> carve;
  for (size_t ti = 0; ti < l.tasks.size(); ++ti) {
    const MfCarve c = mf_carve(l.tasks[ti], l.mf_tasks[ti]);
    for (uint32_t o : {c.o_arena, c.o_invd, c.o_x, c.o_tab, c.o_lvl, c.o_ext, c.o_src, c.o_flags, c.o_cent, c.o_cptr, c.o_cidx,
                       c.o_cp, c.o_anc, c.o_fr, c.o_cnt, c.o_terms})
      carve.push_back(o);
  }
  h->put("mf.carve", carve);  // uint32 x 16, in MfCarve's order
}

}  // namespace

extern "C" {

// s, k, l: hc_plans of a hostcheck handle that outlives this one
ic_handle* ic_create(const void* s, const void* k, const void* l) {
  auto* h = new ic_handle{static_cast<const NlpStructure*>(s), static_cast<const KktPlan*>(k), static_cast<const LdltPlan*>(l)};
  try {
    put_plans(h);
    put_images(h);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ic_create: %s\n", e.what());
    delete h;
    return nullptr;
  }
  return h;
}
void ic_destroy(ic_handle* h) { delete h; }

// bytes of the array `name` (-1: no such array); its address in *data
int64_t ic_array(ic_handle* h, const char* name, const void** data) {
  const auto it = h->arrays.find(name);
  if (it == h->arrays.end()) return -1;
  *data = it->second.data();
  return static_cast<int64_t>(it->second.size());
}
int32_t ic_scalar(ic_handle* h, const char* name, int64_t* out) {
  const auto it = h->scalars.find(name);
  if (it == h->scalars.end()) return -1;
  *out = it->second;
  return 0;
}

// pack_template_tables on the full tape with families made here — the tasks of equal (leaves, nodes, slots, value and
// jacobian outputs), two members and more, in order of first appearance, cut into pieces of at most `max_members`
// (any subset of a family is one), each with `n_groups` row groups — so that no kernel has to be generated: arrays tmpl.inst, tmpl.table0, tmpl.table1, tmpl.blocks, tmpl.family_ptr,
// tmpl.family_tasks; scalar tmpl.n_templated_tasks.  Returns the number of families.
int32_t ic_template_tables(ic_handle* h, int32_t batch, uint32_t block_threads, uint32_t n_groups, uint32_t max_members) {
  const TapeProgram& p = h->s->full;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, size_t> index;
  std::vector<TapeTemplateGroup> all;
  for (uint32_t ti = 0; ti < p.tasks.size(); ++ti) {
    const TapeTask& t = p.tasks[ti];
    const auto key = std::make_tuple(t.n_leaf, t.n_node, t.n_slot, t.n_vout, t.n_jout);
    auto it = index.find(key);
    if (it == index.end()) {
      it = index.emplace(key, all.size()).first;
      all.emplace_back();
      all.back().n_leaf = t.n_leaf, all.back().n_node = t.n_node, all.back().n_slot = t.n_slot, all.back().n_groups = n_groups;
    }
    all[it->second].tasks.push_back(ti);
  }
  std::vector<TapeTemplateGroup> groups;
  for (const TapeTemplateGroup& g : all)
    for (size_t at = 0; g.tasks.size() >= 2 && at < g.tasks.size(); at += max_members) {
      groups.push_back(g);
      groups.back().tasks.assign(g.tasks.begin() + at, g.tasks.begin() + std::min<size_t>(g.tasks.size(), at + max_members));
    }
  const TemplateTables tt = pack_template_tables(p, groups, batch, block_threads);
  h->put("tmpl.inst", tt.inst);
  h->put("tmpl.table0", tt.table[0]);
  h->put("tmpl.table1", tt.table[1]);
  h->put("tmpl.blocks", std::vector<uint32_t>{tt.blocks[0], tt.blocks[1]});
  h->scalars["tmpl.n_templated_tasks"] = tt.n_templated_tasks;
  std::vector<uint32_t> ptr{0}, tasks;
  for (const TapeTemplateGroup& g : groups) {
    tasks.insert(tasks.end(), g.tasks.begin(), g.tasks.end());
    ptr.push_back(static_cast<uint32_t>(tasks.size()));
  }
  h->put("tmpl.family_ptr", ptr);
  h->put("tmpl.family_tasks", tasks);
  return static_cast<int32_t>(groups.size());
}

// pack_ldlt_level_tables on a copy of the plan whose last entry-level pointer is `value`: 1 if it threw
int32_t ic_level_tables_throw_at(ic_handle* h, uint32_t value) {
  LdltPlan doctored = *h->l;
  if (doctored.lvl_ptr.empty()) return -1;
  doctored.lvl_ptr.back() = value;
  try {
    (void)pack_ldlt_level_tables(doctored);
  } catch (const std::runtime_error&) {
    return 1;
  }
  return 0;
}

// build_mf_images with task_terms one entry short: 1 if it declined
int32_t ic_mf_declines_short_task_terms(ic_handle* h) {
  InlineKkt shortened = h->kkt;
  if (shortened.task_terms.empty()) return -1;
  shortened.task_terms.pop_back();
  return build_mf_images(*h->l, shortened, h->bs).declined != nullptr ? 1 : 0;
}

}  // extern "C"
