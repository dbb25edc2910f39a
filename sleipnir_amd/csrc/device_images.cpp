// The packers of device_images.hpp.  Host code only: plans in, vectors out.
#include "device_images.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <stdexcept>

#include "setup_threads.hpp"

namespace slpx {

TemplateTables pack_template_tables(const TapeProgram& p, const std::vector<TapeTemplateGroup>& groups, int batch,
                                    uint32_t block_threads) {
  TemplateTables out;
  std::vector<uint32_t>& inst = out.inst;
  for (const TapeTemplateGroup& g : groups) {
    // the family's leaf bindings and output destinations, transposed: row r of instance i at
    // [r * n_inst + i] (rows: leaves | value dst | value scale | jacobian dst | jacobian scale),
    // so that the lanes of a wave — consecutive instances — read consecutive words
    const uint32_t n_inst = static_cast<uint32_t>(g.tasks.size()), inst_off = static_cast<uint32_t>(inst.size());
    const TapeTask& rep = p.tasks[g.tasks.front()];
    const uint32_t rows = rep.n_leaf + 2 * rep.n_vout + 2 * rep.n_jout;
    inst.resize(inst.size() + static_cast<size_t>(rows) * n_inst);
    for (uint32_t i = 0; i < n_inst; ++i) {
      const TapeTask& t = p.tasks[g.tasks[i]];
      uint32_t* col = inst.data() + inst_off + i;
      uint32_t r = 0;
      for (uint32_t q = 0; q < rep.n_leaf; ++q) col[static_cast<size_t>(r++) * n_inst] = p.leaf_src[t.leaf_off + q];
      for (uint32_t q = 0; q < rep.n_vout; ++q) col[static_cast<size_t>(r++) * n_inst] = p.vout_dst[t.vout_off + q];
      for (uint32_t q = 0; q < rep.n_vout; ++q)
        col[static_cast<size_t>(r++) * n_inst] = static_cast<uint32_t>(p.vout_scale[t.vout_off + q]);
      for (uint32_t q = 0; q < rep.n_jout; ++q) col[static_cast<size_t>(r++) * n_inst] = p.jout_dst[t.jout_off + q];
      for (uint32_t q = 0; q < rep.n_jout; ++q)
        col[static_cast<size_t>(r++) * n_inst] = static_cast<uint32_t>(p.jout_scale[t.jout_off + q]);
    }
    out.n_templated_tasks += n_inst;
    // Adjoint rows are split into wave-uniform groups while the launch would otherwise
    // leave most SIMDs idle; with enough instances x batch items every lane runs all
    // groups (-1) and the forward part is not recomputed per group.
    const uint32_t waves = (n_inst + block_threads - 1) / block_threads;  // workgroups of one row group
    const bool split = ((n_inst + 63) / 64) * static_cast<uint32_t>(batch) < 512 && g.n_groups > 1;
    const int mode[2] = {0, split ? static_cast<int>(g.n_groups) : -1};
    for (int m = 0; m < 2; ++m) {
      out.table[m].push_back(out.blocks[m]);
      out.table[m].push_back(n_inst);
      out.table[m].push_back(inst_off);
      out.table[m].push_back(static_cast<uint32_t>(mode[m]));
      out.blocks[m] += waves * static_cast<uint32_t>(std::max(1, mode[m]));
    }
  }
  return out;
}

LdltLevelTables pack_ldlt_level_tables(const LdltPlan& l) {
  LdltLevelTables out;
  std::vector<uint32_t>&lp = out.lvl_pack, &cp = out.col_lvl_pack;
  lp.resize(l.lvl_ptr.size());
  cp.resize(l.col_lvl_ptr.size());
  for (size_t i = 0; i < lp.size(); ++i) {
    if (l.lvl_ptr[i] > 0xffffu || l.col_lvl_ptr[i] > 0xffffu || l.sn_lvl_ptr[i] > 0xffffu)
      throw std::runtime_error("slpx: an LDLT task exceeds the 16-bit packing of its level table");
    lp[i] = l.lvl_ptr[i] | (l.sn_lvl_ptr[i] << 16);
    cp[i] = l.col_lvl_ptr[i] | (l.sn_lvl_ptr[i] << 16);
  }
  std::vector<uint2>& rng = out.bwd_range;
  rng.assign(l.col_perm.size(), uint2{0, 0});
  for (const LdltTask& t : l.tasks)
    for (uint32_t i = 0; i < t.n_col; ++i) {
      const uint32_t cs = l.col_sn[t.col_off + i];
      rng[t.col_off + i] = uint2{l.bwd_ptr[t.colptr_off + i] + ((cs >> 8) - (cs & 0xffu) - 1u),
                                 l.bwd_ptr[t.colptr_off + i + 1]};
    }
  return out;
}

bool update_slots_have_one_reader(const LdltPlan& l) {
  std::vector<uint8_t> readers(std::max<uint32_t>(1, l.n_contrib), 0);
  bool single_reader = true;
  for (const LdltTask& t : l.tasks)  // (each task's slice is padded to a multiple of four)
    for (uint32_t c = 0; c < t.n_contrib_idx; ++c)
      single_reader = single_reader && ++readers[l.contrib_idx[t.contrib_off + c]] == 1;
  return single_reader;
}

std::vector<int32_t> lhs_diagonal_positions(const KktPlan& k) {
  std::vector<int32_t> diag_pos(std::max(1, k.n), 0);
  for (int c = 0; c < k.n; ++c)
    for (int p = k.lhs.colptr[c]; p < k.lhs.colptr[c + 1]; ++p)
      if (k.lhs.rowidx[p] == c) diag_pos[c] = p;
  return diag_pos;
}

IlMeta pack_il_meta(const LdltPlan& l) {
  IlMeta out;
  uint32_t fbytes = 0, col = 0, solve_bytes = 0;
  std::vector<uint32_t>&meta = out.meta, &meta_off = out.meta_off;
  for (const LdltTask& t : l.tasks) {
    const uint32_t n_cref = l.ent_contrib_ptr[t.contrib_ptr_off + t.n_ent];
    meta_off.push_back(static_cast<uint32_t>(meta.size()));
    const size_t head = meta.size();
    meta.push_back(n_cref);
    meta.push_back(0);
    for (uint32_t q = 0; q < t.n_pairs; ++q) {
      const LdltPair& pr = l.pairs[t.pair_off + q];
      meta.push_back(static_cast<uint32_t>(pr.a) | (static_cast<uint32_t>(pr.b) << 16));
      meta.push_back(pr.k);
    }
    for (uint32_t i = 0; i < t.n_ent + t.n_ext + 1; ++i) meta.push_back(l.ent_pair_ptr[t.pair_ptr_off + i]);
    for (uint32_t i = 0; i < t.n_ent; ++i) meta.push_back(static_cast<uint32_t>(l.ent_src[t.ent_off + i]));
    for (uint32_t i = 0; i < t.n_ent; ++i) meta.push_back(l.ent_out[t.ent_off + i]);
    for (uint32_t i = 0; i < t.n_ent; ++i)
      meta.push_back(static_cast<uint32_t>(l.ent_flags[t.ent_off + i]) | (static_cast<uint32_t>(l.ent_col[t.ent_off + i]) << 8));
    for (uint32_t i = 0; i < t.n_ext; ++i) meta.push_back(l.ext_dst[t.ext_off + i]);
    for (uint32_t i = 0; i < t.n_lvl + 1; ++i) meta.push_back(l.lvl_ptr[t.lvl_off + i]);
    // update-block refs, flat per entry slot (entry e belongs to slot e % kIlSlots), entry order and
    // block order within an entry as in the plan
    {
      const size_t ptr_at = meta.size();
      meta.insert(meta.end(), kIlSlots + 1, 0u);  // filled below: first ref of each slot, total
      uint32_t n_refs = 0;
      for (uint32_t sidx = 0; sidx < kIlSlots; ++sidx) {
        meta[ptr_at + sidx] = n_refs;
        for (uint32_t e = sidx; e < t.n_ent; e += kIlSlots)
          for (uint32_t cix = l.ent_contrib_ptr[t.contrib_ptr_off + e]; cix < l.ent_contrib_ptr[t.contrib_ptr_off + e + 1]; ++cix) {
            meta.push_back(e);
            meta.push_back(l.contrib_idx[t.contrib_off + cix]);
            ++n_refs;
          }
      }
      meta[ptr_at + kIlSlots] = n_refs;
    }
    const uint32_t n_words = static_cast<uint32_t>(meta.size() - head - 2);
    meta[head + 1] = n_words;
    fbytes = std::max(fbytes, std::max<uint32_t>((t.n_ent + t.n_col) * kIlW * 8u, 3u * kIlSlots * kIlW * 8u) + 4u * n_words + 16u);
    col = std::max(col, t.n_col + 1);
    solve_bytes = std::max(solve_bytes, t.n_col * 64u * 8u + 4u * (3u * t.n_col + t.n_lvl + 4u) + 8u * t.n_bwd_items + 16u);
  }
  if (meta.empty()) meta.push_back(0);
  if (meta_off.empty()) meta_off.push_back(0);
  out.factor_lds = fbytes;
  out.solve_lds = std::max(col * 64u * 8u, solve_bytes);  // fwd: y rows; bwd: x rows + its plan slices
  return out;
}

InlineKkt build_inline_kkt(const NlpStructure& s, const KktPlan& k, const LdltPlan& l) {
  std::vector<int32_t> vsrc(l.ent_src.size(), -1);
  std::vector<KktTerm> terms;
  std::vector<uint2> task_terms(l.tasks.size(), uint2{0, 0});
  auto term = [](int kind, int a, int row, int c) { return KktTerm{a, (kind << 28) | row, c}; };
  bool ok = s.nV < (1 << 30) && k.m_i < (1 << 28) && k.m_e < (1 << 28);
  uint32_t widest = 0;
  for (size_t ti = 0; ti < l.tasks.size() && ok; ++ti) {
    const LdltTask& t = l.tasks[ti];
    const size_t block = terms.size();
    for (uint32_t i = 0; i < t.n_ent; ++i) {
      const size_t e = t.ent_off + i;
      const int32_t s0 = l.ent_src[e];
      if (s0 < 0) continue;
      const size_t first = terms.size();
      if (l.ent_flags[e] & 4) {  // rhs entry s0 (kkt_kernels.h: kkt_rhs_entry)
        const int j = s0;
        if (j >= k.n) {
          vsrc[e] = (s.off_ce + j - k.n) | (1 << 30);
          continue;
        }
        if (k.g_src[j] >= 0) terms.push_back(term(1, k.g_src[j], 0, 0));
        for (int p = s.Ae.colptr[j]; p < s.Ae.colptr[j + 1]; ++p)
          terms.push_back(term(2, s.off_Ae + p, s.Ae.rowidx[p], 0));
        for (int p = s.Ai.colptr[j]; p < s.Ai.colptr[j + 1]; ++p)
          terms.push_back(term(3, s.off_Ai + p, s.Ai.rowidx[p], s.off_ci + s.Ai.rowidx[p]));
      } else {  // lhs entry s0 (kkt_kernels.h: kkt_assemble_body)
        const int f = k.fast_src[s0];
        if (f >= 0) {
          vsrc[e] = f;
          continue;
        }
        if (f != -2) continue;
        for (int q = k.dptr[s0]; q < k.dptr[s0 + 1]; ++q) terms.push_back(term(0, k.dsrc[q], 0, 0));
        for (int q = k.pptr[s0]; q < k.pptr[s0 + 1]; ++q) terms.push_back(term(4, k.pa[q], k.pr[q], k.pb[q]));
      }
      const size_t rel = first - block, cnt = terms.size() - first;
      if (rel >= (1u << 20) || cnt >= (1u << 11)) {
        ok = false;
        break;
      }
      // (a sum of nothing — an x row with no gradient, no A_e, no A_i entry — is a zero)
      vsrc[e] = cnt == 0 ? -1 : -static_cast<int32_t>(2 + (rel | (cnt << 20)));
    }
    while ((terms.size() - block) % 4 != 0) terms.push_back(KktTerm{0, 0, 0});  // 4 terms = 3 x 16 bytes
    const uint32_t off16 = static_cast<uint32_t>(block * sizeof(KktTerm) / 16);
    const uint32_t len16 = static_cast<uint32_t>((terms.size() - block) * sizeof(KktTerm) / 16);
    task_terms[ti] = uint2{off16, len16};
    widest = std::max(widest, len16);
  }
  InlineKkt out;
  // the staged terms and, behind them, one product per term (4 terms = 3 x 16 bytes)
  out.factor_lds = l.factor_lds_bytes + 16u + 16u * widest + 8u * (widest * 4u / 3u);
  if (!ok || out.factor_lds > 160u * 1024u) return out;  // (the stand-alone assembly kernels then)
  if (terms.empty()) terms.push_back(KktTerm{0, 0, 0});
  out.vsrc = std::move(vsrc);
  out.terms = std::move(terms);
  out.task_terms = std::move(task_terms);
  out.ok = true;
  return out;
}

InlineBacksub build_inline_backsub(const KktPlan& k, const LdltPlan& l) {
  static_assert(sizeof(BsRow) == 8 && sizeof(BsTerm) == 8, "rows and terms are staged as 16-byte pairs");
  const int dim = l.n;
  std::vector<int32_t> inv_perm(dim, -1), task_of(dim, -1), local_of(dim, -1);
  for (int pj = 0; pj < dim; ++pj) inv_perm[l.perm[pj]] = pj;
  for (size_t ti = 0; ti < l.tasks.size(); ++ti)
    for (uint32_t i = 0; i < l.tasks[ti].n_col; ++i) {
      const uint32_t pj = l.col_perm[l.tasks[ti].col_off + i];
      task_of[pj] = static_cast<int32_t>(ti);
      local_of[pj] = static_cast<int32_t>(i);
    }
  std::vector<std::vector<int>> rows_of(l.tasks.size());
  bool ok = true;
  for (int r = 0; r < k.m_i && ok; ++r) {
    int deepest = -1;
    for (int q = k.ai_rowptr[r]; q < k.ai_rowptr[r + 1]; ++q) {
      const int pj = inv_perm[k.ai_col[q]];
      if (deepest < 0 || pj < deepest) deepest = pj;
    }
    if (deepest < 0) deepest = 0;  // an empty row: anybody
    const int owner = task_of[deepest];
    // what the scheme rests on: every other column is the owner's or an ancestor's (a later round's)
    for (int q = k.ai_rowptr[r]; q < k.ai_rowptr[r + 1]; ++q) {
      const int other = task_of[inv_perm[k.ai_col[q]]];
      if (other != owner && l.tasks[other].round <= l.tasks[owner].round) ok = false;
    }
    rows_of[owner].push_back(r);
  }
  std::vector<BsRow> plan;  // BsRow and BsTerm are both two 32-bit words: one array
  std::vector<uint4> task_plan(l.tasks.size(), uint4{0, 0, 0, 0});
  uint32_t widest = 0;
  for (size_t ti = 0; ti < l.tasks.size() && ok; ++ti) {
    const size_t block = plan.size();
    const std::vector<int>& rows = rows_of[ti];
    const size_t n_rows = rows.size(), rows_padded = (n_rows + 1) / 2 * 2;
    plan.resize(block + rows_padded, BsRow{0, 0});
    uint32_t term = 0;
    for (size_t j = 0; j < n_rows; ++j) {
      const int r = rows[j];
      const uint32_t cnt = static_cast<uint32_t>(k.ai_rowptr[r + 1] - k.ai_rowptr[r]);
      if (term >= (1u << 20) || cnt >= (1u << 12)) ok = false;
      plan[block + j] = BsRow{r, term | (cnt << 20)};
      for (int q = k.ai_rowptr[r]; q < k.ai_rowptr[r + 1]; ++q) {
        const int pj = inv_perm[k.ai_col[q]];
        const uint32_t ref = task_of[pj] == static_cast<int32_t>(ti) ? static_cast<uint32_t>(local_of[pj])
                                                                     : (0x80000000u | static_cast<uint32_t>(pj));
        plan.push_back(BsRow{k.ai_src[q], ref});  // (a BsTerm)
        ++term;
      }
    }
    if ((plan.size() - block) % 2 != 0) plan.push_back(BsRow{0, 0});
    const uint32_t len16 = static_cast<uint32_t>((plan.size() - block) / 2);
    task_plan[ti] = uint4{static_cast<uint32_t>(block / 2), len16, static_cast<uint32_t>(n_rows),
                          static_cast<uint32_t>(rows_padded / 2)};
    widest = std::max(widest, len16);
  }
  InlineBacksub out;
  out.solve_lds = l.solve_lds_bytes + 16u + 16u * widest;
  if (!ok || out.solve_lds > 160u * 1024u) return out;  // (the stand-alone back-substitution kernel then)
  if (plan.empty()) plan.push_back(BsRow{0, 0});
  out.plan = std::move(plan);
  out.task_plan = std::move(task_plan);
  out.ok = true;
  return out;
}

MfImages build_mf_images(const LdltPlan& l, const InlineKkt& kkt, const InlineBacksub& bs) {
  MfImages out;
  if (kkt.task_terms.size() != l.tasks.size() || bs.task_plan.size() != l.tasks.size()) {
    out.declined = "no inline KKT terms or back-substitution rows";
    return out;
  }
  // Every task's static LDS content as ONE image in LDS order (mf_carve: from the tables to the KKT
  // terms, then — behind the terms' products, which are not staged — its back-substitution rows):
  // thirteen arrays staged one after the other were thirteen dependent waits on memory (4.5 us);
  // one copy loop with every load in flight is a single trip.
  uint32_t lds = 0;
  std::vector<uint4> image, desc(l.tasks.size());
  // sizes first (the slots are of one size: the largest image), then every task's image written straight into its
  // slot, the tasks in chunks on the setup threads
  std::vector<uint32_t> blob_bytes(l.tasks.size());
  size_t stride16 = 1;
  for (size_t ti = 0; ti < l.tasks.size(); ++ti) {
    const MfCarve cv = mf_carve(l.tasks[ti], l.mf_tasks[ti]);
    const uint32_t terms16 = kkt.task_terms[ti].y, bs16 = bs.task_plan[ti].y;
    const uint32_t n_terms = terms16 * 4u / 3u;
    const uint32_t end_terms = cv.o_terms + 16u * terms16;
    lds = std::max(lds, mf_align16(end_terms + 8u * n_terms) + 16u * bs16);
    blob_bytes[ti] = end_terms - cv.o_tab + 16u * bs16;
    stride16 = std::max<size_t>(stride16, blob_bytes[ti] / 16u);
    desc[ti] = uint4{0u, (end_terms - cv.o_tab) / 16u, bs16, terms16};
  }
  if (stride16 > kMfImageGroups) {  // (a task image beyond what the staging loop requests)
    out.declined = "a task image is longer than the staging loop requests";
    return out;
  }
  // fixed-size slots (the kernel requests a task's image before it knows its length) + one round of padding
  image.assign(stride16 * l.tasks.size() + kMfImageGroups, uint4{0, 0, 0, 0});
  std::atomic<bool> out_of_bounds{false}, terms_do_not_fit{false};
  parallel_chunks(l.tasks.size(), 8, [&](size_t t_begin, size_t t_end, unsigned) {
    std::vector<uint8_t> fl;
    std::vector<int32_t> vs;
    for (size_t ti = t_begin; ti < t_end; ++ti) {
      const LdltTask& t = l.tasks[ti];
      const LdltMfTask& m = l.mf_tasks[ti];
      const MfCarve cv = mf_carve(t, m);
      const uint32_t terms16 = kkt.task_terms[ti].y, bs16 = bs.task_plan[ti].y;
      const uint32_t end_terms = cv.o_terms + 16u * terms16;
      unsigned char* blob = reinterpret_cast<unsigned char*>(image.data() + ti * stride16);
      const size_t blob_size = blob_bytes[ti];
      auto put = [&](uint32_t at, const void* src, size_t bytes) {
        if (at < cv.o_tab || at - cv.o_tab + bytes > blob_size) {
          out_of_bounds = true;
          return;
        }
        if (bytes) std::memcpy(blob + (at - cv.o_tab), src, bytes);
      };
      put(cv.o_tab, l.mf_tab.data() + m.tab_off, 2u * m.n_tab);
      put(cv.o_lvl, l.mf_lvl_ptr.data() + t.lvl_off, 4u * (t.n_lvl + 1));
      put(cv.o_ext, l.mf_ext.data() + m.ext_off, 4u * m.n_ext);
      {
        // where an entry's value comes from; an entry that is a sum of terms says how many of each kind
        // (kkt_terms_sum_grouped: the terms lie kind by kind)
        vs.assign(kkt.vsrc.begin() + t.ent_off, kkt.vsrc.begin() + t.ent_off + t.n_ent);
        const KktTerm* tt = kkt.terms.data() + static_cast<size_t>(kkt.task_terms[ti].x) * 4u / 3u;
        for (uint32_t i = 0; i < t.n_ent; ++i) {
          if (vs[i] >= -1) continue;
          const uint32_t code = static_cast<uint32_t>(-(vs[i] + 2));
          const uint32_t first = code & 0xfffffu, cnt = code >> 20;
          uint32_t has_g = 0, n_a = 0, n_b = 0;
          bool sorted = true;
          int last = -1;
          for (uint32_t q = first; q < first + cnt; ++q) {
            const int kind = tt[q].b >> 28;
            sorted = sorted && kind >= last;
            last = kind;
            if (kind == 1) ++has_g;
            else if (kind == 0 || kind == 2) ++n_a;
            else ++n_b;
          }
          if (!sorted || has_g > 1 || !mf_term_code_fits(first, n_a, n_b)) {
            terms_do_not_fit = true;
            break;
          }
          vs[i] = -static_cast<int32_t>(2u + mf_term_code(first, has_g, n_a, n_b));
        }
        put(cv.o_src, vs.data(), 4u * t.n_ent);
      }
      {
        // (bit 5: the entry takes update slots)
        fl.assign(l.ent_flags.begin() + t.ent_off, l.ent_flags.begin() + t.ent_off + t.n_ent);
        for (uint32_t j = 0; j < m.n_cent; ++j) fl[l.mf_cent[m.cent_off + j]] |= 0x20;
        put(cv.o_flags, fl.data(), t.n_ent);
      }
      put(cv.o_cent, l.mf_cent.data() + m.cent_off, 2u * m.n_cent);
      put(cv.o_cptr, l.mf_contrib_ptr.data() + m.contrib_ptr_off, 4u * (m.n_cent + 1));
      put(cv.o_cidx, l.mf_contrib_idx.data() + m.contrib_off, 4u * m.n_contrib_idx);
      put(cv.o_cp, l.col_perm.data() + t.col_off, 4u * t.n_col);
      put(cv.o_anc, l.mf_anc.data() + m.anc_off, 4u * m.n_anc);
      put(cv.o_fr, l.mf_fronts.data() + m.front_off, sizeof(LdltFront) * m.n_front);
      {
        // the inertia counters start at zero, the smallest |d| at +inf
        const unsigned long long inf = 0x7ff0000000000000ull;
        put(cv.o_cnt + 16u, &inf, 8);
      }
      put(cv.o_terms, reinterpret_cast<const unsigned char*>(kkt.terms.data()) + 16u * static_cast<size_t>(kkt.task_terms[ti].x),
          16u * terms16);
      put(end_terms, reinterpret_cast<const unsigned char*>(bs.plan.data()) + 16u * static_cast<size_t>(bs.task_plan[ti].x),
          16u * bs16);
    }
  });
  if (out_of_bounds) throw std::runtime_error("slpx: task image layout out of bounds");
  if (terms_do_not_fit) {  // (an entry of hundreds of terms: the pair-list kernels' encoding holds 2047)
    out.declined = "an entry's terms do not fit the image's source word";
    return out;
  }
  out.image = std::move(image);
  out.desc = std::move(desc);
  out.stride16 = static_cast<uint32_t>(stride16);
  out.lds = mf_align16(lds) + 16u;
  return out;
}

}  // namespace slpx
