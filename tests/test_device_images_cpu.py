"""CPU tier: what DeviceNlp's constructor makes of the plans (csrc/device_images.hpp: packed tables, the interleaved
kernels' meta words, inline KKT terms, back-substitution rows, multifrontal task images) decoded again and compared
with the plan arrays and with hostcheck's interpreters (hc_assemble, hc_rhs, hc_backsub) — never with the packers
themselves.  tests/support/imagecheck.cpp hands the arrays over; everything is checked here."""
import numpy as np
import pytest

from tests.support import cases

EPS = 2.0 ** -52
# (tests/support/cases.py has no model with a shared timestep variable.  The inequality rows of cart-pole and flywheel
# are bounds, one column each, so no back-substitution row of theirs reaches into an ancestor task; the g-fold descent's
# cone rows have up to four columns and do.  The models of tests/support/step_models.py have a hub column: a variable in
# 24 rows of each kind (chain130), in 3 + 3 (hub40_3_3, one task), and in 255 + 127 (hub530_255_127: the most terms the
# source word of a multifrontal task image holds, device_layout.h: mf_term_code_fits).)
STEP_MODELS = ["chain130", "hub40_3_3", "hub530_255_127"]
MODELS = [("cart_pole", 4), ("cart_pole", 37), ("flywheel", 50), ("gfold", 8)] + [("step", name) for name in STEP_MODELS]

TASK_FIELDS = ["n_ent", "n_col", "n_ext", "ent_off", "col_off", "lvl_off", "n_lvl", "ext_off", "pair_off", "contrib_off", "round",
               "pair_ptr_off", "contrib_ptr_off", "colptr_off", "n_pairs", "n_bwd_items", "n_contrib_idx"]
MF_FIELDS = ["front_off", "n_front", "tab_off", "n_tab", "ext_off", "n_ext", "cent_off", "n_cent", "contrib_ptr_off", "contrib_off",
             "n_contrib_idx", "anc_off", "n_anc", "arena"]
TAPE_FIELDS = ["n_leaf", "n_node", "n_slot", "leaf_off", "vout_off", "n_vout", "jout_off", "n_jout"]


class Case:
    """One model under SLPX_LDLT_MF=1: its hostcheck handle, its images, and a random state swept and solved once."""

    def __init__(self, kind, N, slpx, orc, hostcheck):
        from tests.support import imagecheck

        orc.lib().orc_reset()
        slpx.lib().slpx_graph_reset()
        self.model = (kind, N)
        if kind == "gfold":
            from tests.support import gfold, model

            self.pp = gfold.build(model.Model(model.ProductBackend("hostcheck")), N).p
        elif kind == "step":
            from tests.support import model, step_models

            self.pp = step_models.make(model.Model(model.ProductBackend("hostcheck")), N)[0].p
            N = self.pp.dims[0]  # (the seed below)
        else:
            self.pp, _ = cases.build_pair(kind, N, slpx, orc)
        self.hc = hc = hostcheck.HostCheck(self.pp)
        self.im = im = imagecheck.Images(hc)
        self.t = {f: v.astype(np.int64) for f, v in im.tasks("l.tasks", TASK_FIELDS).items()}
        self.m = {f: v.astype(np.int64) for f, v in im.tasks("l.mf_tasks", MF_FIELDS).items()}
        self.n_tasks = len(self.t["n_ent"])
        n, me, mi = hc.n, hc.m_e, hc.m_i
        rng = np.random.default_rng(cases.SEED + N)
        self.x = rng.uniform(-1, 1, n)
        self.s, self.z = np.exp(rng.uniform(-2, 2, mi)), np.exp(rng.uniform(-2, 2, mi))
        self.y, self.mu = rng.uniform(-1, 1, me), float(np.exp(rng.uniform(-3, 0)))
        self.V = hc.sweep(self.x, self.y, self.z, True)
        self.lhs = hc.assemble(self.s, self.z)
        self.rhs = hc.rhs(self.s, self.y, self.z, self.mu)
        hc.factor(1e-4, 1e-10)
        self.p = hc.solve()  # (some p: what hc_backsub evaluates the rows at)
        self.ps, self.pz = hc.backsub(self.s, self.z, self.mu)

    def close(self):
        self.im.close()
        self.hc.close()
        self.pp.close()


@pytest.fixture(scope="module", params=MODELS, ids=lambda m: f"{m[0]}-{m[1]}")
def case(request, slpx, orc, hostcheck):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SLPX_LDLT_MF", "1")
        c = Case(*request.param, slpx, orc, hostcheck)
    yield c
    c.close()


def task_of_entry(c):
    """per entry of the plan's entry arrays its task (-1: padding between the tasks' slices)"""
    owner = np.full(len(c.im.array("l.ent_src", "i4")), -1)
    for ti in range(c.n_tasks):
        owner[c.t["ent_off"][ti]:c.t["ent_off"][ti] + c.t["n_ent"][ti]] = ti
    return owner


def test_level_tables(case):
    im, t = case.im, case.t
    lvl, col_lvl, sn_lvl = im.array("l.lvl_ptr", "u4"), im.array("l.col_lvl_ptr", "u4"), im.array("l.sn_lvl_ptr", "u4")
    lp, cp = im.array("lvl_pack", "u4"), im.array("col_lvl_pack", "u4")
    assert len(lp) == len(lvl) and len(cp) == len(col_lvl)
    assert np.array_equal(lp & 0xffff, lvl) and np.array_equal(lp >> 16, sn_lvl)
    assert np.array_equal(cp & 0xffff, col_lvl) and np.array_equal(cp >> 16, sn_lvl)
    bwd_ptr, col_sn = im.array("l.bwd_ptr", "u4"), im.array("l.col_sn", "u4")
    rng = im.array("bwd_range", "u4", 2)
    assert len(rng) == len(im.array("l.col_perm", "u4"))
    expect = np.zeros_like(rng)
    for ti in range(case.n_tasks):
        cols = t["col_off"][ti] + np.arange(t["n_col"][ti])
        ptr = t["colptr_off"][ti] + np.arange(t["n_col"][ti])
        cs = col_sn[cols]
        expect[cols, 0] = bwd_ptr[ptr] + ((cs >> 8) - (cs & 0xff) - 1).astype(np.uint32)
        expect[cols, 1] = bwd_ptr[ptr + 1]
    assert np.array_equal(rng, expect)
    assert im.level_tables_throw_at(0xffff) == 0
    assert im.level_tables_throw_at(0x10000) == 1


@pytest.mark.parametrize("batch,split", [(1, True), (4096, False)])
def test_template_tables(case, batch, split):
    im = case.im
    n_groups, threads = 3, 16  # (workgroups of 16 lanes: the bigger family takes two per row group)
    n_fam = im.template_tables(batch, threads, n_groups, max_members=25)
    tp = {f: v.astype(np.int64) for f, v in im.tasks("tape.tasks", TAPE_FIELDS).items()}
    fam_ptr, fam_tasks = im.array("tmpl.family_ptr", "u4"), im.array("tmpl.family_tasks", "u4")
    sizes = np.diff(fam_ptr.astype(np.int64))
    if case.model == ("cart_pole", 37):  # cart-pole N = 37: its 37 interior stages as families of 25 and 12
        assert n_fam == 2 and sizes.tolist() == [25, 12]
    inst = im.array("tmpl.inst", "u4")
    table = [im.array("tmpl.table0", "u4", 4), im.array("tmpl.table1", "u4", 4)]
    blocks = im.array("tmpl.blocks", "u4")
    words = {k: im.array("tape." + k, "u4") for k in ("leaf_src", "vout_dst", "vout_scale", "jout_dst", "jout_scale")}
    off, first = 0, [0, 0]
    for f in range(n_fam):
        tasks = fam_tasks[fam_ptr[f]:fam_ptr[f + 1]]
        n_inst, rep = len(tasks), tasks[0]
        nl, nv, nj = tp["n_leaf"][rep], tp["n_vout"][rep], tp["n_jout"][rep]
        rows = nl + 2 * nv + 2 * nj
        got = inst[off:off + rows * n_inst].reshape(rows, n_inst)
        for i, ti in enumerate(tasks):
            lo, vo, jo = tp["leaf_off"][ti], tp["vout_off"][ti], tp["jout_off"][ti]
            col = np.concatenate([words["leaf_src"][lo:lo + nl], words["vout_dst"][vo:vo + nv], words["vout_scale"][vo:vo + nv],
                                  words["jout_dst"][jo:jo + nj], words["jout_scale"][jo:jo + nj]])
            assert np.array_equal(got[:, i], col), (f, i)
        waves = (n_inst + threads - 1) // threads
        mode = [0, n_groups if split else -1]
        for m in range(2):
            assert table[m][f].tolist() == [first[m], n_inst, off, mode[m] & 0xffffffff], (f, m)
            first[m] += waves * max(1, mode[m])
        off += rows * n_inst
    assert off == len(inst) and blocks.tolist() == first
    assert im.scalar("tmpl.n_templated_tasks") == int(sizes.sum())


def test_interleaved_meta(case):
    im, t = case.im, case.t
    S, W = im.scalar("kIlSlots"), im.scalar("kIlW")
    meta, meta_off = im.array("il.meta", "u4"), im.array("il.meta_off", "u4")
    pairs = im.array("l.pairs", "u2", 4)
    pair_ptr, cptr, cidx = im.array("l.ent_pair_ptr", "u4"), im.array("l.ent_contrib_ptr", "u4"), im.array("l.contrib_idx", "u4")
    ent_src, ent_out = im.array("l.ent_src", "i4").view("u4"), im.array("l.ent_out", "u4")
    flags, col = im.array("l.ent_flags", "u1"), im.array("l.ent_col", "u2")
    ext_dst, lvl = im.array("l.ext_dst", "u4"), im.array("l.lvl_ptr", "u4")
    assert len(meta_off) == case.n_tasks
    fbytes = colmax = solve = 0
    for ti in range(case.n_tasks):
        g = {f: int(v[ti]) for f, v in t.items()}
        at = int(meta_off[ti])
        n_cref, n_words = int(meta[at]), int(meta[at + 1])
        assert n_cref == cptr[g["contrib_ptr_off"] + g["n_ent"]]
        assert n_words == 2 * g["n_pairs"] + (g["n_ent"] + g["n_ext"] + 1) + 3 * g["n_ent"] + g["n_ext"] + g["n_lvl"] + 1 + S + 1 + 2 * n_cref
        assert at + 2 + n_words == (int(meta_off[ti + 1]) if ti + 1 < case.n_tasks else len(meta))
        w = meta[at + 2:at + 2 + n_words]
        pos = 0

        def take(count):
            nonlocal pos
            pos += count
            return w[pos - count:pos]

        pw = take(2 * g["n_pairs"]).reshape(-1, 2)
        pl = pairs[g["pair_off"]:g["pair_off"] + g["n_pairs"]]
        assert np.array_equal(pw[:, 0] & 0xffff, pl[:, 0]) and np.array_equal(pw[:, 0] >> 16, pl[:, 1]) and np.array_equal(pw[:, 1], pl[:, 2])
        assert np.array_equal(take(g["n_ent"] + g["n_ext"] + 1), pair_ptr[g["pair_ptr_off"]:g["pair_ptr_off"] + g["n_ent"] + g["n_ext"] + 1])
        ents = slice(g["ent_off"], g["ent_off"] + g["n_ent"])
        assert np.array_equal(take(g["n_ent"]), ent_src[ents])
        assert np.array_equal(take(g["n_ent"]), ent_out[ents])
        fc = take(g["n_ent"])
        assert np.array_equal(fc & 0xff, flags[ents]) and np.array_equal(fc >> 8, col[ents])
        assert np.array_equal(take(g["n_ext"]), ext_dst[g["ext_off"]:g["ext_off"] + g["n_ext"]])
        assert np.array_equal(take(g["n_lvl"] + 1), lvl[g["lvl_off"]:g["lvl_off"] + g["n_lvl"] + 1])
        crptr = take(S + 1)
        refs = take(2 * n_cref).reshape(-1, 2)
        assert pos == n_words and crptr[0] == 0 and crptr[S] == n_cref
        tc = cptr[g["contrib_ptr_off"]:g["contrib_ptr_off"] + g["n_ent"] + 1]
        for sl in range(S):  # every (entry, update slot) once, under slot e % kIlSlots, in plan order
            expect = [(e, int(cidx[g["contrib_off"] + q])) for e in range(sl, g["n_ent"], S) for q in range(tc[e], tc[e + 1])]
            assert refs[crptr[sl]:crptr[sl + 1]].tolist() == [list(r) for r in expect], (ti, sl)
        fbytes = max(fbytes, max((g["n_ent"] + g["n_col"]) * W * 8, 3 * S * W * 8) + 4 * n_words + 16)
        colmax = max(colmax, g["n_col"] + 1)
        solve = max(solve, g["n_col"] * 64 * 8 + 4 * (3 * g["n_col"] + g["n_lvl"] + 4) + 8 * g["n_bwd_items"] + 16)
    assert im.scalar("il.factor_lds") == fbytes
    assert im.scalar("il.solve_lds") == max(colmax * 64 * 8, solve)


def kkt_term_values(case, terms):
    """The addends of a block of KktTerm rows (device_layout.h), evaluated the way hc_assemble / hc_rhs evaluate theirs."""
    V, s, y, z, mu = case.V, case.s, case.y, case.z, case.mu
    kind, row = terms[:, 1] >> 28, terms[:, 1] & 0x0fffffff
    out = np.zeros(len(terms))
    for q, (a, _, c) in enumerate(terms):
        k, r = kind[q], row[q]
        if k <= 1:
            out[q] = V[a]
        elif k == 2:
            out[q] = V[a] * y[r]
        else:
            sinv = 1.0 / s[r]
            sigma = sinv * z[r]
            out[q] = V[a] * (-sigma * V[c] + mu * sinv + z[r]) if k == 3 else (V[a] * sigma) * V[c]
    return kind, out


def test_inline_kkt_terms_by_value(case):
    im, t = case.im, case.t
    assert im.scalar("kkt.ok") == 1
    vsrc, terms, task_terms = im.array("kkt.vsrc", "i4"), im.array("kkt.terms", "i4", 3), im.array("kkt.task_terms", "u4", 2)
    ent_src, flags = im.array("l.ent_src", "i4"), im.array("l.ent_flags", "u1")
    n, off_ce = im.scalar("k.n"), im.scalar("s.off_ce")
    assert np.all(task_terms % 3 == 0)  # 16-byte groups of 12-byte terms: a multiple of four terms
    owner = task_of_entry(case)
    widest = int(task_terms[:, 1].max())
    assert im.scalar("kkt.factor_lds") == im.scalar("l.factor_lds_bytes") + 16 + 16 * widest + 8 * (widest * 4 // 3)
    seen_sum = seen_neg = most_terms = 0
    for e in np.flatnonzero((ent_src >= 0) & (owner >= 0)):
        src, v, is_rhs = int(ent_src[e]), int(vsrc[e]), bool(flags[e] & 4)
        want = case.rhs[src] if is_rhs else case.lhs[src]
        if v >= 0:  # a plain copy; bit 30: negated (a c_e row of the right-hand side)
            neg = bool(v & (1 << 30))
            assert neg == (is_rhs and src >= n)
            if neg:
                assert (v & ~(1 << 30)) == off_ce + src - n
                seen_neg += 1
            got = -case.V[v & ~(1 << 30)] if neg else case.V[v]
            assert got == want, (e, v)
        elif v == -1:
            assert want == 0.0, e
        else:
            code = -(v + 2)
            first, cnt = code & 0xfffff, code >> 20
            base = int(task_terms[owner[e], 0]) * 4 // 3
            assert first + cnt <= int(task_terms[owner[e], 1]) * 4 // 3
            kind, val = kkt_term_values(case, terms[base + first:base + first + cnt])
            assert np.all(kind <= 4) and np.all(np.isin(kind, [1, 2, 3]) if is_rhs else np.isin(kind, [0, 4]))
            tot = lambda k: float(val[kind == k].sum())
            got = -tot(1) + tot(2) + tot(3) if is_rhs else tot(0) + tot(4)
            assert abs(got - want) <= (cnt + 1) * EPS * float(np.abs(val).sum()), (e, got, want)
            seen_sum += 1
            most_terms = max(most_terms, cnt)
    assert seen_sum > 0 and seen_neg == case.hc.m_e
    # (the hub's row of the right-hand side: one gradient term, 255 of A_e^T y, 127 of A_i^T)
    assert most_terms > 100 or case.model != ("step", "hub530_255_127")


def test_backsub_rows_by_value(case):
    im, t = case.im, case.t
    assert im.scalar("bs.ok") == 1
    plan, task_plan = im.array("bs.plan", "u4", 2), im.array("bs.task_plan", "u4", 4)
    perm, col_perm = im.array("l.perm", "i4"), im.array("l.col_perm", "u4")
    m_i, off_ci = im.scalar("k.m_i"), im.scalar("s.off_ci")
    round_of_col = np.zeros(im.scalar("l.n"), dtype=np.int64)  # by permuted column
    for ti in range(case.n_tasks):
        round_of_col[col_perm[t["col_off"][ti]:t["col_off"][ti] + t["n_col"][ti]]] = t["round"][ti]
    widest = int(task_plan[:, 1].max())
    assert im.scalar("bs.solve_lds") == im.scalar("l.solve_lds_bytes") + 16 + 16 * widest
    V, s, z, mu, p = case.V, case.s, case.z, case.mu, case.p
    rows_seen, n_ancestor_refs = [], 0
    for ti in range(case.n_tasks):
        off16, len16, n_rows, rows16 = (int(v) for v in task_plan[ti])
        assert rows16 == (n_rows + 1) // 2
        block = plan[2 * off16:2 * (off16 + len16)]
        tail = block[2 * rows16:]
        for r, word in block[:n_rows]:
            r, first, cnt = int(r), int(word) & 0xfffff, int(word) >> 20
            rows_seen.append(r)
            addends = []
            for a, ref in tail[first:first + cnt]:
                if ref & 0x80000000:  # a permuted column of a task of a later round
                    pj = int(ref & 0x7fffffff)
                    assert round_of_col[pj] > t["round"][ti], (ti, r)
                    n_ancestor_refs += 1
                else:  # a local column of this task
                    assert ref < t["n_col"][ti]
                    pj = int(col_perm[t["col_off"][ti] + int(ref)])
                addends.append(V[int(a)] * p[perm[pj]])
            ci_s = V[off_ci + r] - s[r]
            ps = ci_s + float(np.sum(addends))
            sinv = 1.0 / s[r]
            pz = mu * sinv - z[r] - (sinv * z[r]) * ps
            # a sum of cnt + 1 addends taken in another order; p_z = mu / s - z - (z / s) p_s: that error times z / s
            # and the rounding of its own three operations
            bound = (cnt + 2) * EPS * (abs(ci_s) + float(np.sum(np.abs(addends))))
            assert abs(ps - case.ps[r]) <= bound, (r, ps, case.ps[r])
            assert abs(pz - case.pz[r]) <= sinv * z[r] * bound + 3 * EPS * (mu * sinv + z[r] + sinv * z[r] * abs(ps)), (r, pz, case.pz[r])
    assert sorted(rows_seen) == list(range(m_i))  # each row of A_i in exactly one task
    assert n_ancestor_refs > 0 or case.model[0] != "gfold"
    # (the hub's rows h^2 + x_j^2 <= 4 belong to the task of x_j; the hub is eliminated last, in the root task)
    assert n_ancestor_refs > 0 or case.model not in (("step", "chain130"), ("step", "hub530_255_127"))


def test_multifrontal_images(case):
    im, t, m = case.im, case.t, case.m
    from tests.support import imagecheck

    assert im.scalar("l.mf") == 1 and im.scalar("mf.declined") == 0
    G = im.scalar("kMfImageGroups")
    stride16 = im.scalar("mf.stride16")
    img, desc = im.array("mf.image", "u1"), im.array("mf.desc", "u4", 4)
    carve = im.array("mf.carve", "u4", 16).astype(np.int64)
    cv = {name: carve[:, i] for i, name in enumerate(imagecheck.CARVE)}
    plan = {k: im.array("l." + k, dt) for k, dt in
            [("mf_tab", "u2"), ("mf_lvl_ptr", "u4"), ("mf_ext", "u4"), ("mf_cent", "u2"), ("mf_contrib_ptr", "u4"),
             ("mf_contrib_idx", "u4"), ("col_perm", "u4"), ("mf_anc", "u4"), ("ent_flags", "u1")]}
    fronts = im.array("l.mf_fronts", "u1", 16)
    vsrc, terms, task_terms = im.array("kkt.vsrc", "i4"), im.array("kkt.terms", "u1"), im.array("kkt.task_terms", "u4", 2)
    bs_plan, bs_task = im.array("bs.plan", "u1"), im.array("bs.task_plan", "u4", 4)
    fb, ab, bb = (im.scalar(k) for k in ("kMfTermFirstBits", "kMfTermABits", "kMfTermBBits"))
    assert len(img) == 16 * (stride16 * case.n_tasks + G) and 1 <= stride16 <= G
    align16 = lambda v: (v + 15) & ~15
    longest = lds = recoded = 0
    kinds_seen = set()
    for ti in range(case.n_tasks):
        g = {f: int(v[ti]) for f, v in t.items()}
        mm = {f: int(v[ti]) for f, v in m.items()}
        o = {name: int(v[ti]) for name, v in cv.items()}
        slot = img[16 * stride16 * ti:16 * stride16 * (ti + 1)]
        region = lambda at, nbytes: slot[at - o["o_tab"]:at - o["o_tab"] + nbytes]
        same = lambda at, arr: np.array_equal(region(at, arr.nbytes), np.ascontiguousarray(arr).view("u1").ravel())
        assert same(o["o_tab"], plan["mf_tab"][mm["tab_off"]:mm["tab_off"] + mm["n_tab"]])
        assert same(o["o_lvl"], plan["mf_lvl_ptr"][g["lvl_off"]:g["lvl_off"] + g["n_lvl"] + 1])
        assert same(o["o_ext"], plan["mf_ext"][mm["ext_off"]:mm["ext_off"] + mm["n_ext"]])
        cent = plan["mf_cent"][mm["cent_off"]:mm["cent_off"] + mm["n_cent"]]
        fl = plan["ent_flags"][g["ent_off"]:g["ent_off"] + g["n_ent"]].copy()
        assert not np.any(fl & 0x20)
        fl[cent] |= 0x20  # bit 5 on exactly the entries that take update slots
        assert same(o["o_flags"], fl)
        assert same(o["o_cent"], cent)
        assert same(o["o_cptr"], plan["mf_contrib_ptr"][mm["contrib_ptr_off"]:mm["contrib_ptr_off"] + mm["n_cent"] + 1])
        assert same(o["o_cidx"], plan["mf_contrib_idx"][mm["contrib_off"]:mm["contrib_off"] + mm["n_contrib_idx"]])
        assert same(o["o_cp"], plan["col_perm"][g["col_off"]:g["col_off"] + g["n_col"]])
        assert same(o["o_anc"], plan["mf_anc"][mm["anc_off"]:mm["anc_off"] + mm["n_anc"]])
        assert same(o["o_fr"], fronts[mm["front_off"]:mm["front_off"] + mm["n_front"]])
        counters = region(o["o_cnt"], o["o_terms"] - o["o_cnt"]).copy()
        assert counters[16:24].view("u8")[0] == 0x7ff0000000000000  # the smallest |d| starts at +inf
        counters[16:24] = 0
        assert not counters.any()
        # the source words: plain copies and zeros as they were, a sum re-encoded with its counts per kind
        words = region(o["o_src"], 4 * g["n_ent"]).view("i4")
        for i in range(g["n_ent"]):
            v, w = int(vsrc[g["ent_off"] + i]), int(words[i])
            if v >= -1:
                assert w == v
                continue
            c0, c1 = -(v + 2), -(w + 2)
            first, n_a = c1 & ((1 << fb) - 1), (c1 >> fb) & ((1 << ab) - 1)
            n_b, has_g = (c1 >> (fb + ab)) & ((1 << bb) - 1), c1 >> (fb + ab + bb)
            assert first == (c0 & 0xfffff) and has_g <= 1 and has_g + n_a + n_b == c0 >> 20, (ti, i)
            recoded += 1
            kinds_seen |= {name for name, met in (("more b than a", n_b > n_a), ("products only", has_g == 0 and n_a == 0),
                                                  ("the widest word", (n_a, n_b) == ((1 << ab) - 1, (1 << bb) - 1))) if met}
        terms16, bs16 = int(task_terms[ti, 1]), int(bs_task[ti, 1])
        end_terms = o["o_terms"] + 16 * terms16
        assert np.array_equal(region(o["o_terms"], 16 * terms16), terms[16 * int(task_terms[ti, 0]):][:16 * terms16])
        assert np.array_equal(region(end_terms, 16 * bs16), bs_plan[16 * int(bs_task[ti, 0]):][:16 * bs16])
        blob = end_terms - o["o_tab"] + 16 * bs16
        assert not slot[blob:].any()
        assert desc[ti].tolist() == [0, (end_terms - o["o_tab"]) // 16, bs16, terms16]
        longest = max(longest, blob // 16)
        lds = max(lds, align16(end_terms + 8 * (terms16 * 4 // 3)) + 16 * bs16)
    assert stride16 == max(1, longest) and recoded > 0
    assert im.scalar("mf.lds") == align16(lds) + 16
    assert im.mf_declines_short_task_terms() == 1
    # the words kkt_terms_sum_grouped walks otherwise than on the benchmark models: (hub, hub) of the matrix has its direct
    # terms and one product per inequality row of the hub (n_b > n_a); (hub, j) of a row h^2 + x_j^2 <= 4 is that row's
    # product and nothing else (no gradient term, n_a = 0); the hub's row of the right-hand side of hub530_255_127 fills
    # both count fields of the word (n_a = 255, n_b = 127, the fields' widths asserted here)
    if case.model[0] == "step":
        assert {"more b than a", "products only"} <= kinds_seen
    if case.model == ("step", "hub530_255_127"):
        assert (ab, bb) == (8, 7) and "the widest word" in kinds_seen


def test_one_reader_per_slot_and_diagonal_positions(case):
    im, t = case.im, case.t
    cidx = im.array("l.contrib_idx", "u4")
    readers = np.zeros(max(1, im.scalar("l.n_contrib")), dtype=np.int64)
    for ti in range(case.n_tasks):
        np.add.at(readers, cidx[t["contrib_off"][ti]:t["contrib_off"][ti] + t["n_contrib_idx"][ti]], 1)
    assert im.scalar("one_reader") == int(readers.max() <= 1)
    colptr, rowidx = im.array("k.lhs.colptr", "i4"), im.array("k.lhs.rowidx", "i4")
    n = im.scalar("k.n")
    diag = im.array("diag_pos", "i4")
    assert len(diag) == max(1, n)
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    on_diag = np.flatnonzero(rowidx == cols)
    assert np.array_equal(diag[:n], on_diag[cols[on_diag] < n])  # (one diagonal entry per column: the lhs has a full diagonal)
