"""CPU tier of the solution sensitivities: the sensitivity plan (sleipnir_amd/csrc/sens_plan.hpp) and its host executor —
the row formulas of sens_rows.h, the bodies the kernels of sensitivity.hip run — against a dense numpy evaluation of the
same formulas, on values from a seeded generator.  No device: the plan is a pure function of the two structures'
patterns (tests/support/senscheck.py).

Models: tests/support/param_models.py (m2, boxed, mq, chain(4), chain(8): the family-generated body).

TOLERANCE 1e-13 relative to the largest entry: every output is a sum of at most a few dozen products of O(1) numbers
(uniform in [-1, 1], slacks and multipliers in [0.5, 2]), summed here in the plan's order and by numpy in its own."""
import numpy as np
import pytest

from tests.support import param_models as pmod
from tests.support import senscheck

TOL = 1e-13


@pytest.fixture
def m(fresh):
    mm = pmod.new_model()
    mm.be.reset()
    return mm


BUILD = {
    "m2": lambda m: pmod.m2(m, (2.0,)),
    "boxed": lambda m: pmod.boxed(m, (0.0, 2.0)),
    "mq": lambda m: pmod.mq(m, (2.0, 1.0)),
    "chain4": lambda m: pmod.chain(m, 4, pmod.chain_rows(4, 1)[0]),
    "chain8": lambda m: pmod.chain(m, 8, pmod.chain_rows(8, 1)[0]),
}


def close_to(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
    err = float(np.max(np.abs(got - want))) / scale if want.size else 0.0
    assert err <= TOL, (what, err)


@pytest.mark.parametrize("case", list(BUILD))
def test_plan_and_executor_against_dense_numpy(m, case):
    pm = BUILD[case](m)
    sc = senscheck.SensCheck(pm.p.p)
    n, me, mi = pm.p.p.dims
    assert (sc.n, sc.m_e, sc.m_i, sc.n_p) == (n, me, mi, len(pm.params))
    assert (sc.dim, sc.dimM) == (n + me, n + me + mi)
    # the parameters are variables of the extended structure: it has none left; and the system made of it builds
    assert sc.scalar("ext.parameters") == 0
    assert sc.scalar("ext.system.dim") == n + sc.n_p + me and sc.scalar("ext.system.has_device") == 0
    rng = np.random.default_rng(20240 + len(case))
    Vx, V = rng.uniform(-1.0, 1.0, sc.nVx), rng.uniform(-1.0, 1.0, sc.nV)
    s, z = rng.uniform(0.5, 2.0, mi), rng.uniform(0.5, 2.0, mi)
    dp, sol, w = rng.uniform(-1.0, 1.0, sc.n_p), rng.uniform(-1.0, 1.0, sc.dim), rng.uniform(-1.0, 1.0, sc.dim)
    want = senscheck.dense_reference(sc, Vx, V, s, z, dp, sol, w)
    M, R = sc.rhs(Vx, V, s, z)
    close_to(M, want["M"], "M")
    close_to(R, want["R"], "R")
    rhs, r_i = sc.combine(M, R, dp)
    close_to(rhs, want["rhs"], "R dp")
    close_to(r_i, want["r_i"], "r_i dp")
    dx, ds, dy, dz = sc.expand(V, s, z, sol, r_i)
    for name, got in (("dx", dx), ("ds", ds), ("dy", dy), ("dz", dz)):
        close_to(got, want[name], name)
    close_to(sc.vjp(R, w), want["grad"], "w^T R")
    sc.close()
    pm.close()


@pytest.mark.parametrize("case", list(BUILD))
def test_every_cross_entry_once_and_no_entry_of_the_pp_block(m, case):
    pm = BUILD[case](m)
    sc = senscheck.SensCheck(pm.p.p)
    n, n_p = sc.n, sc.n_p
    cross, pp = [], set()
    for name in ("ext.Hf", "ext.Hc"):
        cp, ri, off = sc.pattern(name)
        assert len(cp) == n + n_p + 1
        for c in range(n + n_p):
            for t in range(cp[c], cp[c + 1]):
                assert ri[t] >= c, "lower triangle"
                if c >= n:
                    pp.add(off + t)
                elif ri[t] >= n:
                    cross.append(((ri[t] - n) * sc.dimM + c, off + t))
    for name, first in (("ext.Ae", n), ("ext.Ai", n + sc.m_e)):
        cp, ri, off = sc.pattern(name)
        for c in range(n, n + n_p):
            for t in range(cp[c], cp[c + 1]):
                cross.append(((c - n) * sc.dimM + first + ri[t], off + t))
    m_ptr, m_src = sc.array("m_ptr"), sc.array("m_src")
    assert len(m_ptr) == n_p * sc.dimM + 1 and m_ptr[0] == 0 and m_ptr[-1] == len(m_src)
    got = [(k, int(m_src[t])) for k in range(n_p * sc.dimM) for t in range(m_ptr[k], m_ptr[k + 1])]
    assert len(got) == len(set(src for _, src in got)), "an entry of V' is read twice"
    assert sorted(got) == sorted(cross), "the plan's sources are not the structural non-zeros of the cross blocks"
    assert len(cross) > 0 and not pp & set(int(v) for v in m_src), "an entry of the p-p block is read"
    # the model has cross terms of every kind where its blocks exist: a parameter in the cost, in an equality row, ...
    kinds = {("x" if k % sc.dimM < n else "e" if k % sc.dimM < sc.dim else "i") for k, _ in got}
    assert kinds == {"m2": {"x"}, "boxed": {"i"}, "mq": {"x", "e"}}.get(case, {"x", "e", "i"})
    # the reduction and the expansion name every entry of A_i once each
    cp, ri, off = sc.pattern("model.Ai")
    assert list(sc.array("red_ptr")) == list(cp) and list(sc.array("red_row")) == list(ri)
    assert list(sc.array("red_src")) == list(range(off, off + len(ri)))
    rowptr, col, src = sc.array("ai_rowptr"), sc.array("ai_col"), sc.array("ai_src")
    assert sorted(int(v) for v in src) == list(range(off, off + len(ri)))
    for j in range(sc.m_i):
        cols = list(col[rowptr[j]:rowptr[j + 1]])
        assert cols == sorted(cols)
        for t in range(rowptr[j], rowptr[j + 1]):
            q = src[t] - off
            assert ri[q] == j and cp[col[t]] <= q < cp[col[t] + 1]
    sc.close()
    pm.close()


def test_entry_points_fail_loudly(m, slpx):
    """-100 + slpx_last_error: a null problem; without a device, that; with one, that nothing was solved yet."""
    L = slpx.lib()
    pm = BUILD["mq"](m)
    h = pm.p.p._h
    out = np.zeros(8)
    assert L.slpx_problem_sensitivity(None, None, None, None, None, None) == -100 and b"null problem" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_rhs(None, None) == -100 and b"null problem" in L.slpx_last_error()
    why = b"no HIP device" if L.slpx_device_count() < 1 else b"has not been solved"
    for call in (lambda: L.slpx_problem_sensitivity(h, out.ctypes.data, None, None, None, None),
                 lambda: L.slpx_problem_sensitivity_jvp(h, out.ctypes.data, out.ctypes.data, None, None, None, None),
                 lambda: L.slpx_problem_sensitivity_vjp(h, out.ctypes.data, out.ctypes.data, None),
                 lambda: L.slpx_problem_sensitivity_rhs(h, out.ctypes.data)):
        assert call() == -100 and why in L.slpx_last_error(), L.slpx_last_error()
    assert pm.p.p.compile_count() == 0
    pm.close()


def test_the_family_path_serves_the_extended_structure(m):
    """chain(8): the dynamics rows are a family in the model (kTapeFamilyMin = 8) and stay one with the parameters as
    variables; chain(4) has none either way."""
    pm = BUILD["chain8"](m)
    sc = senscheck.SensCheck(pm.p.p)
    assert sc.scalar("model.full.shared_tasks") > 0 and sc.scalar("ext.full.shared_tasks") > 0
    sc.close()
    pm.close()
    pm = BUILD["chain4"](m)
    sc = senscheck.SensCheck(pm.p.p)
    assert sc.scalar("model.full.shared_tasks") == 0 and sc.scalar("ext.full.shared_tasks") == 0
    sc.close()
    pm.close()
