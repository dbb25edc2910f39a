"""CPU tier of the full vjp (include/slpx.h: the full vjp): cotangents on the whole end iterate and on the optimal cost.
The two maps the plan gains (sleipnir_amd/csrc/sens_plan.hpp: g_src, fp_src) and the host executors of the new row
formulas of sens_rows.h — the bodies sens_adjoint_rhs_kernel and sens_vjp_full_kernel run — against dense numpy, on
values from a seeded generator as in test_sensitivity_plan_cpu.py.  No device (tests/support/sensadjcheck.py).

Models: tests/support/param_models.py (m2, boxed, mq, chain(4), chain(8)).

TOLERANCE 1e-13 relative to the largest entry, as test_sensitivity_plan_cpu.py derives it for sums of this kind: every
output is a sum of at most a few dozen products of O(1) numbers, summed here in the plan's order and by numpy in its own.
The adjoint identity is asked to 1e-12: it goes through two dense solves with a matrix of condition number 2."""
import numpy as np
import pytest

from tests.support import param_models as pmod
from tests.support import sensadjcheck, senscheck

TOL = 1e-13
BLOCKS = sensadjcheck.BLOCKS


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
# which cotangents are present: each of the five alone, all five together (and "x": the old vjp's)
SUBSETS = [("x",), ("s",), ("y",), ("z",), ("cost",), BLOCKS]


def close_to(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
    err = float(np.max(np.abs(got - want))) / scale if want.size else 0.0
    assert err <= TOL, (what, err)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Case:
    """a model's plan, both probes, and seeded values for everything the executors read"""

    def __init__(self, m, case):
        self.pm = BUILD[case](m)
        self.sc = sc = senscheck.SensCheck(self.pm.p.p)
        self.sa = sensadjcheck.SensAdjCheck(self.pm.p.p, sc)
        rng = np.random.default_rng(20240 + len(case))
        self.Vx, self.V = rng.uniform(-1.0, 1.0, sc.nVx), rng.uniform(-1.0, 1.0, sc.nV)
        self.s, self.z = rng.uniform(0.5, 2.0, sc.m_i), rng.uniform(0.5, 2.0, sc.m_i)
        self.dp, self.w = rng.uniform(-1.0, 1.0, sc.n_p), rng.uniform(-1.0, 1.0, sc.dim)
        sizes = {"x": sc.n, "s": sc.m_i, "y": sc.m_e, "z": sc.m_i, "cost": 1}
        self.v = {k: rng.uniform(-1.0, 1.0, sizes[k]) for k in BLOCKS}
        self.rng = rng

    def subset(self, keys):
        return {k: self.v[k] for k in keys}

    def close(self):
        self.sa.close()
        self.sc.close()
        self.pm.close()


@pytest.mark.parametrize("case", list(BUILD))
def test_executors_against_dense_numpy(m, case):
    c = Case(m, case)
    M, R = c.sc.rhs(c.Vx, c.V, c.s, c.z)
    for keys in SUBSETS:
        v = c.subset(keys)
        want = sensadjcheck.dense_adjoint(c.sa, c.Vx, c.V, c.s, c.z, c.w, v)
        close_to(c.sa.adjoint_rhs(c.V, c.s, c.z, v), want["rhs"], ("rhs", keys))
        close_to(c.sa.vjp_full(c.Vx, M, R, c.s, c.z, c.w, v), want["grad"], ("grad", keys))
    c.close()


@pytest.mark.parametrize("case", list(BUILD))
def test_the_two_maps(m, case):
    c = Case(m, case)
    n, n_p = c.sc.n, c.sc.n_p
    g_src, fp_src = c.sa.array("g_src"), c.sa.array("fp_src")
    assert len(g_src) == n and len(fp_src) == n_p
    for src, cp, off, first in ((g_src, c.sa.array("model.g.colptr"), c.sa.scalar("model.off_g"), 0),
                                (fp_src, c.sa.array("ext.g.colptr"), c.sa.scalar("ext.off_g"), n)):
        assert len(cp) == first + len(src) + 1
        structural = []
        for i in range(len(src)):
            entries = list(range(off + cp[first + i], off + cp[first + i + 1]))
            assert len(entries) <= 1
            # -1 exactly where the pattern has no entry, the entry's position otherwise
            assert (int(src[i]) == -1) == (not entries)
            if entries:
                assert int(src[i]) == entries[0]
                structural.append(entries[0])
        named = [int(v) for v in src if v >= 0]
        assert sorted(named) == sorted(structural) and len(named) == len(set(named)), "an entry is named twice or not at all"
    # parameters the cost does not reach: the bounds of boxed, the row value b of mq; a of m2 and mq is in the cost
    reached = [bool(v >= 0) for v in fp_src]
    if case == "m2":
        assert reached == [True]
    elif case == "boxed":
        assert reached == [False, False]
    elif case == "mq":
        assert reached == [True, False]
    else:  # chain: gain, u_max, x_init, r_k, d_k — the references r_k alone are in the cost
        stages = (n_p - 3) // 2
        assert reached == [False] * 3 + [True] * stages + [False] * stages
    assert all(v >= 0 for v in g_src) or case.startswith("chain")  # (X_0 of the chain is not in the cost)
    c.close()


@pytest.mark.parametrize("case", list(BUILD))
def test_adjoint_identity_on_the_host(m, case):
    """<v, J dp> = <J^T v, dp> with a random symmetric nonsingular K in place of the KKT matrix: forward through
    sens_host_combine / sens_host_expand plus dcost = g . dx + f_p . dp, reverse through the new executors."""
    c = Case(m, case)
    sc, sa = c.sc, c.sa
    M, R = sc.rhs(c.Vx, c.V, c.s, c.z)
    # K = Q diag(+-[1, 2]) Q^T: symmetric, indefinite, condition number 2
    Q, _ = np.linalg.qr(c.rng.normal(size=(sc.dim, sc.dim)))
    K = (Q * (c.rng.uniform(1.0, 2.0, sc.dim) * c.rng.choice([-1.0, 1.0], sc.dim))) @ Q.T
    K = 0.5 * (K + K.T)
    g, f_p = sa.g_dense(c.V), sa.fp_dense(c.Vx)
    rhs, r_i = sc.combine(M, R, c.dp)
    sol = np.linalg.solve(K, rhs)
    dx, ds, dy, dz = sc.expand(c.V, c.s, c.z, sol, r_i)
    forward = {"x": dx, "s": ds, "y": dy, "z": dz, "cost": np.array([g @ dx + f_p @ c.dp])}
    for keys in SUBSETS:
        v = c.subset(keys)
        w = np.linalg.solve(K, sa.adjoint_rhs(c.V, c.s, c.z, v))
        grad = sa.vjp_full(c.Vx, M, R, c.s, c.z, w, v)
        left = sum(float(np.dot(v[k], forward[k])) for k in keys)
        right = float(grad @ c.dp)
        err = abs(left - right) / max(abs(left), abs(right), 1e-300)
        print(f"{case} {keys}: <v, J dp> {left:+.15e}  <J^T v, dp> {right:+.15e}  relative {err:.2e}")
        if left == 0.0 and right == 0.0:  # (a block the model does not have, or a parameter nothing reaches)
            continue
        assert err <= 1e-12, (case, keys, left, right, err)
    c.close()


@pytest.mark.parametrize("case", list(BUILD))
def test_vx_alone_is_the_old_vjp_bit_for_bit(m, case):
    c = Case(m, case)
    M, R = c.sc.rhs(c.Vx, c.V, c.s, c.z)
    v = c.subset(("x",))
    rhs = c.sa.adjoint_rhs(c.V, c.s, c.z, v)
    assert bits_equal(rhs, np.concatenate([c.v["x"], np.zeros(c.sc.m_e)]))
    assert bits_equal(c.sa.vjp_full(c.Vx, M, R, c.s, c.z, c.w, v), c.sc.vjp(R, c.w))
    # -0.0 in vx stays -0.0: nothing is added to it
    vx = c.v["x"].copy()
    vx[0] = -0.0
    assert bits_equal(c.sa.adjoint_rhs(c.V, c.s, c.z, {"x": vx})[:c.sc.n], vx)
    c.close()


def test_classify_extras():
    """status 1 for an instance with a value that is not finite in ANY given array; a null array and one without entries
    are not looked at."""
    B = 4
    a, b, cost = np.ones((B, 3)), np.ones((B, 2)), np.ones(B)
    assert list(sensadjcheck.classify_extras(B, [a, None, b, cost], [3, 5, 2, 1])) == [0, 0, 0, 0]
    b2 = b.copy()
    b2[1, 1] = np.nan
    cost2 = cost.copy()
    cost2[3] = np.inf
    assert list(sensadjcheck.classify_extras(B, [a, None, b2, cost2], [3, 5, 2, 1])) == [0, 1, 0, 1]
    assert list(sensadjcheck.classify_extras(B, [a, np.zeros((B, 0)), b2], [3, 0, 2])) == [0, 1, 0, 0]
    assert list(sensadjcheck.classify_extras(B, [], [])) == [0, 0, 0, 0]


def test_entry_points_fail_loudly(m, slpx):
    """-100 + slpx_last_error: a null problem; without a device, that; with one, no cotangent / nothing solved yet."""
    import ctypes

    L = slpx.lib()
    pm = BUILD["mq"](m)
    h = pm.p.p._h
    out, rows = np.zeros(8), np.zeros((1, 8))
    cot = slpx.Cotangent()
    cot.vcost = out.ctypes.data
    size = ctypes.sizeof(cot)
    assert L.slpx_problem_sensitivity_vjp_full(None, ctypes.byref(cot), size, out.ctypes.data, None) == -100
    assert b"null problem" in L.slpx_last_error()
    r = rows.ctypes.data
    assert L.slpx_problem_sensitivity_batch_vjp_full(None, 1, r, r, r, r, r, r, ctypes.byref(cot), size, r, None, None) == -100
    assert b"null problem" in L.slpx_last_error()
    device = L.slpx_device_count() >= 1
    assert L.slpx_problem_sensitivity_vjp_full(h, ctypes.byref(cot), size, out.ctypes.data, None) == -100
    assert (b"has not been solved" if device else b"no HIP device") in L.slpx_last_error(), L.slpx_last_error()
    empty = slpx.Cotangent()
    assert L.slpx_problem_sensitivity_vjp_full(h, ctypes.byref(empty), size, out.ctypes.data, None) == -100
    assert (b"no cotangent" if device else b"no HIP device") in L.slpx_last_error(), L.slpx_last_error()
    assert pm.p.p.compile_count() == 0
    pm.close()
