"""GPU tier: the residual of a solve in double-double and its iterative refinement (slpx_ldlt_residual,
slpx_ldlt_refine) on one problem — the kernel against the host body of row_residual bit for bit, what refinement
buys against a numpy restatement, the harness's own host-side refinement done by the product, the dense branch, and
the edge cases."""
import numpy as np
import pytest

import sleipnir_amd as sa
from sleipnir_amd.optimization import Problem
from tests.support import cases, parity
from tests.support import refine_cases as rc

pytestmark = pytest.mark.gpu


def _factor_solve(system, reg, n, m_e):
    """slpx_ldlt_factor with the pair given, then a solve; returns the pair used.  Where the fixture's pair is (0, 0)
    and the product's unpivoted plan has a structurally zero pivot there, the pair is the next rung of the fixture's
    own ladder, (1e-4, 1e-10): the attempt the regularization policy makes in its place."""
    if tuple(reg) == (0.0, 0.0) and system.info["struct_singular"]:
        reg = rc.REG
    stats = system.factor(reg[0], reg[1])
    assert tuple(int(v) for v in stats[0, :4]) == (n, m_e, 0, 0), stats
    system.solve()
    return reg


def _check_bits(system, reg):
    r_host, lhs, rhs, p = rc.host_residual(system, reg)
    r, norm = system.residual()
    assert rc.same_bits(r[0], r_host), float(np.max(np.abs(r[0] - r_host)))
    assert rc.same_bits(norm[0], np.max(np.abs(r_host)))
    # the residual reads: lhs, rhs and p are what they were
    assert rc.same_bits(system.get("lhs")[0], lhs) and rc.same_bits(system.get("rhs")[0], rhs) and rc.same_bits(system.get("p")[0], p)
    return lhs, rhs, p


@pytest.mark.parametrize("name", rc.FIXTURES)
def test_kernel_equals_host_body_on_the_fixtures(name):
    """Through a problem's System, then through System.linear_solver on the same pattern and values."""
    pp, system, reg = rc.fixture_system(name)
    n, m_e = system.info["n"], system.info["m_e"]
    reg = _factor_solve(system, reg, n, m_e)
    lhs, rhs, _ = _check_bits(system, reg)
    cp, ri = system.pattern(5)
    ls = sa.System.linear_solver(n, m_e, cp, ri)
    ls.set_matrix(lhs)
    ls.set_rhs(rhs)
    assert _factor_solve(ls, reg, n, m_e) == reg
    _check_bits(ls, reg)
    ls.close()
    system.close()
    pp.close()


def test_kernel_equals_host_body_over_several_workgroups():
    """cart-pole N = 30: dim = 282 — two workgroups, a ragged last wave."""
    pp, system = rc.seeded_system("cart_pole", rc.BIG_N)
    n, m_e = system.info["n"], system.info["m_e"]
    assert n + m_e == rc.BIG_DIM and rc.BIG_DIM > 256 and rc.BIG_DIM % 64 != 0
    _factor_solve(system, rc.REG, n, m_e)
    _check_bits(system, rc.REG)
    system.close()
    pp.close()


def test_residual_after_a_fused_newton_step_assembles_the_system():
    """slpx_newton_step never stores lhs / rhs: the residual is taken of the system at the resident state, with the
    regularization the policy settled on."""
    pp, system = rc.seeded_system("cart_pole", 6)
    info = system.newton_step(True)
    assert info[0] == 0
    reg = system.regularization()[0]
    r_host, _, _, _ = rc.host_residual(system, reg)
    r, _ = system.residual()
    assert rc.same_bits(r[0], r_host)
    system.close()
    pp.close()


def _refinement_case(system, reg, steps=3):
    n, m_e = system.info["n"], system.info["m_e"]
    _factor_solve(system, reg, n, m_e)
    cp, ri = system.pattern(5)
    lhs, rhs, p0 = system.get("lhs")[0], system.get("rhs")[0], system.get("p")[0]
    Kreg = cases.regularized(cp, ri, lhs, n, reg[0], reg[1])
    p_true = cases.refined_solution(cp, ri, Kreg, rhs, steps=6)
    norms, accepted = system.refine(steps)
    p = system.get("p")[0]
    k = int(accepted[0])
    print(f"norms {norms[0]} accepted {k}")
    assert k >= 1
    assert np.all(np.diff(norms[0, :k + 1]) < 0) and np.all(np.isnan(norms[0, k + 2:]))
    before, after = cases.max_rel(p0, p_true), cases.max_rel(p, p_true)
    eta_dev = rc.eta(cp, ri, Kreg, rhs, p)
    eta_np = rc.eta(cp, ri, Kreg, rhs, rc.numpy_refinement(cp, ri, Kreg, rhs, p0, k))
    print(f"forward error {before:.3e} -> {after:.3e}; eta {rc.eta(cp, ri, Kreg, rhs, p0):.3e} -> device {eta_dev:.3e}, numpy {eta_np:.3e}")
    assert after <= before
    assert eta_dev <= max(2.0 ** -52, 4.0 * eta_np), (eta_dev, eta_np)
    assert rc.same_bits(system.get("rhs")[0], rhs)  # the right-hand side is the original one again
    # the norm reported last is the norm of the p left behind
    assert rc.same_bits(system.residual()[1][0], norms[0, k])


def test_refinement_works_on_the_interior_fixture():
    """The pair is given to slpx_ldlt_factor.  (0, 1e-10) was checked on the host first: the matrix has the inertia
    (34, 32, 0) there by its eigenvalues, but the product's unpivoted elimination meets exactly-zero pivots with
    delta = 0 at this state (host interpreter of the plan: counters 30 / 23 / 13 zero / 17 bad) — so is the fixture's
    own chosen pair (0, 0).  The pair used is the next rung of the fixture's ladder, (1e-4, 1e-10), whose counters are
    (34, 32, 0, 0) on the host interpreter and are asserted here from the device's."""
    pp, system, _ = rc.fixture_system("cart_pole_N6_interior")
    _refinement_case(system, rc.REG)
    system.close()
    pp.close()


def test_refinement_works_over_several_workgroups():
    """cart-pole N = 30 at the seeded state: (0, 1e-10) meets zero pivots as above (host interpreter: 56 zero); the
    pair is (1e-4, 1e-10), counters (154, 128, 0, 0)."""
    pp, system = rc.seeded_system("cart_pole", rc.BIG_N)
    _refinement_case(system, rc.REG)
    system.close()
    pp.close()


def test_refine_one_step_meets_the_harness_rule(orc, fresh):
    """parity.check_newton_step refines once on the HOST (residual in long double, correction on the backend) and
    asserts p1_vs_true <= max(tol_step, po_vs_true); refine(1) is that step done by the product."""
    pp, op = cases.build_pair("cart_pole", 16, sa, orc)
    system = sa.System(pp, batch=1, device=0)
    backend = parity.GpuBackend(system)
    errs = parity.check_newton_step(backend, op, "interior")
    n, me, mi = pp.dims
    x, s, y, z, mu = cases.newton_state("interior", op.get_x(), n, me, mi, op.scaling()[0])
    rhs = backend.rhs(s, y, z, mu)  # (the harness left its correction's right-hand side behind)
    system.solve()
    delta, gamma, _, _ = op.reg()
    cp, ri = system.pattern(5)
    Kreg = cases.regularized(cp, ri, system.get("lhs")[0], n, delta, gamma)
    p_true = cases.refined_solution(cp, ri, Kreg, rhs)
    norms, accepted = system.refine(1)
    p1 = cases.max_rel(system.get("p")[0], p_true)
    print(f"refine(1): norms {norms[0]} accepted {accepted[0]}; p1_vs_true {p1:.3e}, harness {errs['p1_vs_true']:.3e}, "
          f"oracle {errs['po_vs_true']:.3e}")
    assert p1 <= max(1e-8, errs["po_vs_true"])
    system.close()
    pp.close()


def test_dense_dispatch():
    """A small model the reference factors dense (interior_point.hpp:340-352): the same acceptance and monotonicity."""
    sa.lib().slpx_graph_reset()
    p = Problem()
    x, y, w = p.decision_variable(), p.decision_variable(), p.decision_variable()
    p.minimize(x * x + 2 * y * y + 3 * w * w + x * y + 0.3 * y * w)
    p.subject_to(x + 3 * y + 0.7 * w == 4)
    p.subject_to(x * y >= 0.1)
    system = sa.System(p._p, batch=1, device=0)
    assert system.info["ldlt_dense"] != 0
    n, me, mi = system.info["n"], system.info["m_e"], system.info["m_i"]
    system.set_scaling(np.ones(1 + me + mi))
    system.set_state(np.array([1.3, 0.7, -0.4]), np.array([0.9]), np.array([0.3]), np.array([1.7]), np.array([0.1]))
    system.sweep(True)
    system.assemble()
    system.rhs()
    info, reg, _ = system.compute()
    assert info[0] == 0
    system.solve()
    r_host, _, rhs, p0 = rc.host_residual(system, reg[0])
    assert rc.same_bits(system.residual()[0][0], r_host)
    norms, accepted = system.refine(3)
    k = int(accepted[0])
    print(f"dense: reg {reg[0]} norms {norms[0]} accepted {k}")
    # the same rule: every step taken lowered the norm, and the one that ended it (if any) did not
    assert np.all(np.diff(norms[0, :k + 1]) < 0)
    if k < 3 and norms[0, k] != 0.0:
        assert not norms[0, k + 1] < norms[0, k]
    assert rc.same_bits(system.get("rhs")[0], rhs)
    assert rc.same_bits(system.residual()[1][0], norms[0, k])
    system.close()
    p.close()


def _integer_system(batch=1):
    # Integers, and every pivot a power of two in either elimination order of the coupled pair (rows 0 and 2: pivot 2
    # then -2 - 2 = -4, or pivot -2 then 2 + 2 = 4): the factorization and the solve of an integer p are exact, the
    # kernels' multiplication by the pivot's reciprocal included
    K = np.array([[2.0, 0, 2, 0], [0, 4, 0, 0], [2, 0, -2, 0], [0, 0, 0, -8]])
    n, m_e = 2, 2
    cp, ri, val = [0], [], []
    for c in range(4):
        for r in range(c, 4):
            if r == c or K[r, c] != 0.0:
                ri.append(r)
                val.append(K[r, c])
        cp.append(len(ri))
    ls = sa.System.linear_solver(n, m_e, np.array(cp, np.int32), np.array(ri, np.int32), batch=batch)
    return ls, K, np.array(val)


def test_exact_solution_takes_no_step():
    ls, K, val = _integer_system()
    p_exact = np.array([3.0, -2.0, 5.0, 1.0])
    ls.set_matrix(val)
    ls.set_rhs(K @ p_exact)
    stats = ls.factor(0.0, 0.0)
    assert stats[0, 3] == 0
    ls.solve()
    p = ls.get("p")[0]
    assert rc.same_bits(p, p_exact)
    norms, accepted = ls.refine(3)
    assert norms[0, 0] == 0.0 and np.all(np.isnan(norms[0, 1:])) and accepted[0] == 0
    assert rc.same_bits(ls.get("p")[0], p) and rc.same_bits(ls.get("rhs")[0], K @ p_exact)
    ls.close()


def test_refine_before_any_factorization_is_an_error():
    ls, K, val = _integer_system()
    ls.set_matrix(val)
    ls.set_rhs(np.ones(4))
    L = sa.lib()
    out, acc = np.zeros(4), np.zeros(1, dtype=np.int32)
    assert L.slpx_ldlt_refine(ls._h, 1, out.ctypes.data, acc.ctypes.data) == -100
    assert "factor" in L.slpx_last_error().decode()
    assert L.slpx_ldlt_residual(ls._h, None, out.ctypes.data) == -100
    with pytest.raises(sa.SlpxError):
        ls.refine(1)
    ls.factor(0.0, 0.0)  # factors but no solution yet
    with pytest.raises(sa.SlpxError):
        ls.residual()
    ls.solve()
    assert ls.residual()[1][0] >= 0.0
    ls.close()


def test_nan_in_one_right_hand_side_stays_with_its_problem():
    rng = np.random.default_rng(7)
    ls, K, val = _integer_system(batch=3)
    vals = np.stack([val * (1.0 + 0.25 * b) for b in range(3)])
    vals += 1e-3 * rng.standard_normal(vals.shape)  # (no longer exact: something to refine)
    rhs = rng.standard_normal((3, 4))

    def run(rhs_now):
        ls.set_matrix(vals)
        ls.set_rhs(rhs_now)
        ls.factor(0.0, 1e-10)
        ls.solve()
        norms, accepted = ls.refine(2)
        return norms, accepted, ls.get("p"), ls.get("rhs")

    norms0, acc0, p0, _ = run(rhs)
    bad = rhs.copy()
    bad[1, 2] = np.nan
    norms1, acc1, p1, rhs1 = run(bad)
    assert not np.isfinite(norms1[1, 0]) and acc1[1] == 0 and np.all(np.isnan(norms1[1, 1:]))
    for b in (0, 2):
        assert rc.same_bits(norms1[b], norms0[b]) and acc1[b] == acc0[b] and rc.same_bits(p1[b], p0[b])
    assert rc.same_bits(rhs1, bad)
    ls.close()
