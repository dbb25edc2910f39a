"""GPU tier: the error bounds of a solve (slpx_ldlt_error_bounds, slpx_ldlt_condest) — berr and norm1 against the
host bodies of kkt_errbound.h bit for bit, the estimates against the exact inverse, ferr against the true error, the
state in memory before and after, batches, masks, a NaN, and the other routes to a factorization.

The constants T and C below are MEASURED, on the host, on the very systems these tests use (tables beside them)."""
import numpy as np
import pytest

import sleipnir_amd as sa
from sleipnir_amd.optimization import Problem
from tests.support import cases
from tests.support import errboundcheck as ebc
from tests.support import refine_cases as rc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# (system, pair): the three fixtures of refine_cases under the pair their own ladder chose — (10, 1e-10) for the
# indefinite one; cart_pole_N6_interior's is (0, 0), where the product's plan has a structurally zero pivot, so it runs
# under the next rung REG as in tests/test_refine_gpu.py — the flywheel also under REG, and cart-pole N = 30 (dim 282:
# two workgroups, the second ragged) under REG.  (The indefinite fixture under REG has the inertia (43, 41): not a
# factorization these tests may use.)
SYSTEMS = [("cart_pole_N8_indefinite", "own"), ("cart_pole_N6_interior", "own"), ("flywheel_N5_interior", "own"),
           ("flywheel_N5_interior", "REG"), ("big", "REG")]

# T: how far above the exact ||Kreg^-1||_1 the device's estimate may lie — the estimator itself never exceeds the norm
# of the operator it is given, which here is the COMPUTED inverse.  Measured: the largest relative 1-norm difference
# between the oracle's LDL^T solve of a unit vector (tests/support/oracle: ldlt_solve, its own regularization) and the
# exact column of the inverse of what it factored, over all unit vectors; the device gets 10 x that, floor 1e-10 (the
# margin parity.py grants the product over the oracle).
#   cart_pole_N8_indefinite (dim 84)  2.443e-08   (the oracle settled on (10, 1e-10))
#   cart_pole_N6_interior   (dim 66)  3.119e-07   ((1e-4, 1e-10))
#   flywheel_N5_interior    (dim 17)  1.899e-16   ((0, 0))
#   big                     (dim 282) 4.196e-08   ((1e-4, 1e-10))
T_MEASURED = {"cart_pole_N8_indefinite": 2.443e-08, "cart_pole_N6_interior": 3.119e-07, "flywheel_N5_interior": 1.899e-16,
              "big": 4.196e-08}
T = {k: max(1e-10, 10.0 * v) for k, v in T_MEASURED.items()}

# C: how far below the exact value the estimator may fall.  Measured: the numpy restatement of Higham's algorithm
# (tests/test_errbound_cpu.py: higham) on the exact inverse of every system above, the signs of the entries with
# |v_i| <= 1e-10 max |v| — numerically zero entries of Kreg^-1 e_j, whose computed sign is noise — taken as +1, as -1,
# and at random (seeded); estimate / exact:
#   system / pair                          as computed   +1       -1       random   products
#   cart_pole_N8_indefinite (10, 1e-10)    1.0000        1.0000   1.0000   1.0000   5
#   cart_pole_N8_indefinite (1e-4, 1e-10)  0.9289        0.9289   0.9289   0.9289   5   (measured on the host only)
#   cart_pole_N6_interior   (1e-4, 1e-10)  1.0000        1.0000   1.0000   1.0000   5
#   flywheel_N5_interior    (0, 0)         1.0000        1.0000   1.0000   1.0000   4
#   flywheel_N5_interior    (1e-4, 1e-10)  1.0000        1.0000   1.0000   1.0000   4
#   big                     (1e-4, 1e-10)  1.0000        1.0000   1.0000   1.0000   5 (7 with -1)
# The same restatement on diag(f) Kreg^-1 with f of a double solve and of a refined one, all four sign
# treatments: estimate / exact between 0.66 and 1.0000, and true error <= estimate in every case, before and after the
# refinement, on these systems and on all fourteen (golden fixture, pair) combinations.
# C = half of the smallest ratio seen.
C_SMALLEST_RATIO = 0.9289
C = 0.5 * C_SMALLEST_RATIO


def exact_inverse(K):
    """The inverse of K to working accuracy whatever the conditioning (kappa <= 2e10 here): numpy's, polished by two
    Newton steps X <- X + X (I - K X) with the residual in extended precision."""
    X = np.linalg.inv(K).astype(np.longdouble)
    Kl = K.astype(np.longdouble)
    eye = np.eye(K.shape[0], dtype=np.longdouble)
    for _ in range(2):
        X = X + X @ (eye - Kl @ X)
    return X


def _factor_solve(system, reg):
    n, m_e = system.info["n"], system.info["m_e"]
    if tuple(reg) == (0.0, 0.0) and system.info["struct_singular"]:
        reg = rc.REG
    stats = system.factor(reg[0], reg[1])
    assert np.all(stats[:, :4] == np.array([n, m_e, 0, 0])), stats
    system.solve()
    return tuple(reg)


def _host(system, reg, b=0):
    """The host bodies on what the device holds for problem b."""
    cp, ri = system.pattern(5)
    return ebc.rows(cp, ri, system.get("lhs")[b], system.get("rhs")[b], system.get("p")[b], system.info["n"], reg[0], reg[1])


def _open(name, pair):
    if name == "big":
        pp, system = rc.seeded_system("cart_pole", rc.BIG_N)
        reg = rc.REG
    else:
        pp, system, chosen = rc.fixture_system(name)
        reg = chosen if pair == "own" else rc.REG
    return pp, system, _factor_solve(system, reg)


_CACHE = {}


def case(name, pair):
    """Everything one (system, pair) is asked about, computed once: the device's numbers before and after refine(2),
    the host bodies' on the same data, the exact inverse and the true solution."""
    if (name, pair) in _CACHE:
        return _CACHE[name, pair]
    pp, system, reg = _open(name, pair)
    n = system.info["n"]
    cp, ri = system.pattern(5)
    c = {"reg": reg, "dim": n + system.info["m_e"]}
    lhs, rhs, p0 = system.get("lhs")[0], system.get("rhs")[0], system.get("p")[0]
    Kreg = cases.regularized(cp, ri, lhs, n, reg[0], reg[1])
    c["K"] = cases.lower_csc_to_dense_sym(cp, ri, Kreg, c["dim"])
    c["Kreg_csc"] = (cp, ri, Kreg)
    c["p_true"] = cases.refined_solution(cp, ri, Kreg, rhs, steps=6)
    c["host0"] = _host(system, reg)
    c["eb0"] = system.error_bounds()
    c["cond"] = system.condest()
    c["berr_only"] = system.error_bounds(forward=False)
    c["state0"] = (rc.same_bits(system.get("p")[0], p0), rc.same_bits(system.get("rhs")[0], rhs), rc.same_bits(system.get("lhs")[0], lhs))
    c["p0"] = p0
    norms, accepted = system.refine(2)
    c["accepted"] = int(accepted[0])
    c["p2"] = system.get("p")[0]
    c["host2"] = _host(system, reg)
    c["eb2"] = system.error_bounds()
    system.close()
    pp.close()
    c["m_max"] = int(c["host0"]["terms"].max())
    c["E"] = float(np.abs(exact_inverse(c["K"])).sum(0).max())
    true = lambda p: float(np.max(np.abs(p - c["p_true"])) / np.max(np.abs(p)))
    c["true0"], c["true2"] = true(p0), true(c["p2"])
    print(f"{name}/{pair} reg {reg}: berr {c['eb0']['berr'][0]:.3e} -> {c['eb2']['berr'][0]:.3e}; ferr {c['eb0']['ferr'][0]:.3e} -> "
          f"{c['eb2']['ferr'][0]:.3e} (true {c['true0']:.3e} -> {c['true2']:.3e}, solves {c['eb0']['solves'][0]}, {c['eb2']['solves'][0]}); "
          f"norm1 {c['cond']['norm1'][0]:.6e} inv_norm1 {c['cond']['inv_norm1'][0]:.6e} (exact {c['E']:.6e}) in {c['cond']['solves'][0]}")
    _CACHE[name, pair] = c
    return c


@pytest.mark.parametrize("name,pair", SYSTEMS)
def test_berr_and_norm1_equal_the_host_bodies(name, pair):
    c = case(name, pair)
    for eb, host in ((c["eb0"], c["host0"]), (c["eb2"], c["host2"])):
        berr, norm1 = ebc.berr_norm1(host)
        assert rc.same_bits(eb["berr"][0], berr), (eb["berr"][0], berr)
        assert rc.same_bits(c["cond"]["norm1"][0], norm1)
    assert rc.same_bits(c["berr_only"]["berr"][0], c["eb0"]["berr"][0])
    assert np.isnan(c["berr_only"]["ferr"][0]) and c["berr_only"]["solves"][0] == 0  # berr alone: no solve
    ref = float(np.abs(c["K"]).sum(0).max())
    assert abs(c["cond"]["norm1"][0] - ref) <= c["m_max"] * U * ref


def test_berr_of_a_refined_solution_is_at_rounding_level():
    """A refined solution is componentwise backward stable to the rounding of its residual: berr <= (m_max + 4) 2u."""
    c = case("cart_pole_N6_interior", "REG")
    assert c["accepted"] >= 1
    assert c["eb2"]["berr"][0] <= (c["m_max"] + 4) * 2 * U, c["eb2"]["berr"][0]
    assert c["eb0"]["berr"][0] > c["eb2"]["berr"][0]


@pytest.mark.parametrize("name,pair", SYSTEMS)
def test_condest_against_the_exact_inverse(name, pair):
    c = case(name, pair)
    est, solves = float(c["cond"]["inv_norm1"][0]), int(c["cond"]["solves"][0])
    assert solves <= 12
    assert est <= c["E"] * (1.0 + T[name]), (est, c["E"])
    assert est >= C * c["E"], (est, c["E"])
    cond1 = float(c["cond"]["cond1"][0])
    assert cond1 == c["cond"]["norm1"][0] * c["cond"]["inv_norm1"][0]
    yard = cases.cond_inf_estimate(*c["Kreg_csc"])  # (an estimate too: the ranges are compared)
    assert C / 2 * yard <= cond1 <= 2 / C * yard, (cond1, yard)


@pytest.mark.parametrize("name,pair", SYSTEMS)
def test_ferr_is_a_bound_and_a_useful_one(name, pair):
    c = case(name, pair)
    for eb, true in ((c["eb0"], c["true0"]), (c["eb2"], c["true2"])):
        assert eb["solves"][0] <= 12
        assert true <= eb["ferr"][0] / C, (true, eb["ferr"][0])
    assert c["eb0"]["ferr"][0] >= c["true0"], (c["eb0"]["ferr"][0], c["true0"])
    assert c["eb2"]["ferr"][0] <= 1e3 * U * c["m_max"], (c["eb2"]["ferr"][0], c["m_max"])


@pytest.mark.parametrize("name,pair", SYSTEMS)
def test_the_state_in_memory_is_untouched(name, pair):
    assert case(name, pair)["state0"] == (True, True, True)


def test_backsub_gives_what_it_would_have_given():
    """p, rhs, and p_s / p_z of a following slpx_step_backsub, with and without the two calls in between."""
    def run(between):
        pp, system, _ = rc.fixture_system("cart_pole_N6_interior")
        _factor_solve(system, rc.REG)
        if between:
            system.error_bounds()
            system.condest()
        system.backsub()
        out = tuple(system.get(k) for k in ("p", "rhs", "p_s", "p_z"))
        system.close()
        pp.close()
        return out

    for a, b in zip(run(False), run(True)):
        assert rc.same_bits(a, b)


# ---- batches: one problem (the fronts), three (the pair lists), 64 (the interleaved kernels) ----------------------

N = 6


def _batch(B, equal=False):
    seeds = [cases.SEED] * B if equal else [cases.SEED + b for b in range(B)]
    pp, system = rc.seeded_system("cart_pole", N, batch=B, seeds=seeds)
    _factor_solve(system, rc.REG)
    return pp, system


@pytest.mark.parametrize("B", [1, 3, 64])
def test_equal_states_give_equal_bits_in_every_slot(B):
    """Within a batch: the slots hold the same values and so, by the batched factorizations' own contract, the same p.
    (Across batch sizes p itself differs — fronts, pair lists and interleaved kernels eliminate in different orders —
    so the numbers of one batch size are not those of another; what is the same at any batch size is the arithmetic
    on a given lhs, rhs, p: test_every_slot_equals_the_host_body_of_its_own_values.)"""
    pp, system = _batch(B, equal=True)
    p = system.get("p")
    eb, ce = system.error_bounds(), system.condest()
    assert np.isfinite(eb["berr"][0]) and np.isfinite(eb["ferr"][0]) and np.isfinite(ce["inv_norm1"][0])
    for b in range(B):
        assert rc.same_bits(p[b], p[0]), b
        for k in ("berr", "ferr", "solves"):
            assert rc.same_bits(np.float64(eb[k][b]), np.float64(eb[k][0])), (k, b)
        for k in ("norm1", "inv_norm1", "solves"):
            assert rc.same_bits(np.float64(ce[k][b]), np.float64(ce[k][0])), (k, b)
    system.close()
    pp.close()


@pytest.mark.parametrize("B", [1, 3, 64])
def test_every_slot_equals_the_host_body_of_its_own_values(B):
    pp, system = _batch(B)
    eb, ce = system.error_bounds(forward=False), system.condest()
    for b in sorted({0, 1 % B, B // 2, B - 1}):
        berr, norm1 = ebc.berr_norm1(_host(system, rc.REG, b))
        assert rc.same_bits(eb["berr"][b], berr) and rc.same_bits(ce["norm1"][b], norm1), (B, b)
    if B > 1:
        assert not rc.same_bits(eb["berr"][0], eb["berr"][1])
    system.close()
    pp.close()


@pytest.mark.parametrize("B", [3, 64])
def test_mask_leaves_the_other_instances_alone(B):
    pp, system = _batch(B)
    p0, rhs0 = system.get("p"), system.get("rhs")
    eb_all, ce_all = system.error_bounds(), system.condest()
    mask = np.zeros(B, dtype=np.uint8)
    mask[[1, B - 1]] = 1
    sent = lambda: (np.full(B, 7.0), np.full(B, 7.0), np.full(B, 7, dtype=np.int32))
    eb = system.error_bounds(mask=mask, out=sent())
    ce = system.condest(mask=mask, out=sent())
    for b in range(B):
        for got, ref, keys in ((eb, eb_all, ("berr", "ferr", "solves")), (ce, ce_all, ("norm1", "inv_norm1", "solves"))):
            for k in keys:
                if mask[b]:
                    assert rc.same_bits(np.float64(got[k][b]), np.float64(ref[k][b])), (k, b)
                else:
                    assert got[k][b] == 7, (k, b)
    assert rc.same_bits(system.get("p"), p0) and rc.same_bits(system.get("rhs"), rhs0)
    system.close()
    pp.close()


@pytest.mark.parametrize("B", [3, 64])
def test_nan_in_one_right_hand_side_stays_with_its_problem(B):
    pp, system = _batch(B)
    rhs = system.get("rhs")
    good = system.error_bounds()
    bad = rhs.copy()
    bad[1, 5] = np.nan
    system.set_rhs(bad)
    system.solve()
    eb = system.error_bounds()
    assert np.isnan(eb["berr"][1]) and np.isnan(eb["ferr"][1])
    for b in range(B):
        if b != 1:
            assert rc.same_bits(eb["berr"][b], good["berr"][b]) and rc.same_bits(eb["ferr"][b], good["ferr"][b]), b
            assert eb["solves"][b] == good["solves"][b]
    assert rc.same_bits(system.get("rhs"), bad)
    system.close()
    pp.close()


# ---- the other routes to a factorization ---------------------------------------------------------------------------

def test_after_a_fused_newton_step_the_system_is_assembled():
    """slpx_newton_step never stores lhs / rhs: the bounds are those of the system at the resident state, with the
    regularization the policy settled on."""
    pp, system = rc.seeded_system("cart_pole", 6)
    assert system.newton_step(True)[0] == 0
    reg = system.regularization()[0]
    p0 = system.get("p")[0]
    eb, ce = system.error_bounds(), system.condest()
    berr, norm1 = ebc.berr_norm1(_host(system, reg))
    assert rc.same_bits(eb["berr"][0], berr) and rc.same_bits(ce["norm1"][0], norm1)
    assert np.isfinite(eb["ferr"][0]) and eb["ferr"][0] > 0.0 and 1 <= eb["solves"][0] <= 12
    assert rc.same_bits(system.get("p")[0], p0)
    system.close()
    pp.close()


def test_dense_dispatch():
    """A small model the reference factors dense (set up as tests/test_refine_gpu.py::test_dense_dispatch does)."""
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
    p0, rhs0 = system.get("p")[0], system.get("rhs")[0]
    eb, ce = system.error_bounds(), system.condest()
    berr, norm1 = ebc.berr_norm1(_host(system, reg[0]))
    assert rc.same_bits(eb["berr"][0], berr) and rc.same_bits(ce["norm1"][0], norm1)
    cp, ri = system.pattern(5)
    K = cases.lower_csc_to_dense_sym(cp, ri, cases.regularized(cp, ri, system.get("lhs")[0], n, reg[0][0], reg[0][1]), n + me)
    E = float(np.abs(exact_inverse(K)).sum(0).max())
    assert C * E <= ce["inv_norm1"][0] <= E * (1.0 + 1e-10), (ce["inv_norm1"][0], E)
    true = float(np.max(np.abs(p0 - np.linalg.solve(K, rhs0))) / np.max(np.abs(p0)))
    assert true <= eb["ferr"][0] / C
    assert rc.same_bits(system.get("p")[0], p0) and rc.same_bits(system.get("rhs")[0], rhs0)
    system.close()
    p.close()


def _diagonal_solver(diag, n, m_e):
    dim = len(diag)
    ls = sa.System.linear_solver(n, m_e, np.arange(dim + 1, dtype=np.int32), np.arange(dim, dtype=np.int32))
    ls.set_matrix(np.asarray(diag, dtype=np.float64))
    return ls


def test_bare_linear_solver_with_exact_numbers():
    diag = np.array([4.0, 2.0, 1.0, -0.5, -8.0])
    ls = _diagonal_solver(diag, 3, 2)
    ls.set_rhs(diag * np.ones(5))
    stats = ls.factor(0.0, 0.0)
    assert tuple(int(v) for v in stats[0, :4]) == (3, 2, 0, 0)
    ls.solve()
    assert rc.same_bits(ls.get("p")[0], np.ones(5))
    ce = ls.condest()
    assert ce["norm1"][0] == 8.0 and ce["inv_norm1"][0] == 2.0 and ce["cond1"][0] == 16.0 and ce["solves"][0] <= 12
    eb = ls.error_bounds()
    assert eb["berr"][0] == 0.0 and eb["ferr"][0] == 0.0
    ls.close()


def test_dimension_one():
    ls = _diagonal_solver([4.0], 1, 0)
    ls.set_rhs(np.array([2.0]))
    ls.factor(0.0, 0.0)
    ls.solve()
    assert ls.get("p")[0][0] == 0.5
    ce = ls.condest()
    assert ce["norm1"][0] == 4.0 and ce["inv_norm1"][0] == 0.25 and ce["solves"][0] == 1
    eb = ls.error_bounds()
    assert eb["berr"][0] == 0.0 and eb["ferr"][0] == 0.0
    ls.close()


def test_before_any_factorization_is_an_error():
    ls = _diagonal_solver([4.0, 2.0, -1.0], 2, 1)
    ls.set_rhs(np.ones(3))
    L = sa.lib()
    out, cnt = np.zeros(1), np.zeros(1, dtype=np.int32)
    assert L.slpx_ldlt_error_bounds(ls._h, None, out.ctypes.data, out.ctypes.data, cnt.ctypes.data) == -100
    assert "factor" in L.slpx_last_error().decode()
    assert L.slpx_ldlt_condest(ls._h, None, out.ctypes.data, out.ctypes.data, cnt.ctypes.data) == -100
    assert "factor" in L.slpx_last_error().decode()
    with pytest.raises(sa.SlpxError):
        ls.error_bounds()
    ls.factor(0.0, 0.0)  # factors but no solution yet
    with pytest.raises(sa.SlpxError):
        ls.condest()
    ls.solve()
    assert ls.error_bounds()["berr"][0] >= 0.0
    ls.close()
