"""The host side of the error bounds of a solve (slpx_ldlt_error_bounds, slpx_ldlt_condest): the exported symbols, the
host bodies of kkt_errbound.h — the bodies the kernel runs — against exact rational arithmetic, and the estimator's
state machine against a numpy restatement of Higham's algorithm."""
import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import errboundcheck as ebc

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = sorted(p.stem for p in GOLDEN.glob("*.npz"))
U = Fraction(1, 2 ** 53)
DBL_MIN = Fraction(sys.float_info.min)
F = Fraction


def lower_csc(dense):
    """Lower triangle of a dense symmetric matrix as CSC with every diagonal entry (pattern 5's convention)."""
    dim = dense.shape[0]
    colptr, rowidx, val = [0], [], []
    for c in range(dim):
        for r in range(c, dim):
            if r == c or dense[r, c] != 0.0:
                rowidx.append(r)
                val.append(dense[r, c])
        colptr.append(len(rowidx))
    return np.array(colptr, dtype=np.int32), np.array(rowidx, dtype=np.int32), np.array(val)


def exact_rows(n, colptr, rowidx, val, rhs, p, delta, gamma):
    """(r, W, terms) per row in rational arithmetic: r = b - Kreg p, W = |b| + sum |Kreg_ij p_j| with the regularization
    a term of its own, terms = the products of the row (the regularization included)."""
    dim = len(colptr) - 1
    r = [F(float(b)) for b in rhs]
    W = [abs(F(float(b))) for b in rhs]
    terms = [1] * dim  # the regularization
    pf = [F(float(v)) for v in p]
    for c in range(dim):
        for q in range(colptr[c], colptr[c + 1]):
            i, v = int(rowidx[q]), F(float(val[q]))
            r[i] -= v * pf[c]
            W[i] += abs(v * pf[c])
            terms[i] += 1
            if i != c:
                r[c] -= v * pf[i]
                W[c] += abs(v * pf[i])
                terms[c] += 1
    for i in range(dim):
        reg = F(float(delta)) if i < n else -F(float(gamma))
        r[i] -= reg * pf[i]
        W[i] += abs(reg * pf[i])
    return r, W, terms


def check_rows(n, colptr, rowidx, val, rhs, p, delta, gamma, underflow=False, sanitized=False):
    """Every row of the system: rho bounds the error of the computed residual and is no looser than allowed; w and t
    against their exact values.  underflow: products of the row leave the normal range, where a rounding is absolute
    (2^-1075) and not relative — rho carries a term for it, the relative bounds on w and t do not apply."""
    got = ebc.rows(colptr, rowidx, val, rhs, p, n, delta, gamma, sanitized=sanitized)
    r_exact, W, terms = exact_rows(n, colptr, rowidx, val, rhs, p, delta, gamma)
    worst = F(0)
    for i in range(len(rhs)):
        m = terms[i]
        assert got["terms"][i] == m
        r_hat, w, t, rho = (F(float(got[k][i])) for k in ("r", "w", "t", "rho"))
        err = abs(r_hat - r_exact[i])
        assert err <= rho, (i, m, float(err), float(rho))
        assert rho <= 4 * U * abs(r_hat) + 4 * (m + 3) ** 2 * U * U * w + m * DBL_MIN, (i, m, float(rho))
        if rho > 0:
            worst = max(worst, err / rho)
        if underflow:
            continue
        assert abs(w - W[i]) <= m * U * W[i], (i, m, float(abs(w - W[i]) / W[i]))
        if W[i] == 0:
            assert got["w"][i] == 0.0 and got["t"][i] == 0.0
        else:
            t_exact = abs(r_hat) / W[i]
            assert abs(t - t_exact) <= (m + 4) * U * t_exact, (i, m, float(t), float(t_exact))
    return got, float(worst)


def arrow(row, p, b_last, rng):
    """A symmetric matrix whose LAST row is `row` (len(row) entries, the diagonal last), unit diagonal elsewhere, and a
    right-hand side whose last entry is b_last: the last row has len(row) + 1 terms, the regularization included."""
    dim = len(row)
    K = np.eye(dim)
    K[dim - 1, :] = row
    K[:, dim - 1] = row
    rhs = rng.standard_normal(dim)
    rhs[dim - 1] = b_last
    return lower_csc(K) + (rhs, np.asarray(p, dtype=np.float64))


def adversarial(kind, m, rng):
    """(colptr, rowidx, val, rhs, p) with a last row of m entries."""
    if kind == "cancellation":
        # b is the rounded value of the very sum it is subtracted from: r is what the roundings left
        row, p = rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4, m), rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4, m)
        return arrow(row, p, float(np.dot(row, p)), rng)
    if kind == "huge_and_tiny":
        row, p = rng.standard_normal(m) * 1e-9, rng.standard_normal(m)
        row[0], p[0] = 3.0e150, 7.0e149
        return arrow(row, p, float(row[0] * p[0]), rng)
    if kind == "alternating":
        # +x, -x pairs of 1e16 around terms of order one
        row, p = np.ones(m), rng.standard_normal(m)
        for k in range(0, m - 1, 2):
            p[k], p[k + 1] = 1e16 + k, -(1e16 + k)
        return arrow(row, p, 0.5, rng)
    raise ValueError(kind)


@pytest.mark.parametrize("m", [1, 2, 64, 257])
@pytest.mark.parametrize("kind", ["cancellation", "huge_and_tiny", "alternating"])
def test_rounding_bound_on_adversarial_rows(kind, m):
    rng = np.random.default_rng(1000 * m + len(kind))
    colptr, rowidx, val, rhs, p = adversarial(kind, m, rng)
    for n_dec in (0, m):  # the long row carries -gamma, then +delta
        _, worst = check_rows(n_dec, colptr, rowidx, val, rhs, p, 1e-4, 1e-10)
        print(f"{kind} m={m} n_dec={n_dec}: worst error / rho {worst:.3g}")


@pytest.mark.parametrize("m", [2, 64])
def test_rounding_bound_where_products_underflow(m):
    """Products in the subnormal range: two_prod's error term is no longer exact there, which is what the m DBL_MIN
    term of rho is for."""
    rng = np.random.default_rng(m)
    row, p = rng.standard_normal(m) * 1e-160, rng.standard_normal(m) * 1e-155
    colptr, rowidx, val, rhs, p = arrow(row, p, 3e-315, rng)
    rhs[:] = 0.0
    rhs[m - 1] = 3e-315
    p[:m - 1] *= 1.0  # (the short rows: 1 * p_i, exact)
    check_rows(0, colptr, rowidx, val, rhs, p, 1e-170, 1e-170, underflow=True)


def fixture(name):
    fx = dict(np.load(GOLDEN / f"{name}.npz"))
    n, m_e = int(fx["n"]), int(fx["m_e"])
    colptr, rowidx, val = lower_csc(fx["lhs"])
    delta, gamma = (float(v) for v in fx["chosen"])
    return n, m_e, colptr, rowidx, val, fx["rhs"], fx["p"], delta, gamma


@pytest.mark.parametrize("name", FIXTURES)
def test_rounding_bound_on_the_golden_systems(name):
    """The rows of the fixtures' lhs / rhs with the fixtures' own p (a solve in double: every r_i is cancellation)."""
    n, m_e, colptr, rowidx, val, rhs, p, delta, gamma = fixture(name)
    got, worst = check_rows(n, colptr, rowidx, val, rhs, p, delta, gamma)
    berr, norm1 = ebc.berr_norm1(got)
    K = np.array(dict(np.load(GOLDEN / f"{name}.npz"))["lhs"]) + np.diag([delta] * n + [-gamma] * m_e)
    m_max = int(got["terms"].max())
    assert abs(norm1 - np.abs(K).sum(0).max()) <= m_max * 2.0 ** -53 * norm1
    print(f"{name}: berr {berr:.3e} norm1 {norm1:.6e} worst error / rho {worst:.3g}")


def test_rows_computed_without_a_rounding_have_no_rounding_bound():
    """Integers: every product and sum of row_residual() is exact, the computed r is r, rho is 0 — and one entry that
    rounds brings the bound back for its rows only."""
    K = np.array([[4.0, 0, 3, 0], [0, 2, 0, 0], [3, 0, -7, 0], [0, 0, 0, -8]])
    colptr, rowidx, val = lower_csc(K)
    p = np.array([3.0, -2.0, 5.0, 1.0])
    got, _ = check_rows(2, colptr, rowidx, val, K @ p, p, 0.0, 0.0)
    assert np.all(got["rho"] == 0.0) and np.all(got["r"] == 0.0) and np.all(got["t"] == 0.0)
    got, _ = check_rows(2, colptr, rowidx, val, K @ p + np.array([1.0, 0, 0, 0]), p, 0.0, 0.0)
    assert np.all(got["rho"] == 0.0) and got["r"][0] == 1.0  # an exact, nonzero residual
    p[2] = 0.1  # rows 0 and 2 now round (3 x 0.1, 7 x 0.1)
    got, _ = check_rows(2, colptr, rowidx, val, K @ p, p, 0.0, 0.0)
    assert got["rho"][0] > 0.0 and got["rho"][2] > 0.0 and got["rho"][1] == 0.0 and got["rho"][3] == 0.0
    check_rows(2, colptr, rowidx, val, K @ p, p, 1e-4, 1e-10)  # (and with a regularization: the bound holds row by row)


def test_zero_row_has_zero_backward_error():
    colptr, rowidx, val = lower_csc(np.diag([2.0, 3.0, -1.0]))
    got = ebc.rows(colptr, rowidx, val, [1.0, 0.0, 2.0], [0.5, 0.0, -2.0], 2, 0.0, 0.0)
    assert got["w"][1] == 0.0 and got["t"][1] == 0.0 and got["r"][1] == 0.0
    assert ebc.berr_norm1(got) == (0.0, 3.0)
    # a NaN is passed on, not taken for a zero
    got = ebc.rows(colptr, rowidx, val, [1.0, np.nan, 2.0], [0.5, 0.0, -2.0], 2, 0.0, 0.0)
    assert np.isnan(got["t"][1]) and np.isnan(ebc.berr_norm1(got)[0])


# ---- the estimator ----------------------------------------------------------------------------------------------

def ordered_sum(v):
    total = 0.0
    for a in np.abs(v):
        total += float(a)
    return total


def higham(A, At):
    """Hager's estimator of ||A||_1 in Higham's form (the algorithm of LAPACK's dlacn2, ITMAX = 5), restated.  Returns
    (estimate, products, probes, smallest |entry| / largest |entry| over every product, the alternating vector won)."""
    n = A.shape[0]
    probes, products, smallest = [], 0, [np.inf]

    def product(M, x, what):
        nonlocal products
        probes.append(what)
        products += 1
        v = M @ x
        smallest[0] = min(smallest[0], float(np.min(np.abs(v)) / np.max(np.abs(v))) if np.max(np.abs(v)) > 0 else 0.0)
        return v

    sign = lambda v: np.where(v >= 0.0, 1.0, -1.0)
    v = product(A, np.full(n, 1.0 / n), (ebc.PROBE_UNIFORM, -1))
    if n == 1:
        return abs(float(v[0])), products, probes, smallest[0], False
    est, xi, j, it = ordered_sum(v), sign(v), -1, 1
    while True:
        z = product(At, xi, (ebc.PROBE_SIGNS, -1))
        j_new = int(np.argmax(np.abs(z)))
        if (it >= 2 and j_new == j) or it >= 5:
            break
        it, j = it + 1, j_new
        e = np.zeros(n)
        e[j] = 1.0
        v = product(A, e, (ebc.PROBE_UNIT, j))
        old, est = est, ordered_sum(v)
        if np.array_equal(sign(v), xi) or est <= old:
            break
        xi = sign(v)
    x = np.array([(-1.0) ** i * (1.0 + i / (n - 1)) for i in range(n)])
    alt = 2.0 * (ordered_sum(product(A, x, (ebc.PROBE_ALTERNATING, -1))) / (3 * n))
    return max(est, alt), products, probes, smallest[0], alt > est


def estimator_inputs():
    out = [("identity", np.eye(7)), ("inverse of diag(3, 1, -2, -0.5)", np.diag([1 / 3, 1.0, -0.5, -2.0])),
           ("dim 1", np.array([[-3.5]])), ("dim 2", np.array([[1.0, -4.0], [-4.0, 2.0]])),
           ("alternating wins", np.array([[-2.0, 0.0, -1.0], [0.0, -2.0, 2.0], [-1.0, 2.0, 0.0]]))]
    for k in range(20):
        rng = np.random.default_rng(4242 + k)
        n = 2 + (k * 2) % 39
        A = rng.standard_normal((n, n))
        out.append((f"seeded {k} dim {n}", A + A.T))
    return out


@pytest.mark.parametrize("name,A", estimator_inputs(), ids=[n for n, _ in estimator_inputs()])
def test_state_machine_equals_the_restatement(name, A):
    dim = A.shape[0]
    est, solves, probes = ebc.norm_estimate(lambda x: A @ x, lambda x: A.T @ x, dim)
    ref_est, ref_products, ref_probes, smallest, alt_won = higham(A, A.T)
    print(f"{name}: estimate {est!r} in {solves} products, ||A||_1 = {np.abs(A).sum(0).max()!r}, alternating won: {alt_won}")
    assert probes == ref_probes
    assert solves == ref_products <= 11
    assert est.hex() == ref_est.hex()
    assert est <= np.abs(A).sum(0).max() * (1.0 + dim * 2.0 ** -53)  # a lower estimate
    if name.startswith("seeded"):
        assert smallest > 0.0  # no sign was a tie: where two correct implementations may part
    if name == "identity":
        assert est == 1.0
    if name.startswith("inverse of diag"):
        assert est == 2.0
    if name == "dim 1":
        assert est == 3.5 and solves == 1
    if name == "alternating wins":
        assert alt_won and probes[-1][0] == ebc.PROBE_ALTERNATING and abs(est - 10.0 / 3.0) < 1e-15


def test_non_finite_product_ends_the_estimate_with_nan():
    A = np.array([[1.0, 2.0], [2.0, np.inf]])
    with np.errstate(invalid="ignore"):
        est, solves, probes = ebc.norm_estimate(lambda x: A @ x, lambda x: A.T @ x, 2)
    assert math.isnan(est) and solves == 1


def test_an_operator_and_its_transpose():
    """A non-symmetric operator, diag(f) S with S symmetric — the shape of the forward error bound: the estimate is of
    ||diag(f) S||_1 = || S diag(f) ||_inf."""
    rng = np.random.default_rng(5)
    S = rng.standard_normal((9, 9))
    S = S + S.T
    f = rng.random(9) * 10.0 ** rng.integers(-8, 0, 9)
    A = np.diag(f) @ S
    est, solves, probes = ebc.norm_estimate(lambda x: f * (S @ x), lambda x: S @ (f * x), 9)
    exact = np.abs(A).sum(0).max()
    print(f"estimate {est:.6e} exact {exact:.6e} in {solves}")
    assert 0.3 * exact <= est <= exact * (1.0 + 9 * 2.0 ** -53)


def test_sanitized_probe_runs_clean():
    """The probe built with -fsanitize=address,undefined (a stand-alone program), once: the rows of a fixture and one
    estimate, same answers as the plain build."""
    n, m_e, colptr, rowidx, val, rhs, p, delta, gamma = fixture("flywheel_N5_interior")
    plain = ebc.rows(colptr, rowidx, val, rhs, p, n, delta, gamma)
    san = ebc.rows(colptr, rowidx, val, rhs, p, n, delta, gamma, sanitized=True)
    for k in plain:
        assert np.array_equal(plain[k], san[k], equal_nan=True), k
    A = estimator_inputs()[-1][1]
    run = lambda s: ebc.norm_estimate(lambda x: A @ x, lambda x: A.T @ x, A.shape[0], sanitized=s)
    assert run(False) == run(True)


def test_symbols_are_exported_and_the_abi_version_stays():
    L = sa.lib()
    assert L.slpx_abi_version() == 6
    for name in ("slpx_ldlt_error_bounds", "slpx_ldlt_condest"):
        assert hasattr(L, name), name
    assert callable(sa.System.error_bounds) and callable(sa.System.condest)


def test_null_system_is_an_error_not_a_crash():
    L = sa.lib()
    out = np.zeros(4)
    cnt = np.zeros(1, dtype=np.int32)
    assert L.slpx_ldlt_error_bounds(None, None, out.ctypes.data, out.ctypes.data, cnt.ctypes.data) == -100
    assert L.slpx_last_error().decode()
    assert L.slpx_ldlt_condest(None, None, None, None, None) == -100
    assert L.slpx_last_error().decode()
