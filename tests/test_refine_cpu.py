"""The host side of the residual / refinement path (slpx_ldlt_residual, slpx_ldlt_refine): the exported symbols and
their behaviour without a device, the row map, and the host body of row_residual — the body the kernel runs —
against exact rational arithmetic."""
import math
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import refinecheck

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = ["cart_pole_N8_indefinite", "cart_pole_N6_interior", "flywheel_N5_interior"]


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


def fixture(name):
    fx = dict(np.load(GOLDEN / f"{name}.npz"))
    n, m_e = int(fx["n"]), int(fx["m_e"])
    colptr, rowidx, val = lower_csc(fx["lhs"])
    delta, gamma = (float(v) for v in fx["chosen"])
    return n, m_e, colptr, rowidx, val, fx["rhs"], delta, gamma


def dense_regularized(n, colptr, rowidx, val, delta, gamma):
    dim = len(colptr) - 1
    K = np.zeros((dim, dim))
    for c in range(dim):
        for q in range(colptr[c], colptr[c + 1]):
            K[rowidx[q], c] = K[c, rowidx[q]] = val[q]
    return K + np.diag([delta] * n + [-gamma] * (dim - n))


def test_symbols_are_exported_and_the_abi_version_stays():
    L = sa.lib()
    assert L.slpx_abi_version() == 6
    for name in ("slpx_ldlt_residual", "slpx_ldlt_refine", "slpx_ldlt_residual_masked", "slpx_ldlt_refine_masked"):
        assert hasattr(L, name), name


@pytest.mark.skipif(sa.lib().slpx_device_count() > 0, reason="this machine has a device")
def test_no_device_is_an_error():
    L = sa.lib()
    out = np.zeros(4)
    acc = np.zeros(1, dtype=np.int32)
    assert L.slpx_ldlt_residual(None, out.ctypes.data, out.ctypes.data) == -100
    assert "no HIP device" in L.slpx_last_error().decode()
    assert L.slpx_ldlt_refine(None, 1, out.ctypes.data, acc.ctypes.data) == -100
    assert "no HIP device" in L.slpx_last_error().decode()
    assert L.slpx_ldlt_residual_masked(None, None, None, None) == -100
    assert L.slpx_ldlt_refine_masked(None, 1, None, None, None) == -100


def check_row_map(colptr, rowidx, sanitized=False):
    m = refinecheck.row_map(colptr, rowidx, sanitized=sanitized)
    dim = len(colptr) - 1
    fc, fr = m["colptr"], m["rowidx"]
    nnz = len(fr)
    # the completed pattern: the given entries where user_map says, one diagonal entry per column, rows sorted
    given = [(int(rowidx[q]), c) for c in range(dim) for q in range(colptr[c], colptr[c + 1])]
    full = [(int(fr[q]), c) for c in range(dim) for q in range(fc[c], fc[c + 1])]
    assert [full[k] for k in m["user_map"]] == given
    assert sorted(set(full)) == sorted(set(given) | {(c, c) for c in range(dim)}) and len(set(full)) == nnz
    for c in range(dim):
        assert list(fr[fc[c]:fc[c + 1]]) == sorted(fr[fc[c]:fc[c + 1]])
    # every lower entry once in its row's list, every strictly lower one once more in its column's list
    assert len(m["ent"]) == len(m["col"]) == m["rowptr"][dim] == 2 * nnz - dim
    seen_row, seen_col = np.zeros(nnz, dtype=int), np.zeros(nnz, dtype=int)
    for i in range(dim):
        lst = [(int(m["ent"][q]), int(m["col"][q])) for q in range(m["rowptr"][i], m["rowptr"][i + 1])]
        own = [(e, j) for e, j in lst if j <= i]
        mirrored = [(e, j) for e, j in lst if j > i]
        assert lst == own + mirrored  # the row's own part first
        assert [j for _, j in own] == sorted(j for _, j in own) and [j for _, j in mirrored] == sorted(j for _, j in mirrored)
        for e, j in own:
            assert full[e] == (i, j)
            seen_row[e] += 1
        for e, j in mirrored:
            assert full[e] == (j, i)
            seen_col[e] += 1
    strictly = np.array([r != c for r, c in full])
    assert np.all(seen_row == 1) and np.all(seen_col[strictly] == 1) and np.all(seen_col[~strictly] == 0)
    return m


@pytest.mark.parametrize("name", FIXTURES)
def test_row_map_of_the_golden_patterns(name):
    _, _, colptr, rowidx, _, _, _, _ = fixture(name)
    check_row_map(colptr, rowidx)


def test_row_map_of_a_pattern_with_an_empty_row_and_a_missing_diagonal():
    # 5 x 5: row / column 2 has no off-diagonal entry, column 3 has no diagonal entry
    #   [x . . . .]
    #   [x x . . .]
    #   [. . x . .]
    #   [x . . . .]     <- (3, 3) absent
    #   [. x . x x]
    colptr = [0, 3, 5, 6, 7, 8]
    rowidx = [0, 1, 3, 1, 4, 2, 4, 4]
    m = check_row_map(np.array(colptr), np.array(rowidx))
    assert len(m["rowidx"]) == 9 and m["rowptr"][3] - m["rowptr"][2] == 1  # the diagonal was added; row 2 holds it alone


def exact_residual(n, colptr, rowidx, val, rhs, p, delta, gamma):
    """(r, S) per row in rational arithmetic: r = b - Kreg p and S = |b| + sum |Kreg_ij p_j| (the regularization a
    term of its own)."""
    dim = len(colptr) - 1
    F = Fraction
    r = [F(float(b)) for b in rhs]
    S = [abs(F(float(b))) for b in rhs]
    pf = [F(float(v)) for v in p]
    for c in range(dim):
        for q in range(colptr[c], colptr[c + 1]):
            i, v = int(rowidx[q]), F(float(val[q]))
            r[i] -= v * pf[c]
            S[i] += abs(v * pf[c])
            if i != c:
                r[c] -= v * pf[i]
                S[c] += abs(v * pf[i])
    for i in range(dim):
        reg = F(float(delta)) if i < n else -F(float(gamma))
        r[i] -= reg * pf[i]
        S[i] += abs(reg * pf[i])
    return r, S


def dd_bound(r_exact, S):
    """1/2 ulp of the exact residual rounded to double + 2^-100 of the row's absolute sum: the error of a sum of
    exact products accumulated with its rounding errors (second order in the unit roundoff) and rounded once."""
    return Fraction(math.ulp(float(r_exact))) / 2 + Fraction(1, 2 ** 100) * S


@pytest.mark.parametrize("name", FIXTURES)
def test_host_body_against_exact_arithmetic(name):
    n, m_e, colptr, rowidx, val, rhs, delta, gamma = fixture(name)
    p = np.linalg.solve(dense_regularized(n, colptr, rowidx, val, delta, gamma), rhs)
    r_dd, r_plain = refinecheck.residual(colptr, rowidx, val, rhs, p, n, delta, gamma)
    r_exact, S = exact_residual(n, colptr, rowidx, val, rhs, p, delta, gamma)
    worst_dd = worst_plain = Fraction(0)
    plain_violations = 0
    for i in range(n + m_e):
        bound = dd_bound(r_exact[i], S[i])
        err_dd, err_plain = abs(Fraction(float(r_dd[i])) - r_exact[i]), abs(Fraction(float(r_plain[i])) - r_exact[i])
        worst_dd, worst_plain = max(worst_dd, err_dd / bound), max(worst_plain, err_plain / bound)
        plain_violations += err_plain > bound
        assert err_dd <= bound, (name, i, float(err_dd), float(bound))
    print(f"{name}: worst error / bound: double-double {float(worst_dd):.3g}, plain double {float(worst_plain):.3g} "
          f"({plain_violations} of {n + m_e} rows beyond the bound)")
    if name == "cart_pole_N8_indefinite":
        # the residual of a double solve is all cancellation: the plain sum cannot meet the bound
        assert plain_violations >= 1


def test_sanitized_probe_runs_clean():
    """The probe built with -fsanitize=address,undefined (a stand-alone program), once: the row map of the hand-made
    pattern and the residual of a fixture, same answers as the plain build."""
    n, m_e, colptr, rowidx, val, rhs, delta, gamma = fixture("flywheel_N5_interior")
    p = np.linalg.solve(dense_regularized(n, colptr, rowidx, val, delta, gamma), rhs)
    plain = refinecheck.residual(colptr, rowidx, val, rhs, p, n, delta, gamma)
    san = refinecheck.residual(colptr, rowidx, val, rhs, p, n, delta, gamma, sanitized=True)
    assert np.array_equal(plain[0], san[0]) and np.array_equal(plain[1], san[1])
    check_row_map(np.array([0, 3, 5, 6, 7, 8]), np.array([0, 1, 3, 1, 4, 2, 4, 4]), sanitized=True)
