"""Models and matrices that reach the dense LDLT kernels (csrc/ldlt_dense_kernels.h) at a chosen order — TEST
INFRASTRUCTURE ONLY.

The pivoted kernel is reachable only through a compiled model (the bare slpx_ldlt_* seam never sets dense_pivoted), so:
n decision variables, cost (sum x_i)^2, m_e equalities sum (1 + (i + j) mod 3) x_i = 1.  Its KKT pattern (pattern 5) is
the full lower triangle except the off-diagonals of the (2,2) block, which the reference's rule calls dense at every
order.  Any values can be installed on that pattern with set_lhs / set_rhs; factor(delta, gamma) or compute(), then
solve(), work on them as they are (no set_state in between: the stale flags would have the system rebuilt).

The matrix families below are what the kernels are tested on: all symmetric, the off-diagonals of the (2,2) block zero,
seeds fixed."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from . import model, oracle

# 1025: the smallest order at which one of the kernels' 1024 threads owns two diagonal entries (the second pass of
# every `for (i = tid; i < dim; i += 1024)`); 1100: whole waves in the second pass; 63 / 64 / 65 and 1023 / 1024: either
# side of a wave and of the workgroup; 129: a third wave with one lane
ORDERS = (1, 2, 3, 63, 64, 65, 129, 1023, 1024, 1025, 1100)
EDGE_ORDERS = (3, 65, 1025)  # where the zero-pivot and tiny-pivot families run
_M_E = {3: 2, 63: 2, 129: 2, 1024: 2, 1025: 2}  # the orders with two equality constraints; the others have none


def split(order):
    """(n, m_e) of the model of this order."""
    m_e = _M_E.get(order, 0)
    return order - m_e, m_e


def build(m: "model.Model", n, m_e):
    """The model on backend `m`: an NlpProblem (not solved here — only compiled)."""
    p = model.NlpProblem(m)
    xs = [p.decision_variable(0.0) for _ in range(n)]
    total = xs[0]
    for x in xs[1:]:
        total = total + x
    p.minimize(total * total)
    for j in range(m_e):
        row = float(1 + j % 3) * xs[0]
        for i, x in enumerate(xs[1:], start=1):
            row = row + float(1 + (i + j) % 3) * x
        p.eq(row, 1.0)
    return p


def pattern_size(n, m_e):
    dim = n + m_e
    return dim * (dim + 1) // 2 - m_e * (m_e - 1) // 2


def values(K, pattern):
    """The entries of the symmetric dense matrix K in the order of the lower-triangular CSC `pattern` = (colptr, rowidx)."""
    colptr, rowidx = np.asarray(pattern[0]), np.asarray(pattern[1])
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    return np.ascontiguousarray(np.asarray(K)[rowidx, cols], dtype=np.float64)


def regularized(K, n, delta, gamma):
    """K + diag(delta on the first n, -gamma on the rest), each diagonal entry one addition as the kernels make it."""
    Kr = np.array(K, dtype=np.float64)
    dim = len(Kr)
    idx = np.arange(dim)
    Kr[idx, idx] = Kr[idx, idx] + np.r_[np.full(n, float(delta)), np.full(dim - n, -float(gamma))]
    return Kr


def integer_rhs(order):
    """An integer right-hand side (entries in [-4, 4], none of them all zero)."""
    b = np.random.default_rng([77, order]).integers(-4, 5, size=order).astype(np.float64)
    b[0] = 3.0
    return b


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    m_e: int
    K: np.ndarray      # dense symmetric, unregularized
    delta: float       # what factor() is called with
    gamma: float
    exact: bool        # every product of the factorization and of the solve of an integer rhs is exact: no rounding
                       # differs between a fused and an unfused multiply-add, so p is the oracle's bit for bit

    @property
    def order(self):
        return self.n + self.m_e


def _mirror(M):
    """The symmetric matrix whose lower triangle is M's."""
    L = np.tril(M)
    return L + np.tril(M, -1).T


def _clear_22(K, n):
    """Zero the off-diagonals of the (2,2) block (they are not in the pattern)."""
    dim = len(K)
    if dim - n > 1:
        blk = K[n:, n:]
        K[n:, n:] = np.diag(np.diag(blk))
    return K


def _quasidefinite(rng, n, m_e, shift=1.0):
    # (a negative shift: G G^T of half the rank, so that half of H's eigenvalues are the shift itself but for roundoff)
    G = rng.standard_normal((n, n if shift > 0 else max(1, n // 2)))
    H = G @ G.T / n + shift * np.eye(n)
    A = rng.standard_normal((m_e, n))
    return _mirror(np.block([[H, A.T], [A, np.zeros((m_e, m_e))]]))


FAMILIES = ("quasidefinite", "equal_diagonal", "three_level_diagonal", "zero", "zero_diagonal", "spd_block_then_zero",
            "rank5_integer", "tiny_pivot", "all_nan", "nan_at_k")
EVERY_ORDER_FAMILIES = ("quasidefinite", "equal_diagonal", "three_level_diagonal")
EDGE_FAMILIES = ("zero", "zero_diagonal", "spd_block_then_zero", "rank5_integer", "tiny_pivot")
NAN_FAMILIES = ("all_nan", "nan_at_k")


def defined(name, order):
    """zero_diagonal needs an off-diagonal pair."""
    return not (name == "zero_diagonal" and order < 2)


@functools.lru_cache(maxsize=None)
def case(name, order, variant=0):
    """The matrix of a family at an order (cached: read it, never write to it).
      quasidefinite         H = G G^T / n + I, A standard normal, (2,2) block 0; factored at (0, 1e-10)
      indefinite:<shift>    quasidefinite with H = G G^T / n - shift I (for compute(): the policy has to raise delta)
      equal_diagonal        every diagonal entry 8.0, off-diagonals integers in [-3, 3]: Eigen chooses from the not yet
                            updated diagonal, so every step is a tie over the whole rest and trans is the identity
      three_level_diagonal  the same with the diagonal drawn from {2, 4, 8}: ties inside scattered subsets
      zero                  the zero matrix: success, n_zero = dim, trans the identity
      zero_diagonal         zero but for one off-diagonal pair: fails at k = 0
      spd_block_then_zero   blockdiag(SPD r x r, 0), the SPD block made of 2 x 2 blocks 2^s [[4, 2], [2, 4]]: every
                            multiplier is 1/2, every product exact; exact zero pivots after r
      rank5_integer         G G^T with G an integer dim x 5 matrix: roundoff leaves non-zero pivots after a zero one
      tiny_pivot            quasidefinite with one decoupled diagonal entry 1e-310 (the solve's |d| <= DBL_MIN -> 0)
      all_nan, nan_at_k     quasidefinite with every entry NaN / with only the diagonal entry 0 NaN"""
    n, m_e = split(order)
    dim = order
    rng = np.random.default_rng([(FAMILIES + ("indefinite",)).index(name.split(":")[0]), order, variant])
    delta, gamma, exact = 0.0, 0.0, False
    if name == "quasidefinite":
        K, gamma = _quasidefinite(rng, n, m_e), 1e-10
    elif name.startswith("indefinite:"):
        K, gamma = _quasidefinite(rng, n, m_e, shift=-float(name.split(":")[1])), 1e-10
    elif name in ("equal_diagonal", "three_level_diagonal"):
        K = _mirror(rng.integers(-3, 4, size=(dim, dim)).astype(np.float64))
        diag = np.full(dim, 8.0) if name == "equal_diagonal" else rng.choice([2.0, 4.0, 8.0], size=dim)
        K[np.arange(dim), np.arange(dim)] = diag
        K = _clear_22(K, n)
    elif name == "zero":
        K, exact = np.zeros((dim, dim)), True
    elif name == "zero_diagonal":
        K = np.zeros((dim, dim))
        K[1, 0] = K[0, 1] = 1.0
    elif name == "spd_block_then_zero":
        K, exact = np.zeros((dim, dim)), True
        r = 2 * ((dim + 1) // 4)
        for b in range(r // 2):
            scale = 2.0 ** int(rng.integers(0, 4))
            K[2 * b:2 * b + 2, 2 * b:2 * b + 2] = scale * np.array([[4.0, 2.0], [2.0, 4.0]])
    elif name == "rank5_integer":
        G = rng.integers(-3, 4, size=(dim, 5)).astype(np.float64)
        K = _clear_22(G @ G.T, n)
    elif name == "tiny_pivot":
        K, gamma = _quasidefinite(rng, n, m_e), 1e-10
        j = n // 2
        K[j, :] = 0.0
        K[:, j] = 0.0
        K[j, j] = 1e-310
    elif name == "all_nan":
        K, gamma = np.full((dim, dim), np.nan), 1e-10
        K = _clear_22(K, n)
    elif name == "nan_at_k":
        K, gamma = _quasidefinite(rng, n, m_e), 1e-10
        K[0, 0] = np.nan
    else:
        raise KeyError(name)
    K.setflags(write=False)
    return Case(name, n, m_e, K, delta, gamma, exact)


@functools.lru_cache(maxsize=None)
def dense_pattern(n, m_e):
    """Pattern 5 of the model as it must be: the full lower triangle but the off-diagonals of the (2,2) block."""
    dim = n + m_e
    counts = np.where(np.arange(dim) < n, dim - np.arange(dim), 1)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rowidx = np.concatenate([np.arange(c, dim) if c < n else np.array([c]) for c in range(dim)]).astype(np.int32)
    colptr.setflags(write=False)
    rowidx.setflags(write=False)
    return colptr, rowidx


@functools.lru_cache(maxsize=None)
def oracle_factor(name, order, variant=0):
    """The oracle's dense branch on a case at the case's (delta, gamma), with the solve of integer_rhs(order):
    dict(info, D, trans, inertia, x, n_bad, min_abs) — n_bad and min_abs as the product defines them (n_bad: Eigen's
    info is not Success, or D has a non-finite entry; min_abs: the smallest non-zero finite |D|, inf without one)."""
    c = case(name, order, variant)
    cp, ri = dense_pattern(c.n, c.m_e)
    info, D, trans, inertia, x = oracle.dense_ldlt_factor_once(c.n, c.m_e, cp, ri, values(c.K, (cp, ri)), c.delta, c.gamma,
                                                               rhs=integer_rhs(order))
    ok = np.isfinite(D) & (D != 0.0)
    for a in (D, trans, inertia, x):
        a.setflags(write=False)
    return {"info": int(info), "D": D, "trans": trans, "inertia": tuple(int(v) for v in inertia), "x": x,
            "n_bad": int(info != 0 or not np.all(np.isfinite(D))), "min_abs": float(np.min(np.abs(D[ok]))) if ok.any() else np.inf}


@functools.lru_cache(maxsize=None)
def oracle_compute(name, order, variant=0, gamma_min=1e-10):
    """The oracle's policy loop over its dense solver on a case, with the solve of integer_rhs(order):
    dict(info, x, D, reg = (delta, gamma), factorizations)."""
    c = case(name, order, variant)
    cp, ri = dense_pattern(c.n, c.m_e)
    info, x, D, dg, nf = oracle.dense_ldlt_solve(c.n, c.m_e, cp, ri, values(c.K, (cp, ri)), rhs=integer_rhs(order),
                                                 gamma_min=gamma_min)
    for a in (x, D):
        a.setflags(write=False)
    return {"info": int(info), "x": x, "D": D, "reg": (float(dg[0]), float(dg[1])), "factorizations": int(nf)}


def same_bits(a, b):
    """Equal bit for bit but for the payload of NaNs: NaNs in the same places, everything else identical (+0 / -0 told
    apart)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def backward_error(Kreg, b, p):
    """eta(p) = |b - Kreg p|_inf / (|Kreg|_inf |p|_inf + |b|_inf), the residual accumulated in extended precision
    (parity.residual_longdouble on the lower triangle of Kreg)."""
    from . import parity

    dim = len(b)
    cp, ri = dense_pattern(dim, 0)
    r = parity.residual_longdouble(cp, ri, values(Kreg, (cp, ri)), b, p)
    knorm = float(np.max(np.sum(np.abs(Kreg), axis=1)))
    denom = knorm * float(np.max(np.abs(p))) + float(np.max(np.abs(b)))
    return float(np.max(np.abs(r))) / denom


def solve_bound(eta_reference, dim):
    """What a solve on the same factors may have as backward error: max(4 eta(reference), dim 2^-53).  The factors are
    the same bits; the substitutions differ in the device's fused multiply-adds only — 4 is margin over that."""
    return max(4.0 * eta_reference, dim * 2.0 ** -53)


def eigen_ldlt(K, last_of_equals=False):
    """Eigen::LDLT's unblocked kernel restated in numpy (slow: small orders only), every sum term by term in column
    order: (info, D, trans).  last_of_equals: the wrong tie-break (the LAST index of the largest |diagonal|), what the
    kernel's reduction would compute with `oi > bi` in place of `oi < bi`."""
    A = np.array(K, dtype=np.float64)
    dim = len(A)
    trans = np.arange(dim)
    ret, found_zero = True, False
    for k in range(dim):
        d = np.abs(A[np.arange(k, dim), np.arange(k, dim)])
        big = k
        if not np.isnan(d[0]):
            hits = np.flatnonzero(d == np.nanmax(d))
            big = k + int(hits[-1] if last_of_equals else hits[0])
        trans[k] = big
        if big != k:  # (the trailing part is still symmetric: whole rows and columns can be exchanged)
            A[[k, big], :] = A[[big, k], :]
            A[:, [k, big]] = A[:, [big, k]]
        if k > 0:
            temp = A[np.arange(k), np.arange(k)] * A[k, :k]
            sums = np.zeros(dim - k)
            for c in range(k):
                sums = sums + A[k:, c] * temp[c]
            A[k:, k] = A[k:, k] - sums
        akk = A[k, k]
        valid = abs(akk) > 0.0
        if k == 0 and not valid:
            trans = np.arange(dim)
            ret = bool(np.all(np.tril(A, -1) == 0.0))
            break
        if valid:
            A[k + 1:, k] = A[k + 1:, k] / akk
        else:
            ret = ret and bool(np.all(A[k + 1:, k] == 0.0))
        if found_zero and valid:
            ret = False
        elif not valid:
            found_zero = True
    return (0 if ret else 1), A[np.arange(dim), np.arange(dim)].copy(), trans
