"""Matrices whose regularization ladders END ON DIFFERENT RUNGS, and the plain reference of the ladder — TEST
INFRASTRUCTURE ONLY (numpy alone; no device, no library of the product).

classes(n, m_e, seed): eight symmetric K_c = [[H_c, A^T], [A, -C]] on one lower-triangular CSC pattern (the union over
the classes: a class may hold explicit zeros), C = 1e-2 I, A of full row rank, H0 banded and strictly diagonally
dominant with lambda_min >= 1 (the "banded" family of tests/test_linear_solver_gpu.py).  With C positive definite the
inertia of K + diag(delta, -gamma) is (n, m_e, 0) exactly when H + delta I + A^T (C + gamma I)^-1 A is positive
definite, and has more than m_e negative eigenvalues otherwise: with S = H0 + A^T C^-1 A and lam = lambda_min(S),

    class 0      H0                     accepted without regularization
    class 1..6   H0 - (lam + t) I       accepted at the first rung of the ladder above t
                 t = 3e-5, 7e-5, 7e-4, 3e-2, 0.7, 30
    class 7      H0 with one variable k no row of A touches cut loose (its off-diagonals zero in this class only) and
                 H[k, k] = -1e21: one negative eigenvalue too many at every delta up to the give-up

(two t per decade at the bottom: from an empty memory both meet delta = 1e-4, from the memory of that compute they
meet prev / 2 = 5e-5, which lies between them).  Every value is finite.

expected(K, n, m_e, prev): the policy of the reference's SparseRegularizedLDLT::compute
(util/sparse_regularized_ldlt.hpp:64-152) restated on eigenvalues, for one matrix."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

SHIFTS = (3e-5, 7e-5, 7e-4, 3e-2, 0.7, 30.0)
N_CLASSES = 8
GIVE_UP_CLASS = 7
C22 = 1e-2
CUT_LOOSE = -1e21
MARGIN = 1e-9  # smallest |eigenvalue| of a matrix tried, over its infinity norm (tests/test_reg_models_cpu.py)


@dataclass
class Model:
    n: int
    m_e: int
    K: list            # the eight dense symmetric matrices
    colptr: np.ndarray
    rowidx: np.ndarray
    vals: np.ndarray   # [8][nnz]: K_c on the pattern
    lam: float         # lambda_min(H0 + A^T C^-1 A)
    k: int             # the variable class 7 cuts loose
    H0: np.ndarray
    A: np.ndarray

    @property
    def dim(self):
        return self.n + self.m_e


def _base(rng, n, m_e):
    """H0 and A as _structured_kkt("banded") of tests/test_linear_solver_gpu.py makes them."""
    H = np.zeros((n, n))
    bw = int(rng.integers(2, 9))
    for d in range(1, min(bw, n - 1) + 1):
        v = rng.standard_normal(n - d) * 0.3
        H += np.diag(v, -d) + np.diag(v, d)
    H += np.diag(np.abs(H).sum(axis=1) + 1.0)  # strictly diagonally dominant: lambda_min >= 1 (Gershgorin)
    A = np.zeros((m_e, n))
    centres = np.sort(rng.integers(0, n, size=m_e))
    for r, c0 in enumerate(centres):
        cols = np.unique(np.clip(c0 + rng.integers(-4, 5, size=3), 0, n - 1))
        A[r, cols] = rng.standard_normal(len(cols))
    free = np.ones(n, dtype=bool)
    for r, c0 in enumerate(centres):  # full row rank: every row a pivot column of its own nearby
        c = next(int(k) for k in sorted(range(n), key=lambda k: abs(k - int(c0))) if free[k])
        free[c] = False
        A[r, c] += 2.0 + abs(A[r]).sum()
    return H, A


def dense_pattern(n, m_e):
    """The full lower triangle without the off-diagonals of the (2,2) block, as CSC (colptr, rowidx)."""
    dim = n + m_e
    colptr, rowidx = [0], []
    for c in range(dim):
        rowidx += [r for r in range(c, dim) if r == c or c < n]
        colptr.append(len(rowidx))
    return np.array(colptr, np.int32), np.array(rowidx, np.int32)


def classes(n, m_e, seed, dense=False) -> Model:
    """The eight matrices on their shared pattern (dense: on dense_pattern(n, m_e) instead of the union)."""
    rng = np.random.default_rng(seed)
    H0, A = _base(rng, n, m_e)
    S = H0 + A.T @ A / C22
    lam = float(np.linalg.eigvalsh(S)[0])
    untouched = [k for k in range(n) if not A[:, k].any()]
    if not untouched:
        raise ValueError(f"reg_models.classes({n}, {m_e}, {seed}): every variable is in some row of A")
    k = min(untouched, key=lambda j: abs(j - n // 2))
    Hs = [H0] + [H0 - (lam + t) * np.eye(n) for t in SHIFTS]
    H7 = H0.copy()
    H7[k, :] = 0.0
    H7[:, k] = 0.0
    H7[k, k] = CUT_LOOSE
    Hs.append(H7)
    K = [np.block([[H, A.T], [A, -C22 * np.eye(m_e)]]) for H in Hs]
    assert all(np.isfinite(Kc).all() for Kc in K)
    dim = n + m_e
    if dense:
        colptr, rowidx = dense_pattern(n, m_e)
    else:
        union = np.eye(dim, dtype=bool)
        for Kc in K:
            union |= Kc != 0.0
        cp, ri = [0], []
        for c in range(dim):
            ri += [r for r in range(c, dim) if union[r, c]]
            cp.append(len(ri))
        colptr, rowidx = np.array(cp, np.int32), np.array(ri, np.int32)
    cols = np.repeat(np.arange(dim), np.diff(colptr))
    vals = np.ascontiguousarray(np.stack([Kc[rowidx, cols] for Kc in K]))
    return Model(n, m_e, K, colptr, rowidx, vals, lam, k, H0, A)


def regularized(K, n, delta, gamma):
    """K + diag(delta on the first n, -gamma on the rest)."""
    Kr = np.array(K, dtype=np.float64)
    idx = np.arange(len(Kr))
    Kr[idx, idx] = Kr[idx, idx] + np.r_[np.full(n, float(delta)), np.full(len(Kr) - n, -float(gamma))]
    return Kr


def _blocks(K):
    """Index sets of the connected components of K's graph.  A symmetric matrix is, exactly, the direct sum of these
    blocks, so its spectrum is the union of theirs — taken block by block, eigvalsh's error (a few ulps of the BLOCK's
    norm) cannot carry class 7's 1e21 into the eigenvalues of order one beside it."""
    dim = len(K)
    adj = (K != 0.0) | (K.T != 0.0)
    seen = np.zeros(dim, dtype=bool)
    out = []
    for s in range(dim):
        if seen[s]:
            continue
        comp, frontier = [], [s]
        seen[s] = True
        while frontier:
            v = frontier.pop()
            comp.append(v)
            for w in np.flatnonzero(adj[v] & ~seen):
                seen[w] = True
                frontier.append(int(w))
        out.append(np.array(sorted(comp)))
    return out


def spectrum(K):
    """(eigenvalues, margin): all eigenvalues by eigvalsh, block by block, and the smallest over the blocks of
    min |eigenvalue| / |block|_inf."""
    eig, margin = [], np.inf
    for idx in _blocks(K):
        blk = K[np.ix_(idx, idx)]
        w = np.linalg.eigvalsh(blk)
        eig.append(w)
        margin = min(margin, float(np.abs(w).min() / np.abs(blk).sum(axis=1).max()))
    return np.sort(np.concatenate(eig)), margin


def direct_inertia(K):
    """(positive, negative, zero) eigenvalues of K by one eigvalsh of the whole matrix, and min |eigenvalue|.  Good while
    eps |K| is far below the smallest eigenvalue: the ladders of classes 0 to 6 (delta <= 100), not class 7's."""
    w = np.linalg.eigvalsh(K)
    return (int((w > 0).sum()), int((w < 0).sum()), int((w == 0).sum())), float(np.abs(w).min())


def schur(K, n, delta, gamma):
    """S = H + delta I + A^T (C + gamma I)^-1 A of K + diag(delta, -gamma) = [[H + delta I, A^T], [A, -(C + gamma I)]],
    C diagonal and positive."""
    H, A, C = K[:n, :n], K[n:, :n], -K[n:, n:]
    c = np.diag(C)
    if np.any(C != np.diag(c)) or np.any(c <= 0.0):
        raise ValueError("schur(): the (2,2) block must be minus a positive diagonal")
    idx = np.arange(n)
    S = H + (A.T / (c + gamma)) @ A
    S[idx, idx] = S[idx, idx] + delta
    return S


def inertia(K, n, delta=0.0, gamma=0.0):
    """((positive, negative, zero), margin) of K + diag(delta, -gamma) by eigvalsh — of its Schur complement S on the
    (2,2) block.  By Haynsworth's inertia additivity In(K_reg) = In(-(C + gamma I)) + In(S) = (0, m_e, 0) + In(S), an
    identity, and S is what eigvalsh can resolve on every rung: the eigenvalues of order 1e-2 that -(C + gamma I)
    contributes sit beside delta up to 1e20 in K_reg, where one eigvalsh of the whole matrix returns them with an error
    of eps delta and miscounts from delta = 1e14 on (tests/test_reg_models_cpu.py shows both counts agree below that).
    margin: the smallest |eigenvalue| of S over the norm of its block — how far the count is from turning."""
    m_e = len(K) - n
    w, margin = spectrum(schur(K, n, delta, gamma))
    return (int((w > 0).sum()), m_e + int((w < 0).sum()), int((w == 0).sum())), margin


def expected(K, n, m_e, prev=0.0, gamma_min=1e-10):
    """One compute() of the reference on K from the memory `prev` (the delta of the last compute, 0: none): dict of
    attempts [(delta, gamma), ...], accepted (delta, gamma) or None, info (0, or 1: gave up), memory (delta, gamma)
    afterwards — what hessian_regularization() / constraint_jacobian_regularization() then report — and margins, the
    margin of inertia() at every attempt.

    Inertia alone decides.  That needs two things of K, checked here: no attempt has a zero eigenvalue, and an
    unregularized attempt with the ideal inertia passes the reference's |D| >= 1e-4 test whatever the elimination
    order — K is then quasi-definite, every pivot of every symmetric order is at least min(lambda_min(H),
    lambda_min(C)) in magnitude, and that must be 1e-4 or more."""
    K = np.asarray(K, dtype=np.float64)
    if not np.isfinite(K).all():
        raise ValueError("expected(): a non-finite matrix")
    ideal = (n, m_e, 0)
    attempts, margins = [], []

    def tried(delta, gamma):
        counts, margin = inertia(K, n, delta, gamma)
        attempts.append((float(delta), float(gamma)))
        margins.append(margin)
        return counts

    def result(accepted, info, memory):
        return {"attempts": attempts, "accepted": accepted, "info": info, "memory": memory, "margins": margins}

    if tried(0.0, 0.0) == ideal:  # :74-87
        floor = min(float(np.linalg.eigvalsh(K[:n, :n])[0]), float(np.diag(-K[n:, n:]).min()) if m_e else np.inf)
        if not floor >= 1e-4:
            raise ValueError(f"expected(): the pivots of the unregularized matrix are only known to reach {floor:g}")
        return result((0.0, 0.0), 0, (0.0, 0.0))
    delta = 1e-4 if prev == 0.0 else max(prev / 2.0, float(np.finfo(np.float64).eps))  # :95-98
    gamma = float(gamma_min)                                                             # :102
    while True:
        pos, neg, zero = tried(delta, gamma)
        if (pos, neg, zero) == ideal:  # :111-115
            return result((delta, gamma), 0, (delta, gamma))
        if zero > 0:
            raise ValueError("expected(): a zero eigenvalue — inertia alone does not decide this matrix")
        if neg > m_e:       # :127-130
            delta *= 10.0
        elif pos > n:       # :131-135
            gamma = 1e-10 if gamma == 0.0 else gamma * 10.0
        if delta > 1e20 or gamma > 1e20:  # :145-150
            return result(None, 1, (delta, gamma))


# The shapes the tests run: (n, m_e, dense pattern).  "small": where the conditions of the family were first checked;
# "sparse": two rounds of five tasks at the default task size of a small batch, five rounds of nineteen tasks at the
# interleaved kernels' (asserted where the systems are made); "dense": order 16, the dense kernels.
SEED = 7
SHAPES = {"small": (40, 12, False), "sparse": (120, 40, False), "dense": (11, 5, True)}
_MODELS = {}


def model(shape) -> Model:
    if shape not in _MODELS:
        n, m_e, dense = SHAPES[shape]
        _MODELS[shape] = classes(n, m_e, SEED, dense)
    return _MODELS[shape]


_EXPECTED = {}


def expected_of(shape, c, prev=0.0):
    """expected() of class c of model(shape) from the memory prev, computed once."""
    key = (shape, int(c), float(prev))
    if key not in _EXPECTED:
        m = model(shape)
        _EXPECTED[key] = expected(m.K[int(c)], m.n, m.m_e, prev=float(prev))
    return _EXPECTED[key]


def batch_classes(B, give_up_at=2, seed=0):
    """The class of every instance of a batch.  Small batches: class 7 at `give_up_at`, the others in an order that
    puts accepted instances of different rungs on both sides of it; from B = 16 on: the eight classes dealt round
    robin, then shuffled with a fixed seed."""
    if B < 16:
        others = [3, 0, 5, 1, 6, 2, 4]
        cls = [others[i % len(others)] for i in range(B - 1)]
        cls.insert(give_up_at, GIVE_UP_CLASS)
        return np.array(cls)
    cls = np.arange(B) % N_CLASSES
    np.random.default_rng(seed).shuffle(cls)
    return cls


def right_hand_sides(B, dim, seed):
    return np.random.default_rng(seed).standard_normal((B, dim))
