"""High-precision reference of one feasibility-restoration iteration (sleipnir_amd/csrc/restoration.hpp) —
TEST INFRASTRUCTURE ONLY.

Two layers, proved against each other in tests/test_fr_reference_cpu.py so that an error in this file's algebra cannot
hide a kernel's:

  * Layer A, generic and dense (small problems): the UNREDUCED Newton-KKT system of the restoration problem

        min  rho sum(p_e + n_e + p_i + n_i) + 1/2 (x - x_R)^T zeta D_R (x - x_R)
        s.t. c_e(x) - p_e + n_e = 0,   [c_i(x) - p_i + n_i; p_e; n_e; p_i; n_i] >= 0

    in the variables X = [x | p_e | n_e | p_i | n_i] with A_e' = [A_e -I I 0 0], five inequality blocks, and the
    conventions of oracle/ipm.hpp (build_kkt_lhs, build_kkt_rhs, back_substitute, fraction_to_the_boundary_rule):
    lhs = [H' + delta I + A_i'^T Sigma A_i', A_e'^T; A_e', 0], rhs = -[g' - A_e'^T y - A_i'^T t; c_e'],
    t = -Sigma c_i' + mu / s + z, p_y = -w, p_s = c_i' - s + A_i' dX, p_z = mu / s - z - Sigma p_s.  Solved by Gaussian
    elimination in fractions.Fraction (exact) or numpy longdouble; its Schur complement on the extra variables is the
    reduced system.

  * Layer B, row by row and sparse (any size): each eliminated 1x1 / 2x2 block inverted EXACTLY in rational arithmetic
    (the inputs are doubles, so Sigma_0 = 1e21 next to Sigma_3 = 1 loses nothing), then the x-level sums in longdouble
    together with the sum of the absolute values of the terms of every entry: what the componentwise bounds of
    tests/test_restoration_kernels_gpu.py are made of.

Everything is derived from V = [f | c_e | c_i | g | A_e | A_i | H_f | H_c] and the CSC patterns of a system
(`info`, `pattern(k)`: sa.System on the GPU, hostcheck.HostCheck without one)."""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53  # unit roundoff of the kernels' arithmetic
RHO = 1e3       # feasibility_restoration.hpp:391
KAPPA = 1e10    # the z reset of interior_point.hpp:797-801


def ld(v):
    """Fraction (or anything float() takes) -> longdouble, to about 106 bits"""
    if isinstance(v, Fraction):
        hi = float(v)
        return LD(hi) + LD(float(v - Fraction(hi)))
    return LD(v)


@dataclass
class FrProblem:
    """What the restoration kernels read, as doubles: the outer problem's values and derivatives at (x, y, z_0) as triplet
    lists, the restoration iterate and the constants of the phase."""
    n: int
    m_e: int
    m_i: int
    ce: np.ndarray
    ci: np.ndarray
    Ae: list  # (row, col, value)
    Ai: list
    Hc: list  # lower triangle
    f_outer: float
    x: np.ndarray
    xr: np.ndarray
    w: np.ndarray  # zeta D_R
    y: np.ndarray
    s0: np.ndarray
    z0: np.ndarray
    pn: np.ndarray  # [p_e | n_e | p_i | n_i]
    sx: np.ndarray
    zx: np.ndarray
    scales: np.ndarray = None   # [1 | d_ce | d_ci]
    g_outer: np.ndarray = None
    s_outer: np.ndarray = None
    mu_outer: float = 0.0
    soc_ce: np.ndarray = None   # second-order-correction accumulators (soc=True)
    soc_c0: np.ndarray = None
    soc_x: np.ndarray = None
    Hf_slots: np.ndarray = field(default=None)  # positions of H_f inside V

    @property
    def M(self):
        return 2 * self.m_e + 2 * self.m_i


def triplets(colptr, rowidx, values):
    out = []
    for c in range(len(colptr) - 1):
        for q in range(colptr[c], colptr[c + 1]):
            out.append((int(rowidx[q]), c, float(values[q])))
    return out


def problem_from_V(info, pattern, V, state):
    """`state`: dict with x, xr, w, y, s0, z0, pn, sx, zx and optionally scales, g_outer, s_outer, mu_outer"""
    n, me, mi = info["n"], info["m_e"], info["m_i"]
    V = np.asarray(V, dtype=np.float64)
    pats = {k: pattern(k) for k in (1, 2, 4)}
    seg = lambda off, pat: V[off:off + len(pat[1])]
    return FrProblem(
        n=n, m_e=me, m_i=mi, ce=V[1:1 + me].copy(), ci=V[1 + me:1 + me + mi].copy(),
        Ae=triplets(*pats[1], seg(info["off_Ae"], pats[1])), Ai=triplets(*pats[2], seg(info["off_Ai"], pats[2])),
        Hc=triplets(*pats[4], seg(info["off_Hc"], pats[4])), f_outer=float(V[0]),
        Hf_slots=np.arange(info["off_Hf"], info["off_Hc"]),
        **{k: (np.asarray(v, dtype=np.float64).copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()})


# ---------------------------------------------------------------------------------------------------------------------
# States
# ---------------------------------------------------------------------------------------------------------------------
def random_state(start, n, me, mi, seed, stiff=False):
    """The mild state of the tests (seeded): x = start + 1e-2 U(-1, 1); every slack and dual of the five blocks and p, n
    exp(U(-2, 2)); y U(-1, 1); x_R, zeta D_R positive; scales in [0.1, 10].  stiff: a row of every block at s = 1e-10,
    z = 1e11 (Sigma = 1e21) and one more row of block 0 and of the bound rows at Sigma = 1e-21."""
    rng = np.random.default_rng(seed)
    M = 2 * me + 2 * mi
    e = lambda k: np.exp(rng.uniform(-2, 2, k))
    st = dict(x=np.asarray(start) + 1e-2 * rng.uniform(-1, 1, n), s0=e(mi), z0=e(mi), pn=e(M), sx=e(M), zx=e(M),
              y=rng.uniform(-1, 1, me), xr=np.abs(start) + rng.uniform(0.1, 1.0, n), w=e(n),
              scales=np.concatenate([[1.0], rng.uniform(0.1, 10.0, me + mi)]), g_outer=rng.uniform(-1, 1, n), s_outer=e(mi),
              mu_outer=0.1)
    if stiff:
        def hard(s, z, k):
            s[k], z[k] = 1e-10, 1e11

        def soft(s, z, k):
            s[k], z[k] = 1e11, 1e-10

        if mi:
            hard(st["s0"], st["z0"], 0)
            hard(st["sx"], st["zx"], 2 * me + min(1, mi - 1))  # block 3
            hard(st["sx"], st["zx"], 2 * me + mi + mi - 1)     # block 4
            if mi > 1:
                soft(st["s0"], st["z0"], mi - 1)
                soft(st["sx"], st["zx"], 2 * me)               # block 3, row 0 (beside block 0's stiff row)
        if me:
            hard(st["sx"], st["zx"], 0)            # block 1
            hard(st["sx"], st["zx"], me + me - 1)  # block 2
            if me > 1:
                soft(st["sx"], st["zx"], 1)
    return st


# ---------------------------------------------------------------------------------------------------------------------
# Layer A: the unreduced system, dense
# ---------------------------------------------------------------------------------------------------------------------
def _num(exact):
    return (lambda v: Fraction(float(v))) if exact else (lambda v: LD(v))


def _zeros(shape, exact):
    if exact:
        a = np.empty(shape, dtype=object)
        a.fill(Fraction(0))
        return a
    return np.zeros(shape, dtype=LD)


def _vec(values, exact):
    cv = _num(exact)
    out = _zeros(len(values), exact)
    for k, v in enumerate(values):
        out[k] = cv(v)
    return out


def restoration_matrices(P, exact):
    """A_e' (m_e x n'), A_i' ((m_i + M) x n'), H' without regularization, g', c_e', c_i', S', Z' of the restoration
    problem, dense"""
    cv = _num(exact)
    n, me, mi, M = P.n, P.m_e, P.m_i, P.M
    nx = n + M
    Ae = _zeros((me, nx), exact)
    for r, c, v in P.Ae:
        Ae[r, c] += cv(v)
    for j in range(me):
        Ae[j, n + j] = cv(-1.0)
        Ae[j, n + me + j] = cv(1.0)
    Ai = _zeros((mi + M, nx), exact)
    for r, c, v in P.Ai:
        Ai[r, c] += cv(v)
    for r in range(mi):
        Ai[r, n + 2 * me + r] = cv(-1.0)
        Ai[r, n + 2 * me + mi + r] = cv(1.0)
    for e in range(M):
        Ai[mi + e, n + e] = cv(1.0)
    H = _zeros((nx, nx), exact)
    for r, c, v in P.Hc:
        H[r, c] += cv(v)
        if r != c:
            H[c, r] += cv(v)
    for j in range(n):
        H[j, j] += cv(P.w[j])
    X = _vec(np.concatenate([P.x, P.pn]), exact)
    g = _zeros(nx, exact)
    for j in range(n):
        g[j] = cv(P.w[j]) * (cv(P.x[j]) - cv(P.xr[j]))
    for e in range(M):
        g[n + e] = cv(RHO)
    pe, ne, pi, ni = X[n:n + me], X[n + me:n + 2 * me], X[n + 2 * me:n + 2 * me + mi], X[n + 2 * me + mi:]
    ce = _vec(P.ce, exact) - pe + ne
    ci = np.concatenate([_vec(P.ci, exact) - pi + ni, X[n:]]) if mi + M else _zeros(0, exact)
    S = _vec(np.concatenate([P.s0, P.sx]), exact)
    Z = _vec(np.concatenate([P.z0, P.zx]), exact)
    return dict(Ae=Ae, Ai=Ai, H=H, g=g, ce=ce, ci=ci, S=S, Z=Z, X=X)


def unreduced_system(P, mu, delta, exact, soc=False):
    cv = _num(exact)
    R = restoration_matrices(P, exact)
    nx, me = P.n + P.M, P.m_e
    S, Z = R["S"], R["Z"]
    Sigma = Z / S if len(S) else S
    mu_, delta_ = cv(mu), cv(delta)
    if soc:
        cis = _vec(np.concatenate([P.soc_c0, P.soc_x]), exact)
        t = mu_ / S - Sigma * cis if len(S) else S
        ce = _vec(P.soc_ce, exact)
    else:
        cis = R["ci"] - S
        t = -Sigma * R["ci"] + mu_ / S + Z if len(S) else S
        ce = R["ce"]
    K = _zeros((nx + me, nx + me), exact)
    Ai = R["Ai"]
    K[:nx, :nx] = R["H"] + (Ai.T * Sigma).dot(Ai) if len(S) else R["H"]
    for j in range(nx):
        K[j, j] += delta_
    K[nx:, :nx] = R["Ae"]
    K[:nx, nx:] = R["Ae"].T
    y = _vec(P.y, exact)
    rhs = _zeros(nx + me, exact)
    rhs[:nx] = -R["g"] + (R["Ae"].T.dot(y) if me else 0) + (Ai.T.dot(t) if len(S) else 0)
    rhs[nx:] = -ce
    R.update(K=K, rhs=rhs, Sigma=Sigma, cis=cis, mu=mu_, delta=delta_)
    return R


def solve_dense(K, b):
    """Gaussian elimination with partial pivoting on object (Fraction) or longdouble arrays"""
    K, b = K.copy(), b.copy()
    N = len(b)
    for k in range(N):
        piv = max(range(k, N), key=lambda i: abs(K[i, k]))
        if K[piv, k] == 0:
            raise ZeroDivisionError("singular matrix")
        if piv != k:
            K[[k, piv]] = K[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        if k + 1 < N:
            f = K[k + 1:, k] / K[k, k]
            K[k + 1:, k:] = K[k + 1:, k:] - np.multiply.outer(f, K[k, k:])
            b[k + 1:] = b[k + 1:] - f * b[k]
    x = b.copy()
    for k in range(N - 1, -1, -1):
        x[k] = (b[k] - (K[k, k + 1:].dot(x[k + 1:]) if k + 1 < N else 0)) / K[k, k]
    return x


def ftb(x, p, tau):
    """fraction_to_the_boundary_rule.hpp:19-43 (oracle/ipm.hpp)"""
    alpha = 1
    for xi, pi in zip(x, p):
        if alpha * pi < -tau * xi:
            alpha = -tau / pi * xi
    return alpha


def direction_from_solution(R, P, sol, tau):
    """sol = (dX, w) of the unreduced system -> the whole direction, step sizes, D_phi (oracle/ipm.hpp:462-476)"""
    nx = P.n + P.M
    dX, wv = sol[:nx], sol[nx:]
    S, Z = R["S"], R["Z"]
    if len(S):
        ps = R["cis"] + R["Ai"].dot(dX)
        pz = R["mu"] / S - Z - R["Sigma"] * ps
    else:
        ps = pz = S
    tau_ = Fraction(float(tau)) if isinstance(R["mu"], Fraction) else LD(tau)
    D_phi = R["g"].dot(dX) - R["mu"] * sum(p / s for p, s in zip(ps, S))
    return dict(dX=dX, w=wv, ps=ps, pz=pz, alpha_max=ftb(S, ps, tau_), alpha_z=ftb(Z, pz, tau_), D_phi=D_phi)


def ldl_pivots(A):
    """pivots of the LDL^T factorization without pivoting"""
    A = A.copy()
    N = A.shape[0]
    d = []
    for k in range(N):
        d.append(A[k, k])
        if k + 1 < N:
            f = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.multiply.outer(f, A[k, k + 1:])
    return d


def schur_reduced(R, P):
    """the unreduced system with the extra variables eliminated: dense (n + m_e) system in the order [x | w]"""
    n, nx, me = P.n, P.n + P.M, P.m_e
    K, rhs = R["K"], R["rhs"]
    keep = list(range(n)) + list(range(nx, nx + me))
    elim = list(range(n, nx))
    if not elim:
        return K[np.ix_(keep, keep)], rhs[keep]
    KEE = K[np.ix_(elim, elim)]
    KRE = K[np.ix_(keep, elim)]
    cols = np.empty((len(elim), len(keep) + 1), dtype=K.dtype)
    for c in range(len(keep)):
        cols[:, c] = solve_dense(KEE, KRE[c, :].copy())
    cols[:, -1] = solve_dense(KEE, rhs[elim].copy())
    return K[np.ix_(keep, keep)] - KRE.dot(cols[:, :-1]), rhs[keep] - KRE.dot(cols[:, -1])


# ---------------------------------------------------------------------------------------------------------------------
# Layer B: row by row, the eliminated blocks in exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------
F = lambda v: v if isinstance(v, Fraction) else Fraction(float(v))


def _inv2(a, b, c):
    """inverse of [[a, b], [b, c]]"""
    det = a * c - b * b
    return c / det, -b / det, a / det


def rows_exact(P, mu, delta, soc=False):
    """Per equality row j: d1 = Sigma_1 + delta, d2, r_pe, r_ne, c_e' and the sums of |terms| of r_pe, r_ne, c_e'.
    Per inequality row r: the 2x2 block B of (p_i, n_i), its inverse, Sigma_0, r_pi, r_ni, t0 with their sums of |terms|,
    Sigma_eff = Sigma_0 - k^T B^-1 k with k = Sigma_0 [-1, 1], and the multiplier of A_i(r, :) in the reduced right-hand
    side, t0 - k^T B^-1 [r_pi, r_ni].  All Fractions."""
    n, me, mi = P.n, P.m_e, P.m_i
    mu, delta, rho = F(mu), F(delta), F(RHO)
    eq, ineq = [], []
    for j in range(me):
        s1, z1, s2, z2 = F(P.sx[j]), F(P.zx[j]), F(P.sx[me + j]), F(P.zx[me + j])
        pe, ne, y = F(P.pn[j]), F(P.pn[me + j]), F(P.y[j])
        S1, S2 = z1 / s1, z2 / s2
        if soc:
            c1, c2, ce = F(P.soc_x[j]), F(P.soc_x[me + j]), F(P.soc_ce[j])
            t1, t2 = mu / s1 - S1 * c1, mu / s2 - S2 * c2
            a1, a2 = mu / s1 + S1 * abs(c1), mu / s2 + S2 * abs(c2)
            ace = abs(ce)
        else:
            c1, c2, ce = pe - s1, ne - s2, F(P.ce[j]) - pe + ne
            t1, t2 = -S1 * pe + mu / s1 + z1, -S2 * ne + mu / s2 + z2
            a1, a2 = S1 * abs(pe) + mu / s1 + z1, S2 * abs(ne) + mu / s2 + z2
            ace = abs(F(P.ce[j])) + abs(pe) + abs(ne)
        eq.append(dict(S1=S1, S2=S2, d1=S1 + delta, d2=S2 + delta, rpe=-rho - y + t1, rne=-rho + y + t2, ce=ce, c1=c1, c2=c2,
                       a_rpe=rho + abs(y) + a1, a_rne=rho + abs(y) + a2, a_ce=ace, s1=s1, z1=z1, s2=s2, z2=z2))
    for r in range(mi):
        e3, e4 = 2 * me + r, 2 * me + mi + r
        s0, z0, s3, z3, s4, z4 = F(P.s0[r]), F(P.z0[r]), F(P.sx[e3]), F(P.zx[e3]), F(P.sx[e4]), F(P.zx[e4])
        pi, ni = F(P.pn[e3]), F(P.pn[e4])
        S0, S3, S4 = z0 / s0, z3 / s3, z4 / s4
        if soc:
            c0, c3, c4 = F(P.soc_c0[r]), F(P.soc_x[e3]), F(P.soc_x[e4])
            t0, t3, t4 = mu / s0 - S0 * c0, mu / s3 - S3 * c3, mu / s4 - S4 * c4
            a0, a3, a4 = mu / s0 + S0 * abs(c0), mu / s3 + S3 * abs(c3), mu / s4 + S4 * abs(c4)
        else:
            ci = F(P.ci[r]) - pi + ni
            c0, c3, c4 = ci - s0, pi - s3, ni - s4
            t0, t3, t4 = -S0 * ci + mu / s0 + z0, -S3 * pi + mu / s3 + z3, -S4 * ni + mu / s4 + z4
            a0 = S0 * (abs(F(P.ci[r])) + abs(pi) + abs(ni)) + mu / s0 + z0
            a3, a4 = S3 * abs(pi) + mu / s3 + z3, S4 * abs(ni) + mu / s4 + z4
        a, b, c = S0 + S3 + delta, -S0, S0 + S4 + delta
        ia, ib, ic = _inv2(a, b, c)
        rpi, rni = -rho - t0 + t3, -rho + t0 + t4
        u3, u4, au3, au4 = -rho + t3, -rho + t4, rho + a3, rho + a4
        k1, k2 = -S0, S0  # the coupling of (p_i, n_i) to A_i(r, :) dx
        sig_eff = S0 - (k1 * (ia * k1 + ib * k2) + k2 * (ib * k1 + ic * k2))
        mult = t0 - (k1 * (ia * rpi + ib * rni) + k2 * (ib * rpi + ic * rni))
        # the same multiplier with every leaf term taken in absolute value, in the cancelled form (all factors positive):
        # (a3 a4 |t0| + Sigma_0 (a4 |u3| + a3 |u4|)) / det
        A3, A4 = S3 + delta, S4 + delta
        det = a * c - b * b
        a_mult = (A3 * A4 * a0 + S0 * (A4 * au3 + A3 * au4)) / det
        ineq.append(dict(S0=S0, S3=S3, S4=S4, B=(a, b, c), Binv=(ia, ib, ic), det=det, t0=t0, rpi=rpi, rni=rni, u3=u3, u4=u4,
                         a_t0=a0, a_u3=au3, a_u4=au4, c0=c0, c3=c3, c4=c4, sig_eff=sig_eff, mult=mult, a_mult=a_mult,
                         s=(s0, s3, s4), z=(z0, z3, z4), A3=A3, A4=A4))
    return eq, ineq


def reduced_entries(P, mu, delta, soc=False, exact=False, delta_on_x=True):
    """The reduced system on the lower triangle: {(row, col): [value, sum of |terms|, number of terms]} and the right-hand
    side as (values, sums of |terms|, numbers of terms).  exact: Fractions throughout (the proof against Layer A).
    delta_on_x = False: without the + delta of the x diagonal, which the factorization adds itself (restoration.hpp:
    FrDevice::build) as it adds gamma."""
    n, me, mi = P.n, P.m_e, P.m_i
    eq, ineq = rows_exact(P, mu, delta, soc)
    cv = (lambda v: v if isinstance(v, Fraction) else F(v)) if exact else ld
    zero = cv(Fraction(0))
    lhs = {}

    def add(r, c, v, a):
        if r < c:
            r, c = c, r
        e = lhs.setdefault((r, c), [zero, zero, 0])
        e[0] = e[0] + v
        e[1] = e[1] + a
        e[2] += 1

    for r, c, v in P.Hc:
        add(r, c, cv(v), abs(cv(v)))
    for r, c, v in P.Ae:
        add(n + r, c, cv(v), abs(cv(v)))
    rows_of = [[] for _ in range(mi)]
    for r, c, v in P.Ai:
        rows_of[r].append((c, v))
    for r, entries in enumerate(rows_of):
        se = cv(ineq[r]["sig_eff"])
        for c1, v1 in entries:
            for c2, v2 in entries:
                if c1 >= c2:
                    t = cv(v1) * se * cv(v2)
                    add(c1, c2, t, abs(t))
    for j in range(n):
        dj = cv(P.w[j]) + (cv(F(delta)) if delta_on_x else zero)
        add(j, j, dj, dj)
    for j in range(me):
        v = -(1 / eq[j]["d1"] + 1 / eq[j]["d2"])
        lhs[(n + j, n + j)] = [cv(v), cv(-v), 2]
    rhs = [zero] * (n + me)
    arhs = [zero] * (n + me)
    nrhs = [0] * (n + me)
    for j in range(n):
        g = cv(P.w[j]) * (cv(P.x[j]) - cv(P.xr[j]))
        rhs[j] = -g
        arhs[j] = cv(P.w[j]) * (abs(cv(P.x[j])) + abs(cv(P.xr[j])))
        nrhs[j] = 1
    for r, c, v in P.Ae:
        rhs[c] = rhs[c] + cv(v) * cv(P.y[r])
        arhs[c] = arhs[c] + abs(cv(v) * cv(P.y[r]))
        nrhs[c] += 1
    for r, c, v in P.Ai:
        rhs[c] = rhs[c] + cv(v) * cv(ineq[r]["mult"])
        arhs[c] = arhs[c] + abs(cv(v)) * cv(ineq[r]["a_mult"])
        nrhs[c] += 1
    for j in range(me):
        q = eq[j]
        rhs[n + j] = cv(-q["ce"] + q["rpe"] / q["d1"] - q["rne"] / q["d2"])
        arhs[n + j] = cv(q["a_ce"] + q["a_rpe"] / q["d1"] + q["a_rne"] / q["d2"])
        nrhs[n + j] = 3
    return lhs, (rhs, arhs, nrhs)


def reduced_dense(P, mu, delta, soc=False, exact=False):
    """reduced_entries as a dense symmetric matrix and vector (small problems)"""
    lhs, (rhs, _, _) = reduced_entries(P, mu, delta, soc, exact)
    N = P.n + P.m_e
    K = _zeros((N, N), exact)
    for (r, c), e in lhs.items():
        K[r, c] = e[0]
        K[c, r] = e[0]
    b = _zeros(N, exact)
    for k in range(N):
        b[k] = rhs[k]
    return K, b


def expand_exact(P, p, mu, delta, tau, soc=False, exact_sums=False):
    """p = (dx, w) as doubles -> the direction of the eliminated variables and of the five inequality blocks, exactly
    (Fractions), each with the sum of |terms| of its closed form; the step sizes, D_phi and the smallest eliminated pivot.
    dp_e = (r_pe + w) / d1, dn_e = (r_ne - w) / d2, [dp_i; dn_i] = B^-1 [r_pi + Sigma_0 q; r_ni - Sigma_0 q] with
    q = A_i(r, :) dx; p_s = c_i' - s + A_i' dX, p_z = mu / s - z - Sigma p_s (oracle/ipm.hpp: back_substitute).
    D_phi is summed in longdouble from its exact terms (a rational sum of thousands of unrelated denominators takes minutes)
    unless exact_sums asks for the rational one."""
    n, me, mi, M = P.n, P.m_e, P.m_i, P.M
    eq, ineq = rows_exact(P, mu, delta, soc)
    mu_, tau_ = F(mu), F(tau)
    dx = [F(v) for v in p[:n]]
    wv = [F(v) for v in p[n:]]
    dpn, psx, pzx = [None] * M, [None] * M, [None] * M
    a_dpn, a_psx, a_pzx = [None] * M, [None] * M, [None] * M
    ps0, pz0, a_ps0, a_pz0 = [None] * mi, [None] * mi, [None] * mi, [None] * mi
    q_of, aq_of = [Fraction(0)] * mi, [Fraction(0)] * mi
    for r, c, v in P.Ai:
        q_of[r] += F(v) * dx[c]
        aq_of[r] += abs(F(v) * dx[c])
    for j in range(me):
        e = eq[j]
        dpn[j] = (e["rpe"] + wv[j]) / e["d1"]
        dpn[me + j] = (e["rne"] - wv[j]) / e["d2"]
        a_dpn[j] = (e["a_rpe"] + abs(wv[j])) / e["d1"]
        a_dpn[me + j] = (e["a_rne"] + abs(wv[j])) / e["d2"]
        for k, c, s, z, S in ((j, e["c1"], e["s1"], e["z1"], e["S1"]), (me + j, e["c2"], e["s2"], e["z2"], e["S2"])):
            psx[k] = c + dpn[k]
            a_psx[k] = abs(c) + a_dpn[k]
            pzx[k] = mu_ / s - z - S * psx[k]
            a_pzx[k] = mu_ / s + z + S * a_psx[k]
    for r in range(mi):
        f = ineq[r]
        e3, e4 = 2 * me + r, 2 * me + mi + r
        ia, ib, ic = f["Binv"]
        r1, r2 = f["rpi"] + f["S0"] * q_of[r], f["rni"] - f["S0"] * q_of[r]
        dpn[e3], dpn[e4] = ia * r1 + ib * r2, ib * r1 + ic * r2
        # sums of |terms| in the cancelled closed forms (every factor positive):
        #   dp_i = (a4 (u3 - t0 + S0 q) + S0 (u3 + u4)) / det,  dn_i = (a3 (u4 + t0 - S0 q) + S0 (u3 + u4)) / det
        #   p_s0 = c0 + (a3 a4 q + (a3 + a4) t0 - a4 u3 + a3 u4) / det
        S0, A3, A4, det = f["S0"], f["A3"], f["A4"], f["det"]
        a_dpn[e3] = (A4 * (f["a_u3"] + f["a_t0"] + S0 * aq_of[r]) + S0 * (f["a_u3"] + f["a_u4"])) / det
        a_dpn[e4] = (A3 * (f["a_u4"] + f["a_t0"] + S0 * aq_of[r]) + S0 * (f["a_u3"] + f["a_u4"])) / det
        ps0[r] = f["c0"] + q_of[r] - dpn[e3] + dpn[e4]
        a_ps0[r] = abs(f["c0"]) + (A3 * A4 * aq_of[r] + (A3 + A4) * f["a_t0"] + A4 * f["a_u3"] + A3 * f["a_u4"]) / det
        pz0[r] = mu_ / f["s"][0] - f["z"][0] - S0 * ps0[r]
        a_pz0[r] = mu_ / f["s"][0] + f["z"][0] + S0 * a_ps0[r]
        for k, c, s, z, S in ((e3, f["c3"], f["s"][1], f["z"][1], f["S3"]), (e4, f["c4"], f["s"][2], f["z"][2], f["S4"])):
            psx[k] = c + dpn[k]
            a_psx[k] = abs(c) + a_dpn[k]
            pzx[k] = mu_ / s - z - S * psx[k]
            a_pzx[k] = mu_ / s + z + S * a_psx[k]
    # the eliminated pivots in the order p_e, n_e, p_i, n_i: the (p_i, n_i) block of row r is [[a, b], [b, c]] at the
    # positions e3 < e4, nothing else couples them, so its pivots are a and c - b^2 / a
    pivots = [eq[j]["d1"] for j in range(me)] + [eq[j]["d2"] for j in range(me)]
    pivots += [ineq[r]["B"][0] for r in range(mi)]
    pivots += [ineq[r]["B"][2] - ineq[r]["B"][1] ** 2 / ineq[r]["B"][0] for r in range(mi)]
    S = [F(v) for v in np.concatenate([P.s0, P.sx])]
    Z = [F(v) for v in np.concatenate([P.z0, P.zx])]
    PS, PZ = ps0 + psx, pz0 + pzx
    rho = F(RHO)
    d_terms = [F(P.w[j]) * (F(P.x[j]) - F(P.xr[j])) * dx[j] for j in range(n)] + [rho * v for v in dpn] + \
              [-mu_ * a / b for a, b in zip(PS, S)]
    return dict(dpn=dpn, psx=psx, pzx=pzx, ps0=ps0, pz0=pz0, a_dpn=a_dpn, a_psx=a_psx, a_ps0=a_ps0, a_pzx=a_pzx, a_pz0=a_pz0, q=q_of,
                alpha_max=ftb(S, PS, tau_), alpha_z=ftb(Z, PZ, tau_),
                D_phi=sum(d_terms) if exact_sums else sum((ld(t) for t in d_terms), LD(0)),
                a_D_phi=sum(abs(ld(t)) for t in d_terms),
                n_D_phi=len(d_terms), min_pivot=min(pivots) if pivots else None)


# ---------------------------------------------------------------------------------------------------------------------
# Componentwise bounds: |computed - exact| <= gamma(c + terms) * sum |terms|, gamma(k) = k u / (1 - k u), u = 2^-53, with c
# the roundings on the longest path from a leaf (an input double) to the result, counted on the formulas of
# restoration.hpp's header evaluated in the order their parentheses give (a contraction to fma only removes roundings).
# Every Sigma, every a_k = Sigma_k + delta and det = Sigma_0 (a3 + a4) + a3 a4 are sums and products of POSITIVE numbers,
# so their relative errors simply add up: 1 / s (1), Sigma = (1 / s) z (2), a_k (3), a3 + a4 (4), Sigma_0 (a3 + a4) (7),
# a3 a4 (7), det (8).
#   C_LHS  a product term (A_i(r, i) Sigma_eff) A_i(r, j), Sigma_eff = Sigma_0 a3 a4 / det: Sigma_0 a3 (6), times a4 (10),
#          over det (19), times the two entries of A_i (21), one more for the sum it joins per term: 22 + terms.  (The
#          diagonal of an equality row, -(1 / d1 + 1 / d2), needs 6.)
#   C_RHS  a term A_i(r, j) (a3 a4 t0 + Sigma_0 (a4 u3 - a3 u4)) / det: a leaf of t0 = (-(Sigma_0 c_i') + mu / s) + z is
#          Sigma_0 c_i' with c_i' = (c_i - p_i) + n_i (2 + 2 + 1 = 5), two sums later 7; a3 a4 t0 (15); u3 = -rho + t3 (6),
#          a4 u3 (10), the difference (11), times Sigma_0 (14), the sum (16), over det (25), times A_i (26), the g and A_e y
#          terms are shorter: 28 + terms.  An equality row, (-c_e' + r_pe / d1) - r_ne / d2, needs 13.
#   C_EXPAND  dp_i = (a4 ((u3 - t0) + Sigma_0 q) + Sigma_0 (u3 + u4)) / det with q = A_i(r, :) dx of k terms: u3 - t0 (8),
#          Sigma_0 q (k + 4), their sum (9 + k at most), times a4 (13 + k), plus Sigma_0 (u3 + u4) (14 + k), over det
#          (23 + k); p_s0 = c0 + (a3 a4 q + (a3 + a4) t0 - a4 u3 + a3 u4) / det: 25 + k; p_s = c + dp one more, and
#          p_z = (mu / s - z) - Sigma p_s four more ON the sum of |terms| mu / s + z + Sigma sum|terms of p_s|: 32 + k.
# ---------------------------------------------------------------------------------------------------------------------
C_LHS, C_RHS, C_EXPAND = 22, 28, 32


def gamma(k):
    return k * U / (1.0 - k * U)


def min_pivot_ld(P, delta):
    """The smallest pivot of the eliminated block in the order p_e, n_e, p_i, n_i, vectorized in longdouble: d1, d2 of the
    equality rows; a = Sigma_0 + a3 and c - b^2 / a = (Sigma_0 (a3 + a4) + a3 a4) / a of the inequality rows (positive
    terms only; expand_exact has the same number in Fractions, tests/test_fr_reference_cpu.py compares the two)."""
    me, mi = P.m_e, P.m_i
    sx, zx = np.asarray(P.sx, LD), np.asarray(P.zx, LD)
    Sx = zx / sx + LD(delta)
    piv = [Sx[:2 * me]]
    if mi:
        S0 = np.asarray(P.z0, LD) / np.asarray(P.s0, LD)
        a3, a4 = Sx[2 * me:2 * me + mi], Sx[2 * me + mi:]
        piv += [S0 + a3, (S0 * (a3 + a4) + a3 * a4) / (S0 + a3)]
    return np.concatenate(piv).min()


def step_sizes_from_rows(s, ps, z, pz, tau):
    """The kernel's own evaluation of the fraction-to-the-boundary rule on ITS per-row outputs, in double: a min over rows
    is order-free, so the launch's alpha must equal this bit for bit whatever the grid."""
    a, az = 1.0, 1.0
    for si, pi, zi, qi in zip(s, ps, z, pz):
        if pi < 0.0:
            a = min(a, -tau / pi * si)
        if qi < 0.0:
            az = min(az, -tau / qi * zi)
    return a, az


def clamp_z(zn, sn, mu):
    """the z reset of interior_point.hpp:797-801 (oracle/ipm.hpp:632-633), elementwise in double"""
    lo, hi = 1.0 / KAPPA * mu / sn, KAPPA * mu / sn
    return np.where(zn < lo, lo, np.where(zn > hi, hi, zn))


# ---------------------------------------------------------------------------------------------------------------------
# Filter entry and error norms (kkt_error.hpp:92-146, :216-251; filter.hpp:30-60) of the restoration problem, sparse
# ---------------------------------------------------------------------------------------------------------------------
def _sum_with_bound(terms):
    """(sum, bound) of longdouble terms: a double sum of len terms, however ordered and with whatever fma contraction, is
    within (len + 4) 2^-53 sum |terms| of it — len - 1 additions plus the few roundings that made each term."""
    terms = np.asarray(terms, dtype=LD)
    if terms.size == 0:
        return LD(0), 0.0
    return terms.sum(), float((terms.size + 4) * U * np.abs(terms).sum())


def filter_entry(P, pn, S, ce_outer, ci_outer):
    """f, ||c_e'||_1 + ||c_i' - S'||_1, sum ln S' at the restoration point (x, pn) with slacks S = [s_0 | sx] and the outer
    c_e, c_i given: (value, bound) each"""
    n, me, mi = P.n, P.m_e, P.m_i
    x, pn, S = np.asarray(P.x, LD), np.asarray(pn, LD), np.asarray(S, LD)
    pe, ne, pi, ni = pn[:me], pn[me:2 * me], pn[2 * me:2 * me + mi], pn[2 * me + mi:]
    d = x - np.asarray(P.xr, LD)
    f = _sum_with_bound(np.concatenate([LD(0.5) * np.asarray(P.w, LD) * d * d, LD(RHO) * pn]))
    cep = np.asarray(ce_outer, LD) - pe + ne
    cip = np.concatenate([np.asarray(ci_outer, LD) - pi + ni, pn])
    v_terms = np.concatenate([np.abs(cep), np.abs(cip - S)])
    viol, vb = _sum_with_bound(v_terms)
    # every |c - s| term is itself a difference of up to four numbers: their roundings, relative to their magnitudes
    mag = np.concatenate([np.abs(np.asarray(ce_outer, LD)) + pe + ne, np.concatenate([np.abs(np.asarray(ci_outer, LD)) + pi + ni, pn]) + S])
    vb += float(4 * U * mag.sum())
    logs = np.log(S)
    ls, lb = _sum_with_bound(logs)
    lb += float(2 * U * np.abs(logs).sum() + 2 * U * len(S))  # log to an ulp or two, of an argument off by an ulp
    return dict(f=f, viol=(viol, vb), logsum=(ls, lb))


def error_norms(P):
    """Every quantity of FrErrOut at the iterate of P as (value, bound): sums with _sum_with_bound, max / min quantities
    with the bound of the entry that attains them (the few roundings of one entry, or of the column sum it is)."""
    n, me, mi, M = P.n, P.m_e, P.m_i, P.M
    nx = n + M
    x, pn = np.asarray(P.x, LD), np.asarray(P.pn, LD)
    pe, ne, pi, ni = pn[:me], pn[me:2 * me], pn[2 * me:2 * me + mi], pn[2 * me + mi:]
    S = np.concatenate([np.asarray(P.s0, LD), np.asarray(P.sx, LD)])
    Z = np.concatenate([np.asarray(P.z0, LD), np.asarray(P.zx, LD)])
    y = np.asarray(P.y, LD)
    d_ce = np.asarray(P.scales[1:1 + me], LD)
    d_ci = np.concatenate([np.asarray(P.scales[1 + me:], LD), np.ones(M, LD)])
    ce_o, ci_o = np.asarray(P.ce, LD), np.asarray(P.ci, LD)
    cep = ce_o - pe + ne
    cip = np.concatenate([ci_o - pi + ni, pn])
    cep_mag = np.abs(ce_o) + np.abs(pe) + np.abs(ne)
    cip_mag = np.concatenate([np.abs(ci_o) + np.abs(pi) + np.abs(ni), np.abs(pn)])
    # A_e', A_i' of the restoration problem as triplets
    def trip(outer, extra):
        rows = np.array([t[0] for t in outer] + [t[0] for t in extra], dtype=np.int64)
        cols = np.array([t[1] for t in outer] + [t[1] for t in extra], dtype=np.int64)
        vals = np.array([t[2] for t in outer] + [t[2] for t in extra], dtype=LD)
        return rows, cols, vals

    Ae = trip(P.Ae, [(j, n + j, -1.0) for j in range(me)] + [(j, n + me + j, 1.0) for j in range(me)])
    Ai = trip(P.Ai, [(r, n + 2 * me + r, -1.0) for r in range(mi)] + [(r, n + 2 * me + mi + r, 1.0) for r in range(mi)] +
              [(mi + e, n + e, 1.0) for e in range(M)])
    dxr = x - np.asarray(P.xr, LD)
    g = np.concatenate([np.asarray(P.w, LD) * dxr, np.full(M, LD(RHO))])
    dual = g.copy()
    dual_mag = np.abs(g) + np.concatenate([np.asarray(P.w, LD) * np.abs(np.asarray(P.xr, LD)), np.zeros(M, LD)])
    dual_len = np.ones(nx)
    aetce, aetce_mag, aitcp, aitcp_mag = np.zeros(nx, LD), np.zeros(nx, LD), np.zeros(nx, LD), np.zeros(nx, LD)
    cim = np.minimum(cip, 0)
    for (rows, cols, vals), mult, tot, tot_mag, resid, resid_mag in ((Ae, y, aetce, aetce_mag, cep, cep_mag),
                                                                     (Ai, Z, aitcp, aitcp_mag, cim, cip_mag)):
        if len(rows) == 0:
            continue
        np.add.at(dual, cols, -vals * mult[rows])
        np.add.at(dual_mag, cols, np.abs(vals * mult[rows]))
        np.add.at(dual_len, cols, 1.0)
        np.add.at(tot, cols, vals * resid[rows])
        np.add.at(tot_mag, cols, np.abs(vals) * resid_mag[rows])
    # (the un-scaled dual entry is the same number with four more roundings per term: (a / d)(d y))
    dual_bound = float(np.max((dual_len + 8) * U * dual_mag)) if nx else 0.0

    def sq(v, mag, length):
        b = (length + 6) * U * np.asarray(mag, LD)
        tot, tb = _sum_with_bound(v * v)
        return tot, float(tb + np.sum(2 * np.abs(v) * b + b * b))

    col_len = dual_len + 2
    out = {}
    sz = S * Z
    out["dual_inf"] = (np.max(np.abs(dual)) if nx else LD(0), dual_bound)
    out["dual_inf_u"] = out["dual_inf"]
    rel = lambda v, k=4: (v, float(k * U * abs(v)))
    out["sz_max"] = rel(sz.max() if len(sz) else LD(0))
    out["sz_min"] = rel(sz.min() if len(sz) else LD(1e300))
    out["sz_max_u"] = rel(sz.max() if len(sz) else LD(0), 8)
    out["ce_inf"] = (np.max(np.abs(cep)) if me else LD(0), float(3 * U * np.max(cep_mag)) if me else 0.0)
    ceu = cep / d_ce
    out["ce_inf_u"] = (np.max(np.abs(ceu)) if me else LD(0), float(5 * U * np.max(cep_mag / d_ce)) if me else 0.0)
    cis = cip - S
    cis_mag = cip_mag + S
    out["cis_inf"] = (np.max(np.abs(cis)) if len(S) else LD(0), float(4 * U * np.max(cis_mag)) if len(S) else 0.0)
    out["cis_inf_u"] = (np.max(np.abs(cis / d_ci)) if len(S) else LD(0), float(8 * U * np.max(cis_mag / d_ci)) if len(S) else 0.0)
    out["y1"] = _sum_with_bound(np.abs(y))
    out["y1_u"] = _sum_with_bound(np.abs(d_ce * y))
    out["z1"] = _sum_with_bound(np.abs(Z))
    out["z1_u"] = _sum_with_bound(np.abs(d_ci * Z))
    fe = filter_entry(P, P.pn, S, P.ce, P.ci)
    out["f"], out["viol"], out["logsum"] = fe["f"], fe["viol"], fe["logsum"]
    out["aetce_sq"] = sq(aetce, aetce_mag, col_len)
    out["ce_sq"] = sq(cep, cep_mag, np.full(me, 3.0))
    out["aitcp_sq"] = sq(aitcp, aitcp_mag, col_len)
    out["cp_sq"] = sq(cim, cip_mag, np.full(len(cim), 3.0))
    out["x_inf"] = (np.max(np.abs(np.concatenate([x, pn]))), 0.0)
    out["s_inf"] = (np.max(np.abs(S)) if len(S) else LD(0), 0.0)
    out["finite"] = (LD(1), 0.0)
    out["ci_all_pos"] = (LD(1 if np.all(cip > 0) else 0), 0.0)
    # how close the sign decision of ci_all_pos is to a rounding
    out["_ci_margin"] = float(np.min(np.abs(cip) - 4 * U * cip_mag)) if len(cip) else 1.0
    out["f_outer"] = (LD(P.f_outer), 0.0)
    s0 = np.asarray(P.s0, LD)
    vo = np.concatenate([np.abs(ce_o), np.abs(ci_o - s0)])
    viol_o, vob = _sum_with_bound(vo)
    out["viol_outer"] = (viol_o, vob + float(2 * U * (np.abs(ci_o).sum() + s0.sum())))
    lo, lob = _sum_with_bound(np.log(s0))
    out["logsum_outer"] = (lo, lob + float(2 * U * np.abs(np.log(s0)).sum() + 2 * U * mi))
    so = np.asarray(P.s_outer, LD)
    dterms = np.concatenate([np.asarray(P.g_outer, LD) * dxr, -LD(P.mu_outer) * (s0 - so) / so])
    dmag = np.concatenate([np.abs(np.asarray(P.g_outer, LD)) * (np.abs(x) + np.abs(np.asarray(P.xr, LD))), LD(P.mu_outer) * (s0 + so) / so])
    dv, _ = _sum_with_bound(dterms)
    out["dphi_outer"] = (dv, float((len(dterms) + 6) * U * dmag.sum()))
    out["eliminated_min_pivot"] = rel(min_pivot_ld(P, 0.0), 12) if M else (LD(1e300), 0.0)
    return out
