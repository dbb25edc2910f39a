"""The reference of the restoration kernel tests (tests/support/fr_reference.py) against itself: the row-by-row reduced
system and closed-form expansion (what the GPU tier compares the kernels with) equal the direct solve of the UNREDUCED
Newton-KKT system of the restoration problem — exactly, in rational arithmetic, on random small patterns including
m_e = 0 and m_i = 0, at mild and at stiff states; and to 1e-17 in longdouble at mild states.  And the evidence that the
componentwise bounds have teeth: the naive double evaluation of a stiff row violates them."""
from fractions import Fraction

import numpy as np
import pytest

from tests.support import fr_reference as ref

LD = np.longdouble


def synthetic(n, me, mi, seed, stiff=False, soc=False):
    rng = np.random.default_rng(seed)
    dense = lambda rows: [(r, c, float(rng.uniform(-2, 2))) for r in range(rows) for c in range(n) if rng.uniform() < 0.7 or c == r % n]
    Hc = [(r, c, float(rng.uniform(-1, 1))) for c in range(n) for r in range(c, n) if rng.uniform() < 0.6]
    st = ref.random_state(rng.uniform(0.2, 1.0, n), n, me, mi, seed + 1, stiff)
    P = ref.FrProblem(n=n, m_e=me, m_i=mi, ce=rng.uniform(-1, 1, me), ci=rng.uniform(-1, 1, mi), Ae=dense(me), Ai=dense(mi), Hc=Hc,
                      f_outer=0.5, **st)
    if soc:
        P.soc_ce, P.soc_c0, P.soc_x = rng.uniform(-1, 1, me), rng.uniform(-1, 1, mi), rng.uniform(-1, 1, P.M)
    return P


SHAPES = [(3, 1, 2), (4, 2, 3), (3, 0, 2), (4, 2, 0), (2, 1, 1)]


@pytest.mark.parametrize("n,me,mi", SHAPES)
@pytest.mark.parametrize("stiff", [False, True])
@pytest.mark.parametrize("soc", [False, True])
@pytest.mark.parametrize("delta", [0.0, 1e-4])
def test_reduced_and_expanded_equal_the_unreduced_solve_exactly(n, me, mi, stiff, soc, delta):
    P = synthetic(n, me, mi, 7 * n + me + 3 * mi, stiff, soc)
    mu, tau = 0.1, 0.99
    R = ref.unreduced_system(P, mu, delta, exact=True, soc=soc)
    # the reduced system IS the Schur complement
    Ks, bs = ref.schur_reduced(R, P)
    Kr, br = ref.reduced_dense(P, mu, delta, soc, exact=True)
    assert (Ks == Kr).all() and (bs == br).all()
    # reduced solve + closed-form expansion IS the direct solve
    sol = ref.solve_dense(R["K"], R["rhs"])
    D = ref.direction_from_solution(R, P, sol, tau)
    p = ref.solve_dense(Kr, br)
    nx = n + P.M
    assert list(p[:n]) == list(sol[:n]) and list(p[n:]) == list(sol[nx:])
    E = ref.expand_exact(P, list(p), mu, delta, tau, soc, exact_sums=True)
    assert E["dpn"] == list(D["dX"][n:])
    assert E["ps0"] + E["psx"] == list(D["ps"]) and E["pz0"] + E["pzx"] == list(D["pz"])
    assert E["alpha_max"] == D["alpha_max"] and E["alpha_z"] == D["alpha_z"] and E["D_phi"] == D["D_phi"]
    if P.M:
        assert E["min_pivot"] == min(ref.ldl_pivots(R["K"][n:nx, n:nx]))
        assert abs(float(ref.min_pivot_ld(P, delta) / ref.ld(E["min_pivot"])) - 1.0) <= 1e-18
    # the sums of |terms| dominate the values they bound
    for v, a in zip(E["dpn"] + E["psx"] + E["ps0"], E["a_dpn"] + E["a_psx"] + E["a_ps0"]):
        assert abs(v) <= a


@pytest.mark.parametrize("n,me,mi", SHAPES)
def test_longdouble_layers_agree_at_mild_states(n, me, mi):
    P = synthetic(n, me, mi, 11 * n + me + mi)
    mu, delta, tau = 1e-6, 1e-4, 0.99
    R = ref.unreduced_system(P, mu, delta, exact=False)
    sol = ref.solve_dense(R["K"], R["rhs"])
    D = ref.direction_from_solution(R, P, sol, tau)
    Kr, br = ref.reduced_dense(P, mu, delta)
    p = ref.solve_dense(Kr, br)
    nx = n + P.M
    scale = float(np.max(np.abs(sol)))
    got = np.concatenate([p[:n], p[n:]])
    want = np.concatenate([sol[:n], sol[nx:]])
    err = float(np.max(np.abs(got - want))) / scale
    # the expansion from the longdouble p (rounded to double-double accuracy through Fractions of its two halves)
    pf = [Fraction(float(v)) + Fraction(float(v - LD(float(v)))) for v in p]
    E = ref.expand_exact(P, pf, mu, delta, tau)
    e2 = max([abs(float(ref.ld(a) - b)) for a, b in zip(E["dpn"], D["dX"][n:])] + [0.0]) / scale
    e3 = max([abs(float(ref.ld(a) - b)) for a, b in zip(E["ps0"] + E["psx"], D["ps"])] + [0.0]) / max(1.0, float(np.max(np.abs(D["ps"]))) if len(D["ps"]) else 1.0)
    print(f"n={n} m_e={me} m_i={mi}: reduced vs unreduced p {err:.1e}, dpn {e2:.1e}, p_s {e3:.1e}")
    assert err <= 1e-17 * max(1.0, _cond_allowance(R)) and e2 <= 1e-17 * max(1.0, _cond_allowance(R)) and e3 <= 1e-17 * max(1.0, _cond_allowance(R))


def _cond_allowance(R):
    """1e-17 is asked of a well-conditioned solve; a longdouble elimination (unit roundoff 5e-20) of a system of condition
    kappa is only good to about kappa 5e-20: the allowance is kappa / 200, at least 1."""
    K = np.asarray(R["K"], dtype=np.float64)
    return float(np.linalg.cond(K)) / 200.0


def test_naive_double_evaluation_of_a_stiff_row_violates_the_bound():
    """Teeth of the componentwise bound of the GPU tier (fr_reference.C_EXPAND): on the rows with Sigma_0 = 1e21 the textbook
    evaluation in double — solve the 2x2 block by Cramer's rule, then p_s0 = c0 + q - dp_i + dn_i — is outside it, on every
    shape with two or more inequality rows, while the exact values rounded to double are inside."""
    worst = 0.0
    for n, me, mi in [s for s in SHAPES if s[2] >= 2]:  # (one row: no room for the soft row beside the stiff one)
        P = synthetic(n, me, mi, 5 * n + mi, stiff=True)
        mu, delta, tau = 0.1, 0.0, 0.99
        p = np.random.default_rng(3).uniform(-1, 1, n + me)
        E = ref.expand_exact(P, p, mu, delta, tau)
        r = 0  # random_state(stiff): row 0 of block 0 is the stiff one
        k = len([1 for rr, _, _ in P.Ai if rr == r])
        e3, e4 = 2 * me + r, 2 * me + mi + r
        s0, z0, s3, z3, s4, z4 = P.s0[r], P.z0[r], P.sx[e3], P.zx[e3], P.sx[e4], P.zx[e4]
        pi, ni = P.pn[e3], P.pn[e4]
        S0, S3, S4 = z0 / s0, z3 / s3, z4 / s4
        ci = P.ci[r] - pi + ni
        t0, t3, t4 = -S0 * ci + mu / s0 + z0, -S3 * pi + mu / s3 + z3, -S4 * ni + mu / s4 + z4
        q = sum(v * p[c] for rr, c, v in P.Ai if rr == r)
        a, b, c = S0 + S3 + delta, -S0, S0 + S4 + delta
        r1, r2 = (-ref.RHO - t0 + t3) + S0 * q, (-ref.RHO + t0 + t4) - S0 * q
        with np.errstate(all="ignore"):
            det = np.float64(a * c - b * b)
            dpi, dni = (c * r1 - b * r2) / det, (a * r2 - b * r1) / det
        ps0 = (ci - s0) + q - dpi + dni
        for naive, exact, mag in ((dpi, E["dpn"][e3], E["a_dpn"][e3]), (dni, E["dpn"][e4], E["a_dpn"][e4]), (ps0, E["ps0"][r], E["a_ps0"][r])):
            bound = ref.gamma(ref.C_EXPAND + k) * float(mag)
            if np.isfinite(naive):
                worst = max(worst, abs(naive - float(exact)) / bound)
            assert abs(Fraction(float(exact)) - exact) <= bound  # the exact value rounded once is inside
        # (Sigma_0^2 swallows the rest of the determinant: the naive value is far off, or not even finite)
        inside = lambda got, exact, mag: abs(got - float(exact)) <= ref.gamma(ref.C_EXPAND + k) * float(mag)
        with np.errstate(all="ignore"):
            assert not (inside(ps0, E["ps0"][r], E["a_ps0"][r]) and inside(dpi, E["dpn"][e3], E["a_dpn"][e3])), (n, me, mi)
    print(f"naive evaluation: up to {worst:.1e} times the bound where it is finite at all")


@pytest.mark.parametrize("name,dims", [("tiny", (4, 1, 2)), ("ineq_only", (5, 0, 4)), ("eq_only", (6, 3, 0))])
def test_the_small_models_on_the_host_checker(fresh, hostcheck, name, dims):
    """The models of the GPU tier through the host interpretation of their compiled plans: the dimensions the issue sets,
    the two layers of the reference equal in rational arithmetic on the real patterns and values (mild and stiff), and
    the MEASURED tolerance of test_expand_against_the_unreduced_solve: longdouble against plain double numpy on the
    unreduced system, times 8, stays under the floor of 1e-13 (0.9e-16 .. 4.4e-16 when this was written)."""
    from tests.support import fr_models, model

    p, start = fr_models.make(model.Model(model.ProductBackend()), name)
    hc = hostcheck.HostCheck(p.p)
    n, me, mi = hc.info["n"], hc.info["m_e"], hc.info["m_i"]
    assert (n, me, mi) == dims
    for stiff in (False, True):
        st = ref.random_state(start, n, me, mi, 20261019, stiff)
        V = hc.sweep(st["x"], st["y"], st["z0"], True)
        P = ref.problem_from_V(hc.info, hc.pattern, V, st)
        assert len(P.Hc) > 0 and hc.info["off_Hc"] > hc.info["off_Hf"]
        for mu, delta in ((0.1, 0.0), (1e-6, 1e-4)):
            R = ref.unreduced_system(P, mu, delta, exact=True)
            Ks, bs = ref.schur_reduced(R, P)
            Kr, br = ref.reduced_dense(P, mu, delta, exact=True)
            assert (Ks == Kr).all() and (bs == br).all()
            if not stiff:
                Rl = ref.unreduced_system(P, mu, delta, exact=False)
                sol = ref.solve_dense(Rl["K"], Rl["rhs"])
                sol64 = np.linalg.solve(np.asarray(Rl["K"], float), np.asarray(Rl["rhs"], float))
                measured = float(np.max(np.abs(sol - sol64)) / np.max(np.abs(sol)))
                print(f"{name} mu={mu} delta={delta}: longdouble vs double on the unreduced system {measured:.2e}")
                assert 8 * measured <= 1e-13
    hc.close()
    p.p.close()


def test_chain_has_the_hub_and_the_grid_sizes(fresh, hostcheck):
    """chain(300) on the host checker: m_i >= n, the hub's columns of A_e and A_i hold 24 and 25 entries, H_f and H_c
    share entries, and the launch geometry of FrDevice (restated in the GPU tier) reaches 3 and 10 workgroups."""
    from tests.support import fr_models, model

    p, start = fr_models.make(model.Model(model.ProductBackend()), "chain300")
    hc = hostcheck.HostCheck(p.p)
    n, me, mi = hc.info["n"], hc.info["m_e"], hc.info["m_i"]
    assert n == 300 and mi >= n and abs(me - n // 2) <= 2
    assert np.diff(hc.pattern(1)[0])[n - 1] == fr_models.CHAIN_HUB_ROWS and np.diff(hc.pattern(2)[0])[n - 1] == fr_models.CHAIN_HUB_ROWS + 1
    entries = lambda k: {(int(r), c) for c in range(n) for r in hc.pattern(k)[1][hc.pattern(k)[0][c]:hc.pattern(k)[0][c + 1]]}
    assert len(entries(3) & entries(4)) >= n // 2
    assert (max(n, me, mi) + 255) // 256 == 3 and (8 * n + 255) // 256 == 10
    hc.close()
    p.p.close()
