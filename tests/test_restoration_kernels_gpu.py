"""GPU tier: the kernels of feasibility restoration (sleipnir_amd/csrc/restoration.hip) one launch at a time, through the
probe of FrDevice (tests/support/frcheck.cpp), on models whose inequality rows have two or three entries
(tests/support/fr_models.py), against the high-precision reference of tests/support/fr_reference.py — which is proved
against the UNREDUCED Newton-KKT system of the restoration problem in tests/test_fr_reference_cpu.py.

Every launch gets its inputs from the host (`p` is put into the system's solution buffer, never factored here), so a
failure points at one kernel.

Tolerances.
  * Componentwise bounds gamma(c + terms) sum|terms| with the constants C_LHS, C_RHS, C_EXPAND derived in
    fr_reference.py from the operation counts of the formulas of restoration.hpp's header.
  * Sums: (len + 4) 2^-53 sum|terms| (fr_reference._sum_with_bound).
  * MEASURED, against the reference and not against the kernels: the distance between the longdouble solve of the
    unreduced system and the same solve in plain double numpy, at the mild states of tiny / ineq_only / eq_only with the
    host checker's V: 0.9e-16 .. 4.4e-16 relative (condition numbers 43 .. 73).  Times the margin of 8 that is 3.5e-15, below
    the floor of 1e-13 relative, so the floor is what test_expand_against_the_unreduced_solve asks.
"""
import numpy as np
import pytest

from tests.support import fr_models, fr_reference as ref, model

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = ref.U
SMALL = ["tiny", "ineq_only", "eq_only"]
MODELS = SMALL + ["chain300"]
GRIDS = ["chain300", "chain900", "chain2100"]  # the sizes at which the cross-workgroup code changes path
TAU = 0.99
SEED = 20261019


def expand_blocks(n, me, mi):
    """FrDevice::expand: grid_for(max(n, m_e, m_i, 1), 256, 16)"""
    return max(1, min((max(n, me, mi, 1) + 255) // 256, 16))


def errors_blocks(n, me, mi):
    """FrDevice::errors: grid_for(max(8 n, m_e, m_i, 1), 256, 64) — eight lanes per column of x"""
    return max(1, min((max(8 * n, me, mi, 1) + 255) // 256, 64))


class Rig:
    """One compiled model: problem, system, probe; load() puts a state on the device, sweeps, and returns the reference's
    view of what the kernels will read (cached per state: the reference is computed once and shared)."""

    def __init__(self, sa, name):
        from tests.support import frcheck

        self.name = name
        if name.startswith("cart_pole"):  # the benchmark model: simple bounds only, but a cost the tape sums separably
            from tests.support import models

            self.handle = models.cart_pole(int(name[9:]), 5.0 / int(name[9:]))
            self.start = self.handle.get_x()
        else:
            problem, self.start = fr_models.make(model.Model(model.ProductBackend("gpu")), name)
            self.handle = problem.p
        self.system = sa.System(self.handle, batch=1, device=0)
        self.probe = frcheck.FrProbe(self.system)
        self.n, self.me, self.mi, self.M = self.probe.n, self.probe.m_e, self.probe.m_i, self.probe.M
        self.info = self.system.info
        self.lhs_pattern = self.system.pattern(5)
        self._states = {}
        self._problems = {}

    def state(self, stiff):
        if stiff not in self._states:
            self._states[stiff] = ref.random_state(self.start, self.n, self.me, self.mi, SEED, stiff)
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self._states[stiff].items()}

    def load(self, stiff=False, st=None, key=None):
        st = self.state(stiff) if st is None else st
        pr = self.probe
        pr.set_outer(st["x"], st["s0"], st["y"], st["z0"])
        pr.begin(st["xr"], st["w"], st["g_outer"], st["s_outer"], st["mu_outer"], st["pn"], st["sx"], st["zx"], st["scales"])
        pr.sweep_full(True)
        key = stiff if key is None else key
        if key not in self._problems:
            self._problems[key] = ref.problem_from_V(self.info, self.system.pattern, pr.get("V"), st)
        return self._problems[key]

    def close(self):
        self.probe.close()
        self.system.close()
        self.handle.close()


@pytest.fixture(scope="module")
def rigs(slpx):
    slpx.lib().slpx_graph_reset()
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(slpx, name)
        return made[name]

    yield get
    for r in made.values():
        r.close()
    slpx.lib().slpx_graph_reset()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def within(what, got, want, bound):
    """|got - want| <= bound elementwise; the worst ratio is printed before it is asserted"""
    got, want, bound = np.asarray(got, LD), np.asarray(want, LD), np.asarray(bound, LD)
    if got.size == 0:
        return
    err = np.abs(got - want)
    ratio = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1e-300)))
    k = int(np.argmax(ratio))
    print(f"  {what}: worst |got - ref| / bound = {float(ratio.flat[k]):.3g} at {k} (got {float(got.flat[k])!r}, ref {float(want.flat[k])!r}, "
          f"bound {float(bound.flat[k]):.3g})")
    assert np.all(np.isfinite(np.asarray(got, float))), what
    assert np.all(err <= bound), what


def fr_list(values):
    return np.array([ref.ld(v) for v in values], dtype=LD)


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_sizes_the_models_are_meant_to_reach(rigs):
    """chain(300): expand on 2 or more workgroups, errors on 10; chain(900): errors on 26 or more (the unrolled four-load
    fold); chain(2100): errors at the cap of 64, expand at its cap of 16.  The small models: one workgroup each."""
    seen = {}
    for name in SMALL + GRIDS:
        r = rigs(name)
        seen[name] = (expand_blocks(r.n, r.me, r.mi), errors_blocks(r.n, r.me, r.mi))
        print(f"{name}: n={r.n} m_e={r.me} m_i={r.mi}: expand on {seen[name][0]} workgroups, errors on {seen[name][1]}")
    assert rigs("tiny").n == 4 and rigs("tiny").me == 1 and rigs("tiny").mi == 2
    assert (rigs("ineq_only").n, rigs("ineq_only").me, rigs("ineq_only").mi) == (5, 0, 4)
    assert (rigs("eq_only").n, rigs("eq_only").me, rigs("eq_only").mi) == (6, 3, 0)
    for name in SMALL:
        assert seen[name] == (1, 1)
    assert seen["chain300"][0] >= 2 and seen["chain300"][1] == 10
    assert 26 <= seen["chain900"][1] < 64 and seen["chain900"][1] == 29
    assert seen["chain2100"] == (16, 64) and 8 * 2100 > 64 * 256  # (the grid-stride path: more columns than lanes)
    for name in GRIDS:
        r = rigs(name)
        assert r.mi >= r.n
        ae, ai = r.system.pattern(1)[0], r.system.pattern(2)[0]
        assert np.diff(ae).max() >= 20 and np.diff(ai).max() >= 20  # the hub's columns


# ---------------------------------------------------------------------------------------------------------------------
# build
# ---------------------------------------------------------------------------------------------------------------------
def lhs_reference(r, P, mu, delta, soc=False):
    lhs, (rhs, arhs, nrhs) = ref.reduced_entries(P, mu, delta, soc, delta_on_x=False)
    colptr, rowidx = r.lhs_pattern
    want, bound = np.zeros(len(rowidx), LD), np.zeros(len(rowidx))
    used = 0
    for c in range(len(colptr) - 1):
        for k in range(colptr[c], colptr[c + 1]):
            e = lhs.get((int(rowidx[k]), c))
            if e is not None:
                used += 1
                want[k] = e[0]
                bound[k] = ref.gamma(ref.C_LHS + e[2]) * float(e[1])
    assert used == len(lhs)  # every entry of the reference has its place in the pattern
    rb = np.array([ref.gamma(ref.C_RHS + k) * float(a) for a, k in zip(arhs, nrhs)])
    return want, bound, np.array(rhs, dtype=LD), rb


@pytest.mark.parametrize("mu,delta", [(0.1, 0.0), (1e-6, 1e-4)])
@pytest.mark.parametrize("stiff", [False, True])
@pytest.mark.parametrize("name", MODELS)
def test_build_is_the_schur_complement(rigs, name, stiff, mu, delta):
    """Every lhs entry and rhs row of fr_build_kernel against the Schur complement of the unreduced system, componentwise:
    |got - ref| <= gamma(C_LHS + terms) sum|terms of the entry| (rhs: C_RHS) — fr_reference.py has the derivation, 22 and
    28 roundings on the longest path of a product term.  The diagonal of an equality row is -(1/(Sigma_1 + delta) +
    1/(Sigma_2 + delta)) and the x diagonal carries zeta D_R: both are entries of the reference.  H_f is in no entry (the
    bits do not move when V[off_Hf:off_Hc] is overwritten); rhs_only leaves the lhs alone."""
    r = rigs(name)
    P = r.load(stiff)
    pr = r.probe
    pr.put("lhs_raw", np.full(pr.nnz_lhs, np.nan))
    pr.put("rhs_raw", np.full(pr.dim, np.nan))
    pr.build(delta, mu)
    lhs, rhs = pr.get("lhs_raw"), pr.get("rhs_raw")
    want, bound, rwant, rbound = lhs_reference(r, P, mu, delta)
    print(f"{name} stiff={stiff} mu={mu} delta={delta}: {pr.nnz_lhs} entries, up to {max(1, int(np.max(np.diff(r.lhs_pattern[0]))))} per column")
    within("lhs", lhs, want, bound)
    within("rhs", rhs, rwant, rbound)
    # the cost's Hessian is not part of the restoration problem
    V = pr.get("V")
    V2 = V.copy()
    V2[r.info["off_Hf"]:r.info["off_Hc"]] = 1e6 * (1.0 + np.arange(r.info["off_Hc"] - r.info["off_Hf"]))
    assert r.info["off_Hc"] > r.info["off_Hf"]
    pr.put("V", V2)
    pr.build(delta, mu)
    assert same_bits(pr.get("lhs_raw"), lhs) and same_bits(pr.get("rhs_raw"), rhs)
    pr.put("V", V)
    # rhs_only
    sentinel = 12345.678 + np.arange(pr.nnz_lhs)
    pr.put("lhs_raw", sentinel)
    pr.put("rhs_raw", np.full(pr.dim, np.nan))
    pr.build(delta, mu, soc=False, rhs_only=True)
    assert same_bits(pr.get("lhs_raw"), sentinel) and same_bits(pr.get("rhs_raw"), rhs)


@pytest.mark.parametrize("name", MODELS)
def test_second_system_and_pair_have_the_same_bits(rigs, name):
    """build(second) writes what build writes, into the object's own arrays; build_pair(d0, d1) is build(d0) plus
    build(d1, second), bit for bit."""
    r = rigs(name)
    r.load(True)
    pr = r.probe
    mu, d0, d1 = 0.1, 1e-4, 4e-4
    out = {}
    for d in (d0, d1):
        pr.build(d, mu)
        out[d] = (pr.get("lhs_raw"), pr.get("rhs_raw"))
        pr.put("lhs_raw", np.full(pr.nnz_lhs, np.nan))
        pr.build(d, mu, second=True)
        assert same_bits(pr.get("second_lhs"), out[d][0]) and same_bits(pr.get("second_rhs"), out[d][1])
        assert np.all(np.isnan(pr.get("lhs_raw")))  # ... and not into the system's
    assert not same_bits(out[d0][0], out[d1][0]) or r.mi == 0 and r.me == 0
    pr.put("second_lhs", np.full(pr.nnz_lhs, np.nan))
    pr.put("second_rhs", np.full(pr.dim, np.nan))
    pr.build_pair(d0, d1, mu)
    assert same_bits(pr.get("lhs_raw"), out[d0][0]) and same_bits(pr.get("rhs_raw"), out[d0][1])
    assert same_bits(pr.get("second_lhs"), out[d1][0]) and same_bits(pr.get("second_rhs"), out[d1][1])


# ---------------------------------------------------------------------------------------------------------------------
# expand
# ---------------------------------------------------------------------------------------------------------------------
def host_p(r, P, mu, delta, key):
    """(dx, w): the reduced system solved on the host in longdouble and rounded — or, past a few hundred unknowns, seeded
    random numbers: the closed forms of the expansion hold for any p."""
    cache = r.__dict__.setdefault("_p", {})
    if key not in cache:
        if r.n + r.me <= 500:
            K, b = ref.reduced_dense(P, mu, delta)
            cache[key] = np.asarray(ref.solve_dense(K, b), dtype=np.float64)
        else:
            cache[key] = np.random.default_rng(SEED + 1).uniform(-1, 1, r.n + r.me)
    return cache[key]


def read_direction(pr):
    dpn, psx, pzx = pr.download_direction()
    return dict(dpn=dpn, psx=psx, pzx=pzx, ps0=pr.get("p_s"), pz0=pr.get("p_z"), dir=pr.host()["dir"], trial_x=pr.get("trial_in")[:pr.n],
                alpha=pr.get("alpha"))


def row_lengths(r, P):
    k = np.zeros(r.mi, dtype=int)
    for row, _, _ in P.Ai:
        k[row] += 1
    return k


def check_expansion(r, P, D, E, p, mu, tau):
    """the kernel's direction D against the exact closed forms E (fr_reference.expand_exact), componentwise"""
    me, mi = r.me, r.mi
    k = row_lengths(r, P)
    kM = np.concatenate([np.zeros(2 * me, int), k, k])
    g = lambda kk: np.array([ref.gamma(ref.C_EXPAND + int(v)) for v in kk])
    within("dpn", D["dpn"], fr_list(E["dpn"]), g(kM) * np.array([float(a) for a in E["a_dpn"]]))
    within("psx", D["psx"], fr_list(E["psx"]), g(kM) * np.array([float(a) for a in E["a_psx"]]))
    within("pzx", D["pzx"], fr_list(E["pzx"]), g(kM) * np.array([float(a) for a in E["a_pzx"]]))
    within("p_s0", D["ps0"], fr_list(E["ps0"]), g(k) * np.array([float(a) for a in E["a_ps0"]]))
    within("p_z0", D["pz0"], fr_list(E["pz0"]), g(k) * np.array([float(a) for a in E["a_pz0"]]))
    # the step sizes are minima over rows, order-free: from the kernel's OWN rows they are exact, whatever the grid
    S = np.concatenate([P.s0, P.sx])
    Z = np.concatenate([P.z0, P.zx])
    a, az = ref.step_sizes_from_rows(S, np.concatenate([D["ps0"], D["psx"]]), Z, np.concatenate([D["pz0"], D["pzx"]]), tau)
    print(f"  alpha_max {D['dir']['alpha_max']!r} alpha_z {D['dir']['alpha_z']!r} (exact arithmetic: {float(E['alpha_max'])!r}, {float(E['alpha_z'])!r})")
    assert D["dir"]["alpha_max"] == a and D["dir"]["alpha_z"] == az
    assert same_bits(D["alpha"], np.array([D["dir"][q] for q in ("alpha_max", "alpha_z", "D_phi", "eliminated_min_pivot")]))
    if r.M:
        piv = ref.min_pivot_ld(P, E["delta"])
        within("eliminated_min_pivot", [D["dir"]["eliminated_min_pivot"]], [piv], [12 * U * float(piv)])
    else:
        assert D["dir"]["eliminated_min_pivot"] == 1e300
    # D_phi: the sum bound on its own terms plus what the bounds above let each term be off by
    S_ = [float(v) for v in S]
    slack = ref.gamma(E["n_D_phi"] + 4) * float(E["a_D_phi"])
    slack += sum(ref.RHO * ref.gamma(ref.C_EXPAND + 3 + int(kk)) * float(a) for kk, a in zip(kM, E["a_dpn"]))
    slack += sum(mu / s * ref.gamma(ref.C_EXPAND + 3 + int(kk)) * float(a) for kk, a, s in zip(np.concatenate([k, kM]), E["a_ps0"] + E["a_psx"], S_))
    within("D_phi", [D["dir"]["D_phi"]], [ref.ld(E["D_phi"])], [slack])
    # the first trial x = x + alpha_max dx (one fma or a product and a sum)
    within("trial x", D["trial_x"], np.asarray(P.x, LD) + LD(a) * np.asarray(p[:r.n], LD), 2 * U * (np.abs(P.x) + np.abs(a * p[:r.n])))


@pytest.mark.parametrize("name,stiff", [(m, s) for m in MODELS for s in (False, True)] + [(m, False) for m in GRIDS[1:]])
def test_expand_closed_forms(rigs, name, stiff):
    """dp_e, dn_e, dp_i, dn_i, p_s and p_z of all five blocks from a given p = (dx, w), on every row — among them the rows
    with Sigma = 1e21 and 1e-21 of the stiff state — against the closed forms evaluated exactly (rational arithmetic):
    |got - ref| <= gamma(C_EXPAND + k) sum|terms|, k the entries of the row of A_i (32 + k roundings on the longest path,
    fr_reference.py).  tests/test_fr_reference_cpu.py shows that the naive double evaluation of the same rows is outside.
    Step sizes exactly, D_phi within its sum bound, on 1, 3, 8 and 16 workgroups; twice the same bits."""
    r = rigs(name)
    P = r.load(stiff)
    pr = r.probe
    mu, delta = 0.1, 1e-4
    p = host_p(r, P, mu, delta, stiff)
    pr.put("p", p)
    pr.expand(delta, mu, TAU)
    D = read_direction(pr)
    cache = r.__dict__.setdefault("_E", {})
    if stiff not in cache:
        cache[stiff] = ref.expand_exact(P, p, mu, delta, TAU)
        cache[stiff]["delta"] = delta
    print(f"{name} stiff={stiff}: expand on {expand_blocks(r.n, r.me, r.mi)} workgroups")
    check_expansion(r, P, D, cache[stiff], p, mu, TAU)
    pr.expand(delta, mu, TAU)
    D2 = read_direction(pr)
    for q in ("dpn", "psx", "pzx", "ps0", "pz0", "trial_x", "alpha"):
        assert same_bits(D[q], D2[q]), q


@pytest.mark.parametrize("mu,delta", [(0.1, 0.0), (1e-6, 1e-4)])
@pytest.mark.parametrize("name", SMALL)
def test_expand_against_the_unreduced_solve(rigs, name, mu, delta):
    """Mild states: build's system solved on the host, expanded by the kernel, against the direct longdouble solve of the
    UNREDUCED system — every block of the direction within 1e-13 of its largest entry.  (The tolerance was measured
    against the reference: longdouble against plain double numpy on the same unreduced systems is 0.9e-16 .. 4.4e-16;
    times 8 that stays under the floor of 1e-13.)"""
    r = rigs(name)
    P = r.load(False)
    pr = r.probe
    p = host_p(r, P, mu, delta, ("mild", mu, delta))
    pr.put("p", p)
    pr.expand(delta, mu, TAU)
    D = read_direction(pr)
    R = ref.unreduced_system(P, mu, delta, exact=False)
    sol = ref.solve_dense(R["K"], R["rhs"])
    sol64 = np.linalg.solve(np.asarray(R["K"], float), np.asarray(R["rhs"], float))
    measured = float(np.max(np.abs(sol - sol64)) / np.max(np.abs(sol)))
    tol = max(8 * measured, 1e-13)
    print(f"{name} mu={mu} delta={delta}: longdouble vs double on the unreduced system {measured:.2e}, tolerance {tol:.2e}")
    W = ref.direction_from_solution(R, P, sol, TAU)
    n, nx, mi = r.n, r.n + r.M, r.mi

    def rel(what, got, want):
        want = np.asarray(want, LD)
        within(what, got, want, np.full(len(want), tol * float(np.max(np.abs(want))) if len(want) else 0.0))

    rel("dx", p[:n], W["dX"][:n])
    rel("w", p[n:], W["w"])
    rel("dpn", D["dpn"], W["dX"][n:])
    rel("p_s0", D["ps0"], W["ps"][:mi])
    rel("psx", D["psx"], W["ps"][mi:])
    rel("p_z0", D["pz0"], W["pz"][:mi])
    rel("pzx", D["pzx"], W["pz"][mi:])
    rel("D_phi", [D["dir"]["D_phi"]], [W["D_phi"]])
    # a step size -tau s / p_s moves by (tau s / p_s^2) times the error of p_s, on any row that may attain the minimum
    for q, X, PX in (("alpha_max", R["S"], W["ps"]), ("alpha_z", R["Z"], W["pz"])):
        if len(PX) == 0:
            assert D["dir"][q] == 1.0
            continue
        err = tol * float(np.max(np.abs(PX)))
        cand = [float(TAU * x / (px * px)) for x, px in zip(X, PX) if px < 0 and -TAU * x / px <= 2 * W[q]]
        within(q, [D["dir"][q]], [W[q]], [err * max(cand, default=0.0) + 2 * U])


# ---------------------------------------------------------------------------------------------------------------------
# trial metrics, second-order corrections
# ---------------------------------------------------------------------------------------------------------------------
def expanded(r, stiff=False):
    P = r.load(stiff)
    mu, delta = 0.1, 1e-4
    p = host_p(r, P, mu, delta, stiff)
    r.probe.put("p", p)
    r.probe.expand(delta, mu, TAU)
    return P, p, mu, delta, read_direction(r.probe)


def trial_reference(r, P, D, alpha, Vt):
    """the filter entry at X + alpha dX from the kernel's own direction and the trial V"""
    import copy

    Pt = copy.copy(P)
    Pt.x = r.probe.get("trial_in")[:r.n]
    pn = np.asarray(P.pn, LD) + LD(alpha) * np.asarray(D["dpn"], LD)
    S = np.concatenate([np.asarray(P.s0, LD) + LD(alpha) * np.asarray(D["ps0"], LD), np.asarray(P.sx, LD) + LD(alpha) * np.asarray(D["psx"], LD)])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = ref.filter_entry(Pt, pn, S, Vt[1:1 + r.me], Vt[1 + r.me:1 + r.me + r.mi])
        # the kernel forms every trial p, n and slack itself, v + alpha dv: one fma or two roundings, relative to |v| + |alpha dv|
        e_pn = 2 * U * (np.abs(P.pn) + np.abs(alpha * D["dpn"]))
        e_S = 2 * U * (np.concatenate([np.abs(P.s0), np.abs(P.sx)]) + np.abs(alpha) * np.concatenate([np.abs(D["ps0"]), np.abs(D["psx"])]))
        extra = {"f": ref.RHO * float(e_pn.sum()), "viol": float(3 * e_pn.sum() + e_S.sum()), "logsum": float(np.sum(e_S / np.abs(S)))}
    return want, extra


@pytest.mark.parametrize("alpha", [1.0, 0.3, -1.0])
@pytest.mark.parametrize("name", MODELS)
def test_trial_metrics(rigs, name, alpha):
    """f, viol and logsum after trial_point(alpha) + a value sweep, at alpha 1, 0.3 and alpha < 0 (the device's alpha_max):
    sums within (len + 4) 2^-53 sum|terms| (plus the roundings of the terms themselves, fr_reference.filter_entry)."""
    r = rigs(name)
    P, p, mu, delta, D = expanded(r)
    pr = r.probe
    a = D["dir"]["alpha_max"] if alpha < 0 else alpha
    pr.trial_point(a)
    pr.sweep_values_trial()
    pr.trial_metrics(alpha, mu)
    got = pr.host()["trial"]
    want, extra = trial_reference(r, P, D, a, pr.get("V_trial"))
    print(f"{name} alpha={alpha} ({a!r}): {got}")
    for q in ("f", "viol", "logsum"):
        v, b = want[q]
        if np.isnan(float(v)):  # (a slack past zero at alpha = 1: the logarithm of a negative number on both sides)
            assert np.isnan(got[q]), q
        else:
            within(q, [got[q]], [v], [b + extra[q]])
    assert got["finite"] == 1.0


@pytest.mark.parametrize("which", ["c_e", "c_i"])
def test_trial_metrics_flag_a_nan(rigs, which):
    r = rigs("tiny")
    P, p, mu, delta, D = expanded(r)
    pr = r.probe
    pr.trial_point(0.3)
    pr.sweep_values_trial()
    Vt = pr.get("V_trial")
    Vt[1 if which == "c_e" else 1 + r.me + 1] = np.nan
    pr.put("V_trial", Vt)
    pr.trial_metrics(0.3, mu)
    assert pr.host()["trial"]["finite"] == 0.0
    pr.sweep_values_trial()
    pr.trial_metrics(0.3, mu)
    assert pr.host()["trial"]["finite"] == 1.0


@pytest.mark.parametrize("name", MODELS)
def test_second_order_correction(rigs, name):
    """soc_accumulate(first), a second call, build(soc, rhs_only) and expand(soc).  The accumulators
    alpha prev + (c' at the trial point) within 8 2^-53 sum|terms| (three differences, a product, a sum; the device
    contracts to fma, so numpy's bits are not expected); the right-hand side and the corrected direction from the
    DEVICE's accumulators against the reference's, with the bounds of build and expand."""
    r = rigs(name)
    P, p, mu, delta, D = expanded(r)
    pr = r.probe
    me, mi, n = r.me, r.mi, r.n
    a1, a2 = D["dir"]["alpha_max"], 0.5
    pr.trial_point(a1)
    pr.sweep_values_trial()
    Vt = pr.get("V_trial")
    ce_t, ci_t = np.asarray(Vt[1:1 + me], LD), np.asarray(Vt[1 + me:1 + me + mi], LD)
    pn, dpn = np.asarray(P.pn, LD), np.asarray(D["dpn"], LD)
    sx, psx, s0, ps0 = np.asarray(P.sx, LD), np.asarray(D["psx"], LD), np.asarray(P.s0, LD), np.asarray(D["ps0"], LD)
    split = lambda v: (v[:me], v[me:2 * me], v[2 * me:2 * me + mi], v[2 * me + mi:])
    lhs_before = pr.get("lhs_raw")

    def accumulate(alpha, prev, prev_mag):
        """alpha prev + c'(trial), with sum|terms|, for c_e', block 0 and the bound rows"""
        al = LD(alpha)
        pnt = pn + al * dpn
        pe, ne, pi, ni = split(pnt)
        mag_pn = np.abs(pn) + np.abs(al * dpn)
        mpe, mne, mpi, mni = split(mag_pn)
        t_ce = ce_t - pe + ne
        t_c0 = (ci_t - pi + ni) - (s0 + al * ps0)
        t_x = pnt - (sx + al * psx)
        m_ce = np.abs(ce_t) + mpe + mne
        m_c0 = np.abs(ci_t) + mpi + mni + np.abs(s0) + np.abs(al * ps0)
        m_x = mag_pn + np.abs(sx) + np.abs(al * psx)
        return [al * pv + t for pv, t in zip(prev, (t_ce, t_c0, t_x))], [abs(alpha) * pm + m for pm, m in zip(prev_mag, (m_ce, m_c0, m_x))]

    pe, ne, pi, ni = split(pn)
    first = [np.asarray(P.ce, LD) - pe + ne, (np.asarray(P.ci, LD) - pi + ni) - s0, pn - sx]
    first_mag = [np.abs(np.asarray(P.ce, LD)) + pe + ne, np.abs(np.asarray(P.ci, LD)) + pi + ni + s0, pn + sx]
    want, mag = accumulate(a1, first, first_mag)
    pr.soc_accumulate(a1, True)
    for q, w_, m_ in zip(("soc_ce", "soc_c0", "soc_x"), want, mag):
        within(q + " (first)", pr.get(q), w_, 8 * U * m_)
    got1 = [pr.get(q) for q in ("soc_ce", "soc_c0", "soc_x")]
    want2, mag2 = accumulate(a2, [np.asarray(g, LD) for g in got1], [np.abs(g) for g in got1])
    pr.soc_accumulate(a2, False)
    for q, w_, m_ in zip(("soc_ce", "soc_c0", "soc_x"), want2, mag2):
        within(q + " (second)", pr.get(q), w_, 8 * U * m_)
    # the corrected right-hand side and direction, from the device's accumulators
    import copy

    Ps = copy.copy(P)
    Ps.soc_ce, Ps.soc_c0, Ps.soc_x = (pr.get(q) for q in ("soc_ce", "soc_c0", "soc_x"))
    pr.put("rhs_raw", np.full(pr.dim, np.nan))
    pr.build(delta, mu, soc=True, rhs_only=True)
    _, _, rwant, rbound = lhs_reference(r, Ps, mu, delta, soc=True)
    within("soc rhs", pr.get("rhs_raw"), rwant, rbound)
    assert same_bits(pr.get("lhs_raw"), lhs_before)
    p_soc = 0.5 * p + 0.01
    pr.put("p", p_soc)
    pr.expand(delta, mu, TAU, soc=True)
    E = ref.expand_exact(Ps, p_soc, mu, delta, TAU, soc=True)
    E["delta"] = delta
    Ds = read_direction(pr)
    # (D_phi of a corrected direction is reduced along but not used; its bound holds all the same)
    check_expansion(r, Ps, Ds, E, p_soc, mu, TAU)


@pytest.mark.parametrize("name", MODELS)
def test_save_and_restore_direction(rigs, name):
    """save_direction, an overwriting expand(soc), restore_direction: the same bits are back, in the kept copies too."""
    r = rigs(name)
    P, p, mu, delta, D = expanded(r)
    pr = r.probe
    pr.save_direction()
    for q, kept in (("dpn", "keep_dpn"), ("psx", "keep_psx"), ("pzx", "keep_pzx"), ("ps0", "keep_ps0"), ("pz0", "keep_pz0")):
        assert same_bits(pr.get(kept), D[q]), kept
    assert same_bits(pr.get("keep_p"), p)
    pr.put("soc_ce", np.full(r.me, 0.25))
    pr.put("soc_c0", np.full(r.mi, -0.5))
    pr.put("soc_x", np.full(r.M, 0.125))
    pr.put("p", 3.0 * p + 1.0)
    pr.expand(delta, mu, TAU, soc=True)
    D2 = read_direction(pr)
    assert not same_bits(D2["dpn"], D["dpn"]) or r.M == 0
    pr.restore_direction()
    D3 = read_direction(pr)
    for q in ("dpn", "psx", "pzx", "ps0", "pz0"):
        assert same_bits(D3[q], D[q]), q
    assert same_bits(pr.get("p"), p)


# ---------------------------------------------------------------------------------------------------------------------
# the iterate update: commit, and the look-ahead iterate
# ---------------------------------------------------------------------------------------------------------------------
def read_iterate(pr):
    pn, sx, zx = pr.download_state()
    return dict(inp=pr.get("in"), s=pr.get("s"), y=pr.get("y"), z=pr.get("z"), pn=pn, sx=sx, zx=zx)


def updated_reference(r, P, D, p, alpha, alpha_z, mu):
    """interior_point.hpp:775-801 (oracle/ipm.hpp:625-634) from the direction D: (values, bounds); z with the reset to
    [mu / (kappa s), kappa mu / s] on the updated slack"""
    n, me = r.n, r.me
    step = lambda v, a, d: (np.asarray(v, LD) + LD(a) * np.asarray(d, LD), 2 * U * (np.abs(v) + np.abs(a * np.asarray(d))))
    out = {"x": step(P.x, alpha, p[:n]), "y": step(P.y, alpha_z, -p[n:]), "s": step(P.s0, alpha, D["ps0"]), "pn": step(P.pn, alpha, D["dpn"]),
           "sx": step(P.sx, alpha, D["psx"])}
    return out


@pytest.mark.parametrize("mu", [0.1, 1e-12])
@pytest.mark.parametrize("name", MODELS + GRIDS[1:])
def test_lookahead_equals_commit(rigs, name, mu):
    """expand(ahead) + accept_lookahead leaves x, s_0, y, z_0, p / n, their slacks and duals and the tape input [x|y|z_0] with
    the same bits as expand + commit(alpha_max, alpha_z) from the same state; both are the reference's update, z reset
    to [mu / (kappa s), kappa mu / s].  At mu = 1e-12 the upper end of that interval is active on most rows (s z of
    order one against kappa mu = 1e-2)."""
    r = rigs(name)
    pr = r.probe
    delta = 1e-4
    P = r.load(False)
    p = host_p(r, P, 0.1, delta, False)
    pr.put("p", p)
    pr.expand(delta, mu, TAU, ahead=True)
    D = read_direction(pr)
    a, az = D["dir"]["alpha_max"], D["dir"]["alpha_z"]
    pr.accept_lookahead()
    A = read_iterate(pr)
    pr.accept_lookahead()  # (the buffers back in their first roles)
    P = r.load(False)
    pr.put("p", p)
    pr.expand(delta, mu, TAU)
    D2 = read_direction(pr)
    assert same_bits(D2["dpn"], D["dpn"]) and D2["dir"] == D["dir"]
    pr.commit(a, az, mu)
    B = read_iterate(pr)
    for q in A:
        assert same_bits(A[q], B[q]), q
    n, me, mi = r.n, r.me, r.mi
    assert same_bits(B["inp"][n:n + me], B["y"]) and same_bits(B["inp"][n + me:], B["z"])
    W = updated_reference(r, P, D, p, a, az, mu)
    within("x", B["inp"][:n], *W["x"])
    within("y", B["y"], *W["y"])
    within("s_0", B["s"], *W["s"])
    within("pn", B["pn"], *W["pn"])
    within("sx", B["sx"], *W["sx"])
    clamped = 0
    for what, z, pz, s_new in (("z_0", P.z0, D["pz0"], B["s"]), ("zx", P.zx, D["pzx"], B["sx"])):
        zn = np.asarray(z, LD) + LD(az) * np.asarray(pz, LD)
        bound = 2 * U * (np.abs(z) + np.abs(az * pz))
        lo, hi = LD(1.0) / LD(ref.KAPPA) * LD(mu) / np.asarray(s_new, LD), LD(ref.KAPPA) * LD(mu) / np.asarray(s_new, LD)
        want = np.where(zn < lo, lo, np.where(zn > hi, hi, zn))
        clamped += int(np.sum((zn < lo) | (zn > hi)))
        got = B["z"] if what == "z_0" else B["zx"]
        # (a row within its bound of an end of the interval may fall on either side of it)
        within(what, got, want, np.maximum(bound, 4 * U * np.abs(want)))
    print(f"{name} mu={mu}: {clamped} of {mi + r.M} duals reset")
    if mu == 1e-12 and r.M:
        assert clamped > 0


@pytest.mark.parametrize("name", ["tiny", "ineq_only", "chain300"])
def test_commit_resets_z_at_both_ends(rigs, name):
    """One row of block 0 and one bound row put past each end of [mu / (kappa s), kappa mu / s] through p_z; and
    alpha_z != alpha: y moves by -alpha_z w and y, z_0 are mirrored into the tape input."""
    r = rigs(name)
    P, p, mu, delta, D = expanded(r)
    pr = r.probe
    n, me, mi = r.n, r.me, r.mi
    pz0, pzx = D["pz0"].copy(), D["pzx"].copy()
    pz0[0], pz0[mi - 1] = 1e30, -P.z0[mi - 1] / 0.7 * (1 - 1e-14)  # far above; down to 1e-14 z, below mu / (kappa s)
    pzx[0], pzx[r.M - 1] = 1e30, -P.zx[r.M - 1] / 0.7 * (1 - 1e-14)
    pr.put("p_z", pz0)
    pr.put("pzx", pzx)
    a, az = 0.5 * D["dir"]["alpha_max"], 0.7  # (inside the fraction-to-the-boundary step: the new slacks stay positive)
    pr.commit(a, az, mu)
    B = read_iterate(pr)
    within("y", B["y"], np.asarray(P.y, LD) - LD(az) * np.asarray(p[n:], LD), 2 * U * (np.abs(P.y) + np.abs(az * p[n:])))
    assert same_bits(B["inp"][n:n + me], B["y"]) and same_bits(B["inp"][n + me:], B["z"])
    for z, pz, s_new, got in ((P.z0, pz0, B["s"], B["z"]), (P.zx, pzx, B["sx"], B["zx"])):
        zn = np.asarray(z, LD) + LD(az) * np.asarray(pz, LD)
        lo, hi = LD(1.0) / LD(ref.KAPPA) * LD(mu) / np.asarray(s_new, LD), LD(ref.KAPPA) * LD(mu) / np.asarray(s_new, LD)
        want = np.where(zn < lo, lo, np.where(zn > hi, hi, zn))
        assert zn[0] > hi[0] and zn[-1] < lo[-1]
        within("z", got, want, np.maximum(2 * U * (np.abs(z) + np.abs(az * pz)), 4 * U * np.abs(want)))
        assert abs(got[0] - float(hi[0])) <= 4 * U * float(hi[0]) and abs(got[-1] - float(lo[-1])) <= 4 * U * float(lo[-1])


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def check_errors(name, got, want, skip=()):
    from tests.support.frcheck import ERR_KEYS

    for q in ERR_KEYS:
        if q in skip:
            continue
        v, b = want[q]
        within(q, [got[q]], [v], [b])


@pytest.mark.parametrize("stiff", [False, True])
@pytest.mark.parametrize("name", MODELS + GRIDS[1:])
def test_errors_every_quantity(rigs, name, stiff):
    """All 29 numbers of FrErrOut (the 28 reduced ones and f_outer) with random scales, on 1, 10, 29 and 64 workgroups:
    sums within (len + 4) 2^-53 sum|terms|, max / min quantities within the roundings of the entry that attains them
    (fr_reference.error_norms), the flags exactly; twice the same bits."""
    r = rigs(name)
    P = r.load(stiff)
    pr = r.probe
    pr.errors(True, 0.1)
    got = pr.host()["err"]
    want = ref.error_norms(P)
    print(f"{name} stiff={stiff}: errors on {errors_blocks(r.n, r.me, r.mi)} workgroups")
    check_errors(name, got, want)
    pr.errors(True, 0.1)
    again = pr.host()["err"]
    assert same_bits(np.array(list(got.values())), np.array(list(again.values())))


@pytest.mark.parametrize("name", ["tiny", "chain900"])
def test_errors_flags(rigs, name):
    """check_all_V with one NaN in V gives finite = 0; ci_all_pos is 1 when every c_i - p_i + n_i (and every p, n) is
    positive and flips when one is not."""
    r = rigs(name)
    pr = r.probe
    st = r.state(False)
    me, mi = r.me, r.mi
    st["pn"][2 * me:2 * me + mi] = 1e-3   # p_i small,
    st["pn"][2 * me + mi:] = 50.0         # n_i large: c_i - p_i + n_i > 0 on every row
    P = r.load(st=st, key="all_pos")
    pr.errors(True, 0.1)
    got = pr.host()["err"]
    want = ref.error_norms(P)
    assert want["ci_all_pos"][0] == 1 and want["_ci_margin"] > 0
    assert got["ci_all_pos"] == 1.0 and got["finite"] == 1.0
    # one NaN among the derivatives
    V = pr.get("V")
    V2 = V.copy()
    V2[-1] = np.nan
    pr.put("V", V2)
    pr.errors(True, 0.1)
    assert pr.host()["err"]["finite"] == 0.0
    pr.errors(False, 0.1)
    assert pr.host()["err"]["finite"] == 1.0  # (not looked at without check_all_V: H_c is in no norm)
    pr.put("V", V)
    # one row at c_i - p_i + n_i <= 0
    row = mi // 2
    st["pn"][2 * me + row] = P.ci[row] + st["pn"][2 * me + mi + row] + 1.0
    P2 = r.load(st=st, key="one_nonpos")
    pr.errors(True, 0.1)
    got = pr.host()["err"]
    assert ref.error_norms(P2)["ci_all_pos"][0] == 0
    assert got["ci_all_pos"] == 0.0 and got["finite"] == 1.0


@pytest.mark.parametrize("name", MODELS + GRIDS[1:] + ["cart_pole100"])
def test_errors_with_the_sums_riding(rigs, name):
    """After sweep_full(false) the tape's separable sums ride in the error launch as extra workgroups: f_outer is the cost,
    within the sum bound of its closed form (fr_models.cost_terms), and every other quantity is what the plain launch
    gives, bit for bit.  The tape sums none of the general models' costs separably (their launch has no extra workgroup);
    the cart-pole's (a chain of 64 or more terms: N = 100) it does."""
    r = rigs(name)
    assert (r.probe.n_reduces > 0) == name.startswith("cart_pole")
    P = r.load(False)
    pr = r.probe
    pr.errors(False, 0.1)
    plain = pr.host()["err"]
    pr.sweep_full(False)
    pr.errors(False, 0.1, ahead=False, sums_ride=True)
    got = pr.host()["err"]
    terms = fr_models.cost_terms(name, P.x)
    f, b = ref._sum_with_bound(terms)
    b += 3 * U * float(np.abs(terms).sum())  # a square of a difference: three roundings a term
    print(f"{name}: {pr.n_reduces} separable sums; f_outer {got['f_outer']!r}, closed form {float(f)!r}")
    within("f_outer (riding)", [got["f_outer"]], [f], [b])
    within("f_outer (swept)", [plain["f_outer"]], [f], [b])
    for q in plain:
        if q != "f_outer":
            assert bits(np.array([plain[q]]))[0] == bits(np.array([got[q]]))[0], q


@pytest.mark.parametrize("name", ["tiny", "chain300"])
def test_errors_at_the_lookahead_iterate(rigs, name):
    """expand(ahead), the full tape at the look-ahead iterate, errors(ahead, sums_ride) -> err_ahead: the same numbers as
    errors() after accept_lookahead, bit for bit (they read the same buffers in the other role)."""
    r = rigs(name)
    P, p, mu, delta, D = expanded(r)
    pr = r.probe
    pr.expand(delta, mu, TAU, ahead=True)
    pr.sweep_full_lookahead(False)
    pr.errors(False, mu, ahead=True, sums_ride=True)
    ahead = pr.host()["err_ahead"]
    pr.accept_lookahead()
    pr.errors(False, mu)
    now = pr.host()["err"]
    pr.accept_lookahead()
    assert same_bits(np.array(list(ahead.values())), np.array(list(now.values())))
    assert ahead["finite"] == 1.0
