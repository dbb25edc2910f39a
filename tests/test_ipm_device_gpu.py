"""the interior-point iteration AROUND the Newton step on the
device (sleipnir_amd/csrc/ipm_kernels.h through slpx_ipm_* of include/slpx.h).

1. every scalar the kernels reduce is compared with the same formula in numpy on the
   downloaded vectors (interior_point.hpp:488-509, util/fraction_to_the_boundary_rule.hpp,
   util/filter.hpp:30-60, util/kkt_error.hpp:92-146, util/is_locally_infeasible.hpp);
2. whole solves with the iterate resident on the device agree with the host-resident
   driver (SLPX_IPM_RESIDENT=0) in exit status and solution.
Tolerances: sums of n terms in a different order — 1e-12 relative; min / max — exact.
"""
import os

import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import cases
from tests.support import models

pytestmark = pytest.mark.gpu


def csc_to_dense_T_mul(colptr, rowidx, vals, v, n):
    """(Aᵀ v)[c] for A in CSC."""
    out = np.zeros(n)
    for c in range(n):
        lo, hi = colptr[c], colptr[c + 1]
        out[c] = np.dot(vals[lo:hi], v[rowidx[lo:hi]])
    return out


def ftb(x, p, tau):
    m = p < 0
    return min(1.0, np.min(-tau / p[m] * x[m])) if m.any() else 1.0


@pytest.fixture(scope="module")
def stepped():
    N = 40
    pp = models.cart_pole(N, 5.0 / N)
    system = sa.System(pp)
    info = dict(system.info)
    n, me, mi = info["n"], info["m_e"], info["m_i"]
    info.update(off_f=0, off_ce=1, off_ci=1 + me)  # V = [f | c_e | c_i | g | ...] (nlp.hpp)
    x0 = pp.get_x()
    rng = np.random.default_rng(cases.SEED)
    scales = np.concatenate([[0.37], rng.uniform(0.2, 1.0, me), rng.uniform(0.2, 1.0, mi)])
    system.set_scaling(scales)
    x, s, y, z, mu = cases.newton_state("interior", x0, n, me, mi, scales[0])
    system.set_state(x, s, y, z, np.array([mu]))
    assert system.newton_step(True)[0] == 0
    return dict(pp=pp, system=system, info=info, scales=scales, x=x, s=s, y=y, z=z, mu=mu)


def g_dense(system, info, V):
    cp, ri = system.pattern(0)
    g = np.zeros(info["n"])
    vals = V[info["off_g"]:info["off_g"] + info["nnz_g"]]
    for c in range(info["n"]):
        g[c] = vals[cp[c]:cp[c + 1]].sum()
    return g


def test_direction_trial_commit(stepped):
    st = stepped
    system, info = st["system"], st["info"]
    n, me, mi = info["n"], info["m_e"], info["m_i"]
    x, s, y, z, mu = st["x"], st["s"], st["y"], st["z"], st["mu"]
    V = system.get("V")[0]
    p = system.get("p")[0]
    p_s, p_z = system.get("p_s")[0], system.get("p_z")[0]
    p_x, p_y = p[:n], -p[n:]
    tau = 0.99

    d = system.ipm_direction(tau)
    assert d["alpha_max"] == ftb(s, p_s, tau)
    assert d["alpha_z"] == ftb(z, p_z, tau)
    D_phi = g_dense(system, info, V) @ p_x - mu * np.sum((1.0 / s) * p_s)
    assert d["D_phi"] == pytest.approx(D_phi, rel=1e-12, abs=1e-12)

    for alpha in (d["alpha_max"], 0.25 * d["alpha_max"]):
        t = system.ipm_trial(alpha)
        # reference: the same forward sweep through the ordinary entry points
        system.set_state(x=x + alpha * p_x)
        system.sweep(False)
        Vt = system.get("V")[0]
        system.set_state(x=x)
        ce = Vt[info["off_ce"]:info["off_ce"] + me]
        ci = Vt[info["off_ci"]:info["off_ci"] + mi]
        s_t = s + alpha * p_s
        assert t["finite"] == 1.0
        # (trial x differs in the last bit: the device fuses x + alpha * p into one FMA)
        assert t["f"] == pytest.approx(Vt[info["off_f"]], rel=1e-12)
        assert t["viol"] == pytest.approx(np.abs(ce).sum() + np.abs(ci - s_t).sum(), rel=1e-12)
        assert t["logsum"] == pytest.approx(np.log(s_t).sum(), rel=1e-12, abs=1e-12)
        # feasible-IPM variant: trial s = trial c_i (only meaningful where c_i > 0; the
        # kernel's log of a negative entry is NaN exactly like the host's)
        if (ci > 0).all():
            tf = system.ipm_trial(alpha, s_from_ci=True)
            assert tf["viol"] == pytest.approx(np.abs(ce).sum(), rel=1e-12)

    alpha, alpha_z = d["alpha_max"], d["alpha_z"]
    system.ipm_trial(alpha)
    system.ipm_commit(alpha, alpha_z)
    s_new = s + alpha * p_s
    z_new = np.clip(z + alpha_z * p_z, 1e-10 * mu / s_new, 1e10 * mu / s_new)
    # (the device contracts a + alpha * b into one fused multiply-add: last-bit differences)
    xc, sc, yc, zc = (system.get(k)[0] for k in "xsyz")
    tight = dict(rtol=1e-14, atol=1e-300)
    assert np.allclose(xc, x + alpha * p_x, **tight)
    assert np.allclose(sc, s_new, **tight)
    assert np.allclose(yc, y + alpha_z * p_y, **tight)
    assert np.allclose(zc, z_new, **tight)
    # the committed iterate is what the next sweep differentiates at
    system.sweep(True)
    V_dev = system.get("V")[0]
    system.set_state(xc, sc, yc, zc)
    system.sweep(True)
    assert np.array_equal(V_dev, system.get("V")[0])
    st.update(x=xc, s=sc, y=yc, z=zc)


def test_trial_f_is_the_cost_in_closed_form_where_the_trial_launch_finishes_the_sums():
    """ipm_trial_metrics_kernel finishes the tape's separable sums itself (separable_sum_tree), and the comparison
    above takes its reference f from a sweep that runs the same tree.  Here f of the trial point is compared with the
    cart-pole's cost in closed form, J = d_f sum u_k^2 in long double, at the smallest horizon whose cost the tape sums
    separably in four partial terms or more (N = 100: sums of up to three terms come out right from a tree that walks
    its levels in any order).  Bound: a double sum of N terms in whatever order is within (N + 4) 2^-53 sum |terms| of
    it (fr_reference._sum_with_bound); the trial u_k = u + alpha p is rounded once on the device before it is squared,
    two more roundings a term at most; the product with d_f and the reference's own conversion to double are a rounding of
    the result each."""
    N = 100
    U = 2.0 ** -53
    pp = models.cart_pole(N, 5.0 / N)
    system = sa.System(pp)
    info = system.info
    n, me, mi = info["n"], info["m_e"], info["m_i"]
    assert info["nV"] - (info["off_Hc"] + info["nnz_Hc"]) >= 4  # the partial terms in V's hidden tail
    rng = np.random.default_rng(cases.SEED)
    scales = np.concatenate([[0.37], rng.uniform(0.2, 1.0, me), rng.uniform(0.2, 1.0, mi)])
    system.set_scaling(scales)
    x, s, y, z, mu = cases.newton_state("interior", pp.get_x(), n, me, mi, scales[0])
    system.set_state(x, s, y, z, np.array([mu]))
    assert system.newton_step(True)[0] == 0
    p_x = system.get("p")[0][:n]
    d = system.ipm_direction(0.99)
    for alpha in (d["alpha_max"], 0.25 * d["alpha_max"]):
        t = system.ipm_trial(alpha)
        u = (np.asarray(x, dtype=np.longdouble) + np.longdouble(alpha) * np.asarray(p_x, dtype=np.longdouble))[4 * (N + 1):]
        terms = np.longdouble(scales[0]) * u ** 2
        assert len(terms) == N
        f = float(terms.sum())
        bound = (N + 4 + 2) * U * float(np.abs(terms).sum()) + 2 * U * abs(f)
        print(f"alpha {alpha!r}: f {t['f']!r}, closed form {f!r}, bound {bound:.3e}")
        assert abs(t["f"] - f) <= bound, (alpha, t["f"], f, bound)
    system.close()
    pp.close()


def test_error_reductions(stepped):
    st = stepped
    system, info, scales = st["system"], st["info"], st["scales"]
    n, me, mi = info["n"], info["m_e"], info["m_i"]
    x, s, y, z = st["x"], st["s"], st["y"], st["z"]
    system.set_state(x, s, y, z)
    system.sweep(True)
    V = system.get("V")[0]
    e = system.ipm_errors(scales)

    g = g_dense(system, info, V)
    ce = V[info["off_ce"]:info["off_ce"] + me]
    ci = V[info["off_ci"]:info["off_ci"] + mi]
    ae_cp, ae_ri = system.pattern(1)
    ai_cp, ai_ri = system.pattern(2)
    Ae = V[info["off_Ae"]:info["off_Ae"] + info["nnz_Ae"]]
    Ai = V[info["off_Ai"]:info["off_Ai"] + info["nnz_Ai"]]
    aet = lambda v, vals=Ae: csc_to_dense_T_mul(ae_cp, ae_ri, vals, v, n)
    ait = lambda v, vals=Ai: csc_to_dense_T_mul(ai_cp, ai_ri, vals, v, n)

    rel = dict(rel=1e-12, abs=1e-13)
    # scaled (kkt_error.hpp:92-146 inputs)
    assert e["dual_inf"] == pytest.approx(np.abs(g - aet(y) - ait(z)).max(), **rel)
    assert e["sz_min"] == (s * z).min() and e["sz_max"] == (s * z).max()
    assert e["ce_inf"] == np.abs(ce).max() and e["cis_inf"] == np.abs(ci - s).max()
    assert e["y1"] == pytest.approx(np.abs(y).sum(), **rel)
    assert e["z1"] == pytest.approx(np.abs(z).sum(), **rel)
    # un-scaled (kkt_error.hpp:216-251)
    d_f, d_ce, d_ci = scales[0], scales[1:1 + me], scales[1 + me:]
    yu, zu, su = d_ce * y / d_f, d_ci * z / d_f, s / d_ci
    Ae_u = Ae / d_ce[ae_ri]
    Ai_u = Ai / d_ci[ai_ri]
    dual_u = g / d_f - aet(yu, Ae_u) - ait(zu, Ai_u)
    assert e["dual_inf_u"] == pytest.approx(np.abs(dual_u).max(), **rel)
    assert e["sz_max_u"] == pytest.approx(np.abs(su * zu).max(), **rel)
    assert e["ce_inf_u"] == pytest.approx(np.abs(ce / d_ce).max(), **rel)
    assert e["cis_inf_u"] == pytest.approx(np.abs(ci / d_ci - su).max(), **rel)
    assert e["y1_u"] == pytest.approx(np.abs(yu).sum(), **rel)
    assert e["z1_u"] == pytest.approx(np.abs(zu).sum(), **rel)
    # filter entry of the current iterate
    assert e["f"] == V[info["off_f"]]
    assert e["viol"] == pytest.approx(np.abs(ce).sum() + np.abs(ci - s).sum(), **rel)
    assert e["logsum"] == pytest.approx(np.log(s).sum(), **rel)
    # local infeasibility, divergence
    cm = np.minimum(ci, 0.0)
    assert e["aetce_sq"] == pytest.approx(np.sum(aet(ce) ** 2), **rel)
    assert e["ce_sq"] == pytest.approx(np.sum(ce ** 2), **rel)
    assert e["aitcp_sq"] == pytest.approx(np.sum(ait(cm) ** 2), **rel)
    assert e["cp_sq"] == pytest.approx(np.sum(cm ** 2), **rel)
    assert e["x_inf"] == np.abs(x).max() and e["s_inf"] == np.abs(s).max()
    assert e["finite"] == 1.0
    assert e["ci_all_pos"] == float((ci > 0).all())

    # a non-finite iterate is reported
    xb = x.copy()
    xb[3] = np.inf
    system.set_state(x=xb)
    assert system.ipm_errors(scales)["finite"] == 0.0
    system.set_state(x=x)


def _solve(make, resident):
    old = os.environ.get("SLPX_IPM_RESIDENT")
    os.environ["SLPX_IPM_RESIDENT"] = "1" if resident else "0"
    try:
        pp = make()
        status, rep = pp.solve()
        return status, rep, pp.get_x(), pp.duals()
    finally:
        if old is None:
            del os.environ["SLPX_IPM_RESIDENT"]
        else:
            os.environ["SLPX_IPM_RESIDENT"] = old


@pytest.mark.parametrize("name,makes", [
    # Whether this IPM gets through the cart-pole swing-up on a given grid is sensitive to last-bit
    # differences (the reference's own sweep drops N=200; profiles/r03_horizon_sweep.txt: N=50, 200,
    # 700, 800, 1000 end LOCALLY_INFEASIBLE with the multifrontal step, N=150 does with it and not
    # with the pair lists, N=300 the other way round under some switches of
    # profiles/switch_matrix.sh) — so the horizon is the first of a short list on which the host
    # driver converges; the resident driver must then converge on it too.
    ("cart_pole", [lambda: models.cart_pole(300, 5.0 / 300), lambda: models.cart_pole(150, 5.0 / 150),
                   lambda: models.cart_pole(500, 5.0 / 500), lambda: models.cart_pole(400, 5.0 / 400)]),
    ("cart_pole_100", [lambda: models.cart_pole(100, 0.05)]),   # restoration on the way
    ("flywheel_50", [lambda: models.flywheel(50, 0.005)]),
])
def test_resident_solve_matches_host_driver(name, makes):
    tried = []
    for make in makes:
        st_h, rep_h, x_h, duals_h = _solve(make, resident=False)
        st_d, rep_d, x_d, duals_d = _solve(make, resident=True)
        tried.append((st_h, st_d))
        # either driver may leave a swing-up grid as locally infeasible (-2); nothing else is a legitimate end
        assert st_h in (0, -2) and st_d in (0, -2), tried
        if st_h == 0 and st_d == 0:
            break
    assert st_d == st_h == 0, f"no horizon of the list on which both drivers converge: {tried}"
    assert rep_d["final_error"] <= 1e-8 and rep_h["final_error"] <= 1e-8
    assert rep_d["iterations"] > 0 and rep_h["iterations"] > 0
    scale = max(1.0, np.abs(x_h).max())
    same = np.abs(x_d - x_h).max() <= 1e-5 * scale
    # Same algorithm, different summation order in the norms: the first iterations coincide
    # line for line, later ones need not (ill-conditioned early systems amplify last-bit
    # differences; cart-pole N=50 takes 331 iterations one way and 169 the other).  The flywheel
    # problem has one solution and both must end there; the cart-pole swing-up has several local
    # ones (the pole can go round either way), and on some grids a last-bit change anywhere —
    # r02: the KKT products no longer contracted into fused multiply-adds — sends the two drivers
    # to different ones (profiles/r02_oracle_sensitivity.txt: the reference algorithm itself does
    # that under 1e-13 perturbations).  Both are KKT points to the tolerance, checked above.
    if name.startswith("flywheel"):
        assert same
    else:
        print(f"{name}: tried {tried}; host driver {rep_h['iterations']} iterations, resident {rep_d['iterations']}; "
              f"same local solution: {bool(same)}")


@pytest.mark.parametrize("resident", [False, True])
def test_a_solve_is_reproducible_bit_for_bit(resident):
    """Nothing on the path sums in a run-dependent order (no floating-point atomics: the r02
    refinement of the multiplier estimate used them at first, and the trajectory of a swing-up —
    chaotic in the last bits, profiles/r02_oracle_sensitivity.txt — then differed from run to
    run): two solves of the same model give the same iterates, to the bit."""
    runs = [_solve(lambda: models.cart_pole(100, 0.05), resident) for _ in range(3)]
    st0, rep0, x0, duals0 = runs[0]
    assert st0 == 0
    for st, rep, x, duals in runs[1:]:
        assert st == st0 and rep["iterations"] == rep0["iterations"]
        assert np.array_equal(x, x0)
        for a, b in zip(duals, duals0):
            assert np.array_equal(a, b)


def _solve_with_env(make, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pp = make()
        status, rep = pp.solve()
        return status, rep, pp.get_x(), pp.duals()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name,make", [
    ("cart_pole_50", lambda: models.cart_pole(50, 0.1)),
    ("cart_pole_100", lambda: models.cart_pole(100, 0.05)),     # restoration on the way
    ("cart_pole_300", lambda: models.cart_pole(300, 5.0 / 300)),
    ("flywheel_50", lambda: models.flywheel(50, 0.005)),
])
def test_twin_attempts_follow_the_sequential_policy_bit_for_bit(name, make, capfd):
    """Two regularizations per launch (ldlt_mf_twin_kernel, NewtonSystem::compute_twin) are judged in the
    order sparse_regularized_ldlt.hpp:64-152 tries them: the iterates, the iteration count and the number of
    factorizations the policy counts are those of one attempt per launch (SLPX_TWIN=0), to the bit — and on
    the cart-pole, which regularizes throughout, the second attempt of a launch IS taken."""
    capfd.readouterr()
    st_t, rep_t, x_t, duals_t = _solve_with_env(make, SLPX_TWIN_VERBOSE="1")
    err = capfd.readouterr().err
    st_s, rep_s, x_s, duals_s = _solve_with_env(make, SLPX_TWIN="0")
    assert st_t == st_s
    assert rep_t["iterations"] == rep_s["iterations"] and rep_t["factorizations"] == rep_s["factorizations"]
    assert np.array_equal(x_t, x_s)
    for a, b in zip(duals_t, duals_s):
        assert np.array_equal(a, b)
    lines = [l for l in err.splitlines() if l.startswith("slpx twin attempts:")]
    assert lines or cases.OUTER_SWITCHES, err  # (the host-resident driver, SLPX_IPM_RESIDENT=0, prints none)
    launches = sum(int(l.split()[3]) for l in lines)
    taken = sum(int(l.split("second of")[1].split()[0]) for l in lines)
    if not cases.OUTER_SWITCHES:  # (the pair-list step, unfused launches, ... have no twin attempts)
        assert launches > 0
        if name.startswith("cart_pole"):
            assert taken > 0, lines
    print(f"{name}: {rep_t['iterations']} iterations, {rep_t['factorizations']} factorizations, {launches} twin launches, "
          f"second attempt taken {taken} times")


@pytest.mark.parametrize("name,make", [
    ("cart_pole_50", lambda: models.cart_pole(50, 0.1)),
    ("cart_pole_100", lambda: models.cart_pole(100, 0.05)),     # restoration on the way
    ("cart_pole_300", lambda: models.cart_pole(300, 5.0 / 300)),
    ("cart_pole_1000", lambda: models.cart_pole(1000, 5.0 / 1000)),  # 512-thread twin launches, restoration, a long filter
    ("flywheel_50", lambda: models.flywheel(50, 0.005)),
])
def test_iterations_decided_on_the_device_are_the_hosts_bit_for_bit(name, make, capfd):
    """The common iteration's decisions — the filter's acceptance of the full step (util/filter.hpp:109-172), the
    exits and the barrier test of interior_point.hpp:387-408 and :809-832 — taken by the launch that reduces the
    look-ahead iterate's norms (ipm_decide.h, ipm_error_fold), with the next step enqueued behind it before the host
    has seen anything: the iterates, the iteration count and the factorization count are those of the host deciding
    every iteration (SLPX_IPM_PIPELINE=0), to the bit, and most iterations ARE decided on the device."""
    capfd.readouterr()
    st_p, rep_p, x_p, duals_p = _solve_with_env(make, SLPX_TWIN_VERBOSE="1")
    err = capfd.readouterr().err
    st_h, rep_h, x_h, duals_h = _solve_with_env(make, SLPX_IPM_PIPELINE="0")
    # (default: the deciding error launch RIDES in the step it decides about, which holds its results back until the
    # verdict is in — ldlt_mf_twin_kernel<.., true>; SLPX_IPM_RIDE=0: it runs in front of a step that passes at a gate)
    st_g, rep_g, x_g, duals_g = _solve_with_env(make, SLPX_IPM_RIDE="0")
    assert st_g == st_h and rep_g["iterations"] == rep_h["iterations"] and rep_g["factorizations"] == rep_h["factorizations"]
    assert np.array_equal(x_g, x_h)
    for a, b in zip(duals_g, duals_h):
        assert np.array_equal(a, b)
    assert st_p == st_h
    assert rep_p["iterations"] == rep_h["iterations"] and rep_p["factorizations"] == rep_h["factorizations"]
    assert rep_p["restorations"] == rep_h["restorations"]
    assert np.array_equal(x_p, x_h)
    for a, b in zip(duals_p, duals_h):
        assert np.array_equal(a, b)
    lines = [l for l in err.splitlines() if l.startswith("slpx pipelined iterations:")]
    assert lines or cases.OUTER_SWITCHES, err
    decided = sum(int(l.split()[3]) for l in lines)
    passed = sum(int(l.split("the device,")[1].split()[0]) for l in lines)
    if not cases.OUTER_SWITCHES and os.environ.get("SLPX_IPM_PIPELINE") != "0":
        assert decided >= (rep_p["iterations"] - rep_p["restoration_iterations"]) // 2, lines
    print(f"{name}: {rep_p['iterations']} iterations, {decided} decided on the device, {passed} steps enqueued ahead let pass")
