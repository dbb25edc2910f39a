"""The full vjp on the device (include/slpx.h: the full vjp; sleipnir_amd/csrc/sensitivity.hip: sens_adjoint_rhs_kernel,
sens_vjp_full_kernel): slpx_problem_sensitivity_vjp_full and slpx_problem_sensitivity_batch_vjp_full — cotangents on x,
s, y, z and on the optimal cost, one solve.

Models: tests/support/param_models.py, sens_models.py, sens_batch_models.py.  What is compared with what:
  1  closed forms        mq (1e-12), mq_scaled (1e-10), boxed (1e-6, the bound test_sensitivity_gpu.py uses for it), and
                         the sign under maximize()
  2  the Jacobian        sum_blocks J_block^T v_block + vcost (J_x g + f_p) after sensitivity(), each cotangent alone and
                         all together; relative to the largest expected entry, 1e-12 for mq and 1e-6 otherwise.  g comes
                         from a sweep read through the system handle; f_p from central differences of that sweep's f,
                         which are exact up to rounding here: f is quadratic in every parameter of these models.
  3  the dot product     <v, jvp(dp)> + vcost dcost(dp) = <vjp_full(v), dp>, no Jacobian; each side is a sum of block terms
                         with an error relative to its own size, so the difference is taken relative to the largest term
  4  the old entry points and "nothing else moved"
  5  batched             per instance as in 2, permuted, a NaN in vz of one instance, the kept factorization, a following
                         solve_batch
  6  lane wrap           chain(130): m_i = 260 and n + m_e = 392, both strided sums of sens_vjp_full_kernel go round twice
  7  errors
  8  the torch layers

THE vz BLOCK where Sigma = z / s is of order 1e9 (bounds that bind at mu of order 1e-9: chain4 row 0): dz = -Sigma ds is
an O(1) number computed from terms of order 1e9, forward and reverse alike.  Where a case with a cotangent on z exceeds
1e-6 there, it is held to ten times the error of the existing jvp against the Jacobian on dz in the same run — one
order, because both routes share the factorization and differ by one refined solve (profiles/sensitivity_adjoint.txt
keeps both figures).

Figures are printed (run with -s)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from sleipnir_amd import SlpxError
from tests.support import param_models as pmod
from tests.support import sens_batch_models as sb
from tests.support import sens_models as smod
from tests.test_sensitivity_gpu import CHAINS, bits_equal, kkt_residual, parameter_values, python_mq, solved

pytestmark = pytest.mark.gpu

SUCCESS = 0
BLOCKS = ("x", "s", "y", "z", "cost")
JAC = {"x": "dx", "s": "ds", "y": "dy", "z": "dz"}


@pytest.fixture
def m(fresh):
    mm = pmod.new_model()
    mm.be.reset()
    return mm


def sizes(p):
    n, me, mi = p.dims
    return {"x": n, "s": mi, "y": me, "z": mi, "cost": 1}


def subsets(p):
    """each cotangent the model has rows for alone, and all of them together"""
    present = [k for k in BLOCKS if sizes(p)[k]]
    return [(k,) for k in present] + [tuple(present)]


def cotangents(p, seed=5):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(-1.0, 1.0, size) for k, size in sizes(p).items()}


def unit(size, j):
    v = np.zeros(size)
    v[j] = 1.0
    return v


def cost_derivatives(sysm, dims, x, s, y, z, params):
    """(g (n), f_p (n_p)) at unit scales through the system handle (installed by the caller): g from the sweep's V, f_p
    from central differences of the sweep's f with h = 1e-2 — exact up to eps |f| / h for a cost quadratic in p."""
    n = dims[0]
    V = kkt_residual(sysm, dims, x, s, y, z, params)[1]
    gcp, _ = sysm.pattern(0)
    off_g = sysm.info["off_g"]
    g = np.array([V[off_g + gcp[c]:off_g + gcp[c + 1]].sum() for c in range(n)])
    f_p = np.zeros(len(params))
    h = 1e-2
    for q in range(len(params)):
        up, dn = np.array(params, dtype=np.float64), np.array(params, dtype=np.float64)
        up[q] += h
        dn[q] -= h
        f_p[q] = (kkt_residual(sysm, dims, x, s, y, z, up)[1][0] - kkt_residual(sysm, dims, x, s, y, z, dn)[1][0]) / (2.0 * h)
    sysm.set_parameters(np.asarray(params, dtype=np.float64))  # (as they were)
    return g, f_p


def expected_from_jacobian(jac, v, keys, g, f_p):
    """sum_blocks J_block^T v_block + vcost (J_x g + f_p); jac[k]: (n_p, .)"""
    out = np.zeros(jac["dx"].shape[0])
    for k in keys:
        if k == "cost":
            out = out + float(v["cost"][0]) * (jac["dx"] @ g + f_p)
        else:
            out = out + jac[JAC[k]] @ v[k]
    return out


def rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), 1e-300)


# ---- 1. closed forms -------------------------------------------------------------------------------------------------
def test_closed_form_mq(m):
    """x = (a + b - 1) / 2, y = (b - a + 1) / 2, cost* = (b - 1 - a)^2 / 2, lambda = b - 1 - a ... (a, b) = (2, 1)"""
    pm = pmod.mq(m, (2.0, 1.0))
    solved(pm)
    p = pm.p.p
    grad, info = p.sensitivity_vjp_full(cost=1.0)
    dy, _ = p.sensitivity_vjp_full(y=[1.0])
    print("mq: cost gradient", grad, "dy", dy, info)
    assert np.max(np.abs(grad - np.array([2.0, -2.0]))) <= 1e-12
    assert np.max(np.abs(dy - np.array([-1.0, 1.0]))) <= 1e-12
    assert info["solves"] >= 1 and info["n_p"] == 2 and info["solve_status"] == SUCCESS
    pm.close()


def test_closed_form_units(m):
    pm = smod.mq_scaled(m, (2.0, 1.0))
    solved(pm)
    p = pm.p.p
    grad, _ = p.sensitivity_vjp_full(cost=1.0)
    dy, _ = p.sensitivity_vjp_full(y=[1.0])
    print("mq_scaled: cost gradient", grad, "dy", dy)
    assert np.max(np.abs(grad - 1000.0 * np.array([2.0, -2.0]))) <= 1e-10 * 1000.0
    assert np.max(np.abs(dy - np.array([-2.0, 2.0]))) <= 1e-10
    pm.close()


def test_closed_form_boxed(m):
    """min (x - 3)^2, lo <= x <= hi at (0, 2): x = hi, cost* = (hi - 3)^2, z_hi = 2 (3 - hi), s_hi = 0, s_lo = hi - lo"""
    pm = pmod.boxed(m, (0.0, 2.0))
    solved(pm)
    p = pm.p.p
    lo, hi = 0, 1
    cost, _ = p.sensitivity_vjp_full(cost=1.0)
    z_hi, _ = p.sensitivity_vjp_full(z=unit(2, hi))
    s_hi, _ = p.sensitivity_vjp_full(s=unit(2, hi))
    s_lo, _ = p.sensitivity_vjp_full(s=unit(2, lo))
    print("boxed (0, 2): cost", cost, "z_hi", z_hi, "s_hi", s_hi, "s_lo", s_lo)
    assert np.max(np.abs(cost - np.array([0.0, -2.0]))) <= 1e-6
    assert np.max(np.abs(z_hi - np.array([0.0, -2.0]))) <= 1e-6
    assert np.max(np.abs(s_hi - np.array([0.0, 0.0]))) <= 1e-6
    assert np.max(np.abs(s_lo - np.array([-1.0, 1.0]))) <= 1e-6
    pm.close()


def test_the_sign_is_that_of_the_reported_cost(m):
    """maximize(-c) stores f = c: the solve reports c, and c is what is differentiated.  On m2 the gradient of the optimal
    cost vanishes whatever the sign (cost* = 0 for every a), so mq pins it: (2, -2) as with minimize(c), not (-2, 2); and
    the cost solve_batch reports moves by that much."""
    from tests.support import model

    p2 = model.NlpProblem(m)
    x, y = p2.decision_variable(0.0), p2.decision_variable(0.0)
    a = m.variable(2.0)
    p2.maximize(m.constant(0.0) - (m.pow(x - a, 2) + m.pow(y - 1, 2)))
    status, _ = p2.p.solve()
    assert status == SUCCESS
    grad, _ = p2.p.sensitivity_vjp_full(cost=1.0)
    dx, _ = p2.p.sensitivity_vjp_full(x=[1.0, 0.0])
    print("m2 maximize(-c): cost gradient", grad, "dx/da", dx)
    assert np.max(np.abs(grad)) <= 1e-12 and abs(dx[0] - 1.0) <= 1e-12
    p2.p.close()

    q = model.NlpProblem(m)
    x, y = q.decision_variable(0.0), q.decision_variable(0.0)
    a, b = m.variable(2.0), m.variable(1.0)
    q.maximize(m.constant(0.0) - (m.pow(x - a, 2) + m.pow(y - 1, 2)))
    q.eq(x + y, b)
    status, _ = q.p.solve()
    assert status == SUCCESS
    grad, _ = q.p.sensitivity_vjp_full(cost=1.0)
    h = 1e-3
    r = q.p.solve_batch(np.zeros((2, 2)), parameters=np.array([[2.0 + h, 1.0], [2.0 - h, 1.0]]), tolerance=1e-12)
    fd = (r["cost"][0] - r["cost"][1]) / (2.0 * h)
    print("mq maximize(-c): cost gradient", grad, "reported costs", r["cost"], "their central difference in a", fd)
    assert np.max(np.abs(grad - np.array([2.0, -2.0]))) <= 1e-12
    assert r["cost"][0] > 0.0 and abs(fd - grad[0]) <= 1e-6
    q.p.close()


# ---- 2. against the Jacobian, 3. the dot product ---------------------------------------------------------------------
CASES23 = ["mq"] + list(CHAINS)


def solved_case(m, case):
    pm = pmod.mq(m, (2.0, 1.0)) if case == "mq" else CHAINS[case](m)
    solved(pm)
    return pm


@pytest.mark.parametrize("case", CASES23)
def test_against_the_jacobian(m, case):
    pm = solved_case(m, case)
    p = pm.p.p
    dims = p.dims
    x, s, y, z, mu = p.iterate()
    n_p = len(pm.params)
    jac = p.sensitivity()
    assert jac["info"]["factorizations"] >= 1
    v = cotangents(p)
    dp = np.random.default_rng(5).uniform(-1.0, 1.0, n_p)
    jvp = p.sensitivity_jvp(dp)
    got = {}
    for keys in subsets(p):
        got[keys], info = p.sensitivity_vjp_full(**{k: v[k] for k in keys})
        assert info["factorizations"] == 0 and info["solves"] >= 1 and info["n_p"] == n_p, (keys, info)
    # (the handle last: asking for it drops the kept factorization)
    sysm = p.system()
    sysm.set_scaling(np.ones(1 + dims[1] + dims[2]))
    g, f_p = cost_derivatives(sysm, dims, x, s, y, z, parameter_values(pm))
    tol = 1e-12 if case == "mq" else 1e-6
    e_jvp_dz = rel(jvp["dz"], dp @ jac["dz"]) if dims[2] else 0.0
    if dims[2]:
        print(f"{case}: the existing jvp against the Jacobian on dz {e_jvp_dz:.3e}, Sigma up to {np.max(z / s):.3e}")
    for keys in subsets(p):
        want = expected_from_jacobian(jac, v, keys, g, f_p)
        err = rel(got[keys], want)
        print(f"{case} {'+'.join(keys)}: vjp_full against the Jacobian {err:.3e} (largest expected entry {np.max(np.abs(want)):.3e})")
        if "z" in keys and err > tol and case == "chain4 row 0":
            print(f"{case} {'+'.join(keys)}: above {tol:.0e} with Sigma up to {np.max(z / s):.3e}; jvp against the Jacobian on dz {e_jvp_dz:.3e}")
            assert err <= 10.0 * e_jvp_dz, (keys, err, e_jvp_dz)
            continue
        assert err <= tol, (case, keys, err)
    pm.close()


@pytest.mark.parametrize("case", CASES23)
def test_dot_product(m, case):
    pm = solved_case(m, case)
    p = pm.p.p
    dims = p.dims
    x, s, y, z, mu = p.iterate()
    n_p = len(pm.params)
    v = cotangents(p, seed=6)
    dp = np.random.default_rng(7).uniform(-1.0, 1.0, n_p)
    jvp = p.sensitivity_jvp(dp)
    got = {}
    for keys in subsets(p):
        got[keys], info = p.sensitivity_vjp_full(**{k: v[k] for k in keys})
        assert info["factorizations"] == 0, (keys, info)
    sysm = p.system()
    sysm.set_scaling(np.ones(1 + dims[1] + dims[2]))
    g, f_p = cost_derivatives(sysm, dims, x, s, y, z, parameter_values(pm))
    forward = {"x": jvp["dx"], "s": jvp["ds"], "y": jvp["dy"], "z": jvp["dz"], "cost": np.array([g @ jvp["dx"] + f_p @ dp])}
    tol = 1e-12 if case == "mq" else 1e-6
    for keys in subsets(p):
        terms = [float(np.dot(v[k], forward[k])) for k in keys]
        left, right = sum(terms), float(got[keys] @ dp)
        scale = max([abs(t) for t in terms] + [abs(left), abs(right), 1e-300])
        err = abs(left - right) / scale
        print(f"{case} {'+'.join(keys)}: <v, J dp> {left:+.12e}  <J^T v, dp> {right:+.12e}  relative to the largest term {err:.3e}")
        assert err <= tol, (case, keys, left, right, err)
    pm.close()


# ---- 4. the old entry points, and nothing else moved -----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES23)
def test_vx_alone_is_the_old_vjp(m, case):
    pm = solved_case(m, case)
    p = pm.p.p
    v = cotangents(p, seed=8)["x"]
    old, _ = p.sensitivity_vjp(v)
    new, info = p.sensitivity_vjp_full(x=v)
    assert info["factorizations"] == 0
    assert bits_equal(old, new), (old, new)
    pm.close()


BUILD4 = {
    "mq": lambda m: pmod.mq(m, (2.0, 1.0)),
    "boxed": lambda m: pmod.boxed(m, (0.0, 1.0)),
    "chain4": lambda m: CHAINS["chain4 row 0"](m),
}


@pytest.mark.parametrize("case", list(BUILD4))
def test_a_following_solve_is_not_affected(m, case):
    with_calls, without = BUILD4[case](m), BUILD4[case](m)
    results = []
    for pm, call in ((with_calls, True), (without, False)):
        p = pm.p.p
        x0 = p.get_x()
        solved(pm)
        if call:
            compiles = p.compile_count()
            v = cotangents(p)
            present = {k: v[k] for k in BLOCKS if sizes(p)[k]}
            p.sensitivity_vjp_full(**present)
            p.sensitivity_vjp_full(cost=1.0)
            assert p.compile_count() == compiles
        p.set_x(x0)
        status, rep = p.solve()
        results.append((status, rep["iterations"], p.get_x(), *p.duals(), *p.iterate()))
    a, b = results
    assert a[0] == b[0] == SUCCESS and a[1] == b[1], (a[:2], b[:2])
    for u, w in zip(a[2:], b[2:]):
        assert bits_equal(u, w)
    with_calls.close()
    without.close()


# ---- 5. batched ------------------------------------------------------------------------------------------------------
def batch_cotangents(p, B, seed=9):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(-1.0, 1.0, (B, size) if k != "cost" else (B,)) for k, size in sizes(p).items()}


def batch_present(p, v, keys=BLOCKS):
    return {k: v[k] for k in keys if sizes(p)[k]}


@pytest.mark.parametrize("case,B", [(c, B) for c in ("mq", "boxed", "chain4") for B in (3, 5)], ids=lambda a: str(a))
def test_batched_against_the_jacobian_per_instance(m, case, B):
    ref = sb.reference(m, case)
    pm, rows = sb.build(m, case)
    p = pm.p.p
    dims = p.dims
    rows = rows[:B]
    it = sb.iterate_rows(ref, range(B))
    jac = p.sensitivity_batch(it, rows)
    v = batch_cotangents(p, B)
    got = {}
    for keys in subsets(p):
        r = p.sensitivity_batch_vjp_full(it, rows, **batch_present(p, v, keys))
        assert list(r["status"]) == [0] * B and r["grad"].shape == (B, rows.shape[1])
        assert all(i["factorizations"] == 0 and i["solves"] >= 1 for i in r["info"]), keys
        got[keys] = r["grad"]
    old = p.sensitivity_batch_vjp(it, rows, v["x"])
    assert bits_equal(old["grad"], got[("x",)])
    sysm = p.system()
    sysm.set_scaling(np.ones(1 + dims[1] + dims[2]))
    tol = 1e-12 if case == "mq" else 1e-6
    for b in range(B):
        g, f_p = cost_derivatives(sysm, dims, it["x"][b], it["s"][b], it["y"][b], it["z"][b], rows[b])
        jb = {k: jac[k][b] for k in JAC.values()}
        for keys in subsets(p):
            vb = {k: np.atleast_1d(v[k][b]) for k in keys}
            want = expected_from_jacobian(jb, vb, keys, g, f_p)
            err = rel(got[keys][b], want)
            print(f"{case} B={B} instance {b} {'+'.join(keys)}: {err:.3e} (largest expected entry {np.max(np.abs(want)):.3e})")
            assert err <= tol, (case, b, keys, err)
    pm.close()


def test_batched_instances_do_not_notice_each_other(m):
    """permuted: equal bits per instance; a NaN in vz of instance 1: status [0, 1, 0, 0, 0], its gradient row NaN, the
    others' bits unchanged; the same rows again: factorizations = 0"""
    case, B = "chain4", 5
    ref = sb.reference(m, case)
    pm, rows = sb.build(m, case)
    p = pm.p.p
    v = batch_cotangents(p, B)
    it = sb.iterate_rows(ref, range(B))
    straight = p.sensitivity_batch_vjp_full(it, rows, **v)
    again = p.sensitivity_batch_vjp_full(it, rows, **v)
    assert all(i["factorizations"] >= 1 for i in straight["info"]) and all(i["factorizations"] == 0 for i in again["info"])
    assert bits_equal(straight["grad"], again["grad"])
    order = [3, 0, 4, 1, 2]
    permuted = p.sensitivity_batch_vjp_full(sb.iterate_rows(ref, order), rows[order], **{k: a[order] for k, a in v.items()})
    for pos, b in enumerate(order):
        assert bits_equal(straight["grad"][b], permuted["grad"][pos]), (b, pos)
    bad_v = {k: a.copy() for k, a in v.items()}
    bad_v["z"][1, 2] = np.nan
    bad = p.sensitivity_batch_vjp_full(it, rows, **bad_v)
    assert list(bad["status"]) == [0, 1, 0, 0, 0], bad["status"]
    assert np.all(np.isnan(bad["grad"][1]))
    for b in (0, 2, 3, 4):
        assert bits_equal(straight["grad"][b], bad["grad"][b]), b
    bad_v = {k: a.copy() for k, a in v.items()}
    bad_v["cost"][4] = np.inf
    bad = p.sensitivity_batch_vjp_full(it, rows, cost=bad_v["cost"], y=v["y"])
    assert list(bad["status"]) == [0, 0, 0, 0, 1] and np.all(np.isnan(bad["grad"][4]))
    pm.close()


@pytest.mark.parametrize("case", ["mq", "chain4"])
def test_a_following_solve_batch_is_not_affected(m, case):
    ref = sb.reference(m, case)
    with_calls, rows = sb.build(m, case)
    without, _ = sb.build(m, case)
    it = sb.iterate_rows(ref, range(5))
    results = []
    for pm, call in ((with_calls, True), (without, False)):
        p = pm.p.p
        x0 = np.repeat(p.get_x()[None, :], 5, axis=0)
        first = p.solve_batch(x0, parameters=rows, warm_start={})
        if call:
            v = batch_cotangents(p, 5)
            p.sensitivity_batch_vjp_full(it, rows, **batch_present(p, v))
            p.sensitivity_batch_vjp_full(it, rows, cost=np.ones(5))
        r = p.solve_batch(x0, parameters=rows, warm_start={})
        assert list(first["status"]) == [SUCCESS] * 5
        results.append(r)
    a, b = results
    for k in ("status", "iterations", "restorations", "x", "s", "y", "z", "mu", "cost", "repaired"):
        assert np.array_equal(a[k], b[k]) and bits_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), k
    with_calls.close()
    without.close()


# ---- 6. lane wrap ----------------------------------------------------------------------------------------------------
LANE_WRAP_STAGES = 130  # n = 261, m_e = 131, m_i = 260: m_i > 256 and n + m_e = 392 > 256


def test_lane_wrap(m):
    """The batched calls take any interior iterate: no solve.  f_p in closed form here (263 parameters): the cost is
    sum_k (X_{k+1} - r_k)^2 + 0.1 U_k^2, so df/dr_k = -2 (X_{k+1} - r_k) and nothing else; g from a sweep."""
    stages, B = LANE_WRAP_STAGES, 2
    rows = pmod.chain_rows(stages, B)
    pm = pmod.chain(m, stages, rows[0])
    p = pm.p.p
    n, me, mi = dims = p.dims
    assert mi > 256 and n + me > 256, dims
    rng = np.random.default_rng(13)
    it = {"x": rng.uniform(-1.0, 1.0, (B, n)), "s": rng.uniform(0.5, 2.0, (B, mi)), "y": rng.uniform(-1.0, 1.0, (B, me)),
          "z": rng.uniform(0.5, 2.0, (B, mi)), "mu": np.ones(B)}
    v = batch_cotangents(p, B, seed=14)
    jac = p.sensitivity_batch(it, rows)
    assert list(jac["status"]) == [0] * B, jac["status"]
    print("chain(130): regularization (delta, gamma)", [(i["delta"], i["gamma"]) for i in jac["info"]])
    got = {}
    for keys in subsets(p):
        r = p.sensitivity_batch_vjp_full(it, rows, **batch_present(p, v, keys))
        assert list(r["status"]) == [0] * B and all(i["factorizations"] == 0 for i in r["info"])
        got[keys] = r["grad"]
    sysm = p.system()
    sysm.set_scaling(np.ones(1 + me + mi))
    gcp, _ = sysm.pattern(0)
    for b in range(B):
        V = kkt_residual(sysm, dims, it["x"][b], it["s"][b], it["y"][b], it["z"][b], rows[b])[1]
        off_g = sysm.info["off_g"]
        g = np.array([V[off_g + gcp[c]:off_g + gcp[c + 1]].sum() for c in range(n)])
        f_p = np.zeros(rows.shape[1])
        f_p[3:3 + stages] = -2.0 * (it["x"][b][1:stages + 1] - rows[b][3:3 + stages])
        jb = {k: jac[k][b] for k in JAC.values()}
        for keys in subsets(p):
            vb = {k: np.atleast_1d(v[k][b]) for k in keys}
            want = expected_from_jacobian(jb, vb, keys, g, f_p)
            err = rel(got[keys][b], want)
            print(f"chain(130) instance {b} {'+'.join(keys)}: {err:.3e} (largest expected entry {np.max(np.abs(want)):.3e})")
            assert err <= 1e-6, (b, keys, err)
    sysm.set_parameters(rows[0])
    pm.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def test_errors(m, slpx):
    L = slpx.lib()
    pm = pmod.mq(m, (2.0, 1.0))
    p = pm.p.p
    out = np.zeros(8)
    cot = slpx.Cotangent()
    cot.vcost = out.ctypes.data
    size = ctypes.sizeof(cot)
    call = lambda h, c: L.slpx_problem_sensitivity_vjp_full(h, ctypes.byref(c), size, out.ctypes.data, None)
    assert call(p._h, cot) == -100 and b"has not been solved" in L.slpx_last_error()
    assert call(None, cot) == -100 and b"null problem" in L.slpx_last_error()
    solved(pm)
    assert call(p._h, slpx.Cotangent()) == -100 and b"no cotangent" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_vjp_full(p._h, None, size, out.ctypes.data, None) == -100 and b"no cotangent" in L.slpx_last_error()
    with pytest.raises(SlpxError, match="no cotangent"):
        p.sensitivity_vjp_full()
    # members beyond cotangent_bytes are absent: only vx .. vz are read, and they are NULL
    assert L.slpx_problem_sensitivity_vjp_full(p._h, ctypes.byref(cot), 4 * ctypes.sizeof(ctypes.c_void_p), out.ctypes.data, None) == -100
    assert b"no cotangent" in L.slpx_last_error()
    out[0] = 1.0
    assert call(p._h, cot) == 0 and L.slpx_problem_sensitivity_vjp_full(p._h, ctypes.byref(cot), size, None, None) == 0
    # a cotangent on rows the model does not have is ignored
    with_s, _ = p.sensitivity_vjp_full(cost=1.0, s=np.zeros(0))
    assert bits_equal(with_s, p.sensitivity_vjp_full(cost=1.0)[0])
    with pytest.raises(SlpxError, match="must have shape"):
        p.sensitivity_vjp_full(x=np.ones(3))
    p.set_parameters([2.0, 1.5])
    assert call(p._h, cot) == -100 and b"parameters were changed" in L.slpx_last_error()
    with pytest.raises(SlpxError, match="parameters were changed"):
        p.sensitivity_vjp_full(cost=1.0)
    # batched: a null problem, and no cotangent
    rows = np.array([[2.0, 1.0]])
    it = {"x": np.array([[1.0, 0.0]]), "y": np.array([[-2.0]]), "mu": np.zeros(1)}
    args = (it["x"].ctypes.data, None, it["y"].ctypes.data, None, it["mu"].ctypes.data, rows.ctypes.data)
    assert L.slpx_problem_sensitivity_batch_vjp_full(None, 1, *args, ctypes.byref(cot), size, out.ctypes.data, None, None) == -100
    assert b"null problem" in L.slpx_last_error()
    empty = slpx.Cotangent()
    assert L.slpx_problem_sensitivity_batch_vjp_full(p._h, 1, *args, ctypes.byref(empty), size, out.ctypes.data, None, None) == -100
    assert b"no cotangent" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_batch_vjp_full(p._h, 1, *args, ctypes.byref(cot), size, out.ctypes.data, None, None) == 0
    pm.close()


# ---- 8. the Python and torch surfaces --------------------------------------------------------------------------------
def test_python_surface(fresh):
    from sleipnir_amd import optimization

    p = python_mq()
    assert p.solve() == optimization.ExitStatus.SUCCESS
    old = p.sensitivity_vjp([1.0, 2.0])
    assert bits_equal(old, p.sensitivity_vjp(optimization.Cotangent(x=[1.0, 2.0])))
    assert np.max(np.abs(p.cost_gradient() - np.array([2.0, -2.0]))) <= 1e-12 and p.sensitivity_info["factorizations"] == 0
    assert abs(p.cost_value() - 2.0) <= 1e-9  # cost* = (b - 1 - a)^2 / 2
    grad = p.sensitivity_vjp(optimization.Cotangent(y=[1.0], cost=0.5))
    assert np.max(np.abs(grad - np.array([0.0, 0.0]))) <= 1e-12  # (-1, 1) + 0.5 (2, -2)
    rows = np.array([[2.0, 1.0], [2.5, 0.5], [-1.0, 0.25]])
    r = p.solve_batch(np.zeros((3, 2)), parameters=rows, warm_start=optimization.BatchIterate())
    want = np.stack([-(rows[:, 1] - 1.0 - rows[:, 0]), rows[:, 1] - 1.0 - rows[:, 0]], axis=1)  # cost* = (b - 1 - a)^2 / 2
    got = p.cost_gradient_batch(r.iterate, rows)
    assert got.shape == (3, 2) and np.max(np.abs(got - want)) <= 1e-10 and list(p.sensitivity_status) == [0, 0, 0]
    assert np.max(np.abs(np.asarray(r.cost) - 0.5 * (rows[:, 1] - 1.0 - rows[:, 0]) ** 2)) <= 1e-9
    vx = np.ones((3, 2))
    assert bits_equal(p.sensitivity_batch_vjp(r.iterate, rows, vx), p.sensitivity_batch_vjp(r.iterate, rows, optimization.Cotangent(x=vx)))
    p.close()


def test_solve_layer_outputs(fresh):
    """backward against the closed forms of mq: x = ((a + b - 1) / 2, (b - a + 1) / 2), cost = (b - 1 - a)^2 / 2,
    y = b - 1 - a (the multiplier of f - y c_e ... dy/da = -1, dy/db = 1)"""
    import torch

    from sleipnir_amd import torch_layer

    p = python_mq()
    layer = torch_layer.SolveLayer(p, outputs=("x", "y", "cost"))
    params = torch.tensor([2.0, 1.0], dtype=torch.float64, requires_grad=True)
    out = layer(params)
    assert isinstance(out, tuple) and len(out) == 3 and all(t.dtype == torch.float64 for t in out)
    x, y, cost = out
    assert tuple(x.shape) == (2,) and tuple(y.shape) == (1,) and tuple(cost.shape) == ()
    assert abs(float(cost.detach()) - 2.0) <= 1e-9 and abs(float(y.detach()[0]) + 2.0) <= 1e-9
    wx, wy, wc = torch.tensor([1.0, 2.0], dtype=torch.float64), 3.0, 0.25
    ((wx * x).sum() + wy * y[0] + wc * cost).backward(retain_graph=True)
    dx = np.array([[0.5, -0.5], [0.5, 0.5]])  # row q = dx/dp_q
    want = dx @ wx.numpy() + wy * np.array([-1.0, 1.0]) + wc * np.array([2.0, -2.0])
    assert np.max(np.abs(params.grad.numpy() - want)) <= 1e-12, (params.grad, want)
    assert p.sensitivity_info["solves"] >= 1
    # an output nothing downstream uses contributes nothing: the loss on the cost alone
    params.grad = None
    (2.0 * cost).backward()
    assert np.max(np.abs(params.grad.numpy() - np.array([4.0, -4.0]))) <= 1e-12
    with pytest.raises(ValueError, match="outputs"):
        torch_layer.SolveLayer(p, outputs=("cost", "x"))
    with pytest.raises(ValueError, match="outputs"):
        torch_layer.SolveLayer(p, outputs=())
    p.close()


def test_default_outputs_are_a_single_tensor_with_today_s_bits(fresh):
    import torch

    from sleipnir_amd import torch_layer

    results = []
    for kwargs in ({}, {"outputs": ("x",)}):
        p = python_mq()
        layer = torch_layer.SolveLayer(p, **kwargs)
        params = torch.tensor([2.0, 1.0], dtype=torch.float64, requires_grad=True)
        xs = layer(params)
        assert isinstance(xs, torch.Tensor) and tuple(xs.shape) == (2,)
        (xs[0] + 2.0 * xs[1]).backward()
        direct = p.sensitivity_vjp([1.0, 2.0])  # what backward computed, by the old entry point
        assert bits_equal(params.grad.numpy(), direct)
        results.append((xs.detach().numpy().copy(), params.grad.numpy().copy()))
        p.close()
    assert bits_equal(results[0][0], results[1][0]) and bits_equal(results[0][1], results[1][1])


def python_boxed(lo_val=0.0, hi_val=2.0):
    from sleipnir_amd import autodiff, optimization

    p = optimization.Problem()
    x = p.decision_variable()
    x.set_value(0.5)
    lo, hi = autodiff.Variable(), autodiff.Variable()
    lo.set_value(lo_val)
    hi.set_value(hi_val)
    p.minimize((x - 3) ** 2)
    p.subject_to(x >= lo)
    p.subject_to(x <= hi)
    return p


def test_batch_solve_layer_outputs(fresh):
    """boxed rows: cost* = (hi - 3)^2 where the upper bound binds (hi < 3), 0 where it does not; an instance whose
    incoming gradient is not finite is skipped and gets a zero gradient row."""
    import torch

    from sleipnir_amd import torch_layer

    p = python_boxed()
    layer = torch_layer.BatchSolveLayer(p, outputs=("x", "cost"))
    rows = torch.tensor(sb.BOXED_ROWS[:3], dtype=torch.float64, requires_grad=True)
    x, cost = layer(rows)
    assert tuple(x.shape) == (3, 1) and tuple(cost.shape) == (3,) and list(layer.status) == [0, 0, 0]
    hi = sb.BOXED_ROWS[:3, 1]
    active = np.array(sb.BOXED_ACTIVE[:3])
    assert np.max(np.abs(cost.detach().numpy() - np.where(active, (hi - 3.0) ** 2, 0.0))) <= 1e-6
    weights = torch.tensor([1.0, 1.0, float("nan")], dtype=torch.float64)
    (x[:, 0].sum() + (weights * cost).sum()).backward()
    assert list(layer.sensitivity_status) == [0, 0, 1]
    # dx/dhi = 1 and dcost/dhi = 2 (hi - 3) where the bound binds, 0 and 0 where it does not; d/dlo = 0
    want = np.zeros((3, 2))
    want[:, 1] = np.where(active, 1.0 + 2.0 * (hi - 3.0), 0.0)
    want[2] = 0.0  # the skipped instance
    print("BatchSolveLayer boxed: grad", rows.grad.numpy(), "want", want)
    assert np.max(np.abs(rows.grad.numpy() - want)) <= 1e-6
    default = torch_layer.BatchSolveLayer(python_mq())
    xs = default(torch.tensor([[2.0, 1.0]], dtype=torch.float64, requires_grad=True))
    assert isinstance(xs, torch.Tensor) and tuple(xs.shape) == (1, 2)
    default.problem.close()
    p.close()
