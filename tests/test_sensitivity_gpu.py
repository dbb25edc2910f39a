"""Solution sensitivities on the device (include/slpx.h: solution sensitivities; sleipnir_amd/csrc/sensitivity.hpp):
slpx_problem_sensitivity, _jvp, _vjp, _rhs after whole solves.

Models: tests/support/param_models.py and sens_models.py.  What is compared with what:
  closed forms        m2, mq (derivatives that do not depend on the iterate: 1e-12), boxed (the barrier solution differs
                      from the model's by O(mu), mu of order 1e-9 at the end: 1e-6, the bound of test_warm_start_gpu.py
                      for these models' solutions), mq_scaled (scales other than 1: 1e-10)
  M                   entry by entry against central differences of the KKT residual, the iterate held fixed
  the linear algebra  every column's backward error on the downloaded lhs, ds / dz identities, jvp and vjp against the
                      Jacobian
  nothing else moved  a solve after the sensitivity calls has the bits of one without them
  end to end          dx against central differences of warm re-solves (profiles/sensitivity.txt keeps the figures)

Figures are printed (run with -s)."""
from __future__ import annotations

import numpy as np
import pytest

from sleipnir_amd import SlpxError
from tests.support import cases
from tests.support import param_models as pmod
from tests.support import sens_models as smod
from tests.test_configs_gpu import backward_error

pytestmark = pytest.mark.gpu

SUCCESS = 0


@pytest.fixture
def m(fresh):
    mm = pmod.new_model()
    mm.be.reset()
    return mm


def chain_case(m, stages, row):
    return pmod.chain(m, stages, pmod.chain_rows(stages, 2)[row])


CHAINS = {
    "chain4 row 0": lambda m: chain_case(m, 4, 0),  # u_max = 0.3: bounds bind
    "chain4 row 1": lambda m: chain_case(m, 4, 1),  # u_max = 2.0
    "chain8 row 0": lambda m: chain_case(m, 8, 0),  # the family-generated body
}


def solved(pm, **kw):
    status, rep = pm.p.p.solve(**kw)
    assert status == SUCCESS, status
    return rep


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def parameter_values(pm):
    return np.array([pm.p.be.value(node) for node in pm.param_ids])


# ---- 2. closed forms, scales of 1 ------------------------------------------------------------------------------------
def test_closed_form_newton(m):
    pm = pmod.m2(m, (2.0,))
    solved(pm)
    r = pm.p.p.sensitivity()
    print("m2 dx/da", r["dx"], r["info"])
    assert r["dx"].shape == (1, 2) and r["ds"].shape == (1, 0) and r["dy"].shape == (1, 0) and r["dz"].shape == (1, 0)
    assert np.max(np.abs(r["dx"] - np.array([[1.0, 0.0]]))) <= 1e-12
    assert r["info"]["n_p"] == 1 and r["info"]["solve_status"] == SUCCESS and r["info"]["n_neg"] == 0 and r["info"]["n_zero"] == 0
    pm.close()


def test_closed_form_sqp(m):
    pm = pmod.mq(m, (2.0, 1.0))
    solved(pm)
    r = pm.p.p.sensitivity()
    print("mq dx", r["dx"], "dy", r["dy"], r["info"])
    assert np.max(np.abs(r["dx"] - np.array([[0.5, -0.5], [0.5, 0.5]]))) <= 1e-12
    assert np.max(np.abs(r["dy"] - np.array([[-1.0], [1.0]]))) <= 1e-12
    assert r["info"]["n_neg"] == 1 and r["info"]["n_zero"] == 0 and r["info"]["solves"] >= 2
    pm.close()


# ---- 3. closed forms, interior point ---------------------------------------------------------------------------------
def test_closed_form_interior_point_active_bound(m):
    """min (x - 3)^2, lo <= x <= hi with (lo, hi) = (0, 2): x = hi, z_hi = 2 (3 - hi); rows: x - lo, hi - x"""
    pm = pmod.boxed(m, (0.0, 2.0))
    solved(pm)
    r = pm.p.p.sensitivity()
    print("boxed (0, 2): dx", r["dx"].ravel(), "ds", r["ds"], "dz", r["dz"], r["info"])
    lo, hi = 0, 1
    assert abs(r["dx"][hi, 0] - 1.0) <= 1e-6 and abs(r["dx"][lo, 0]) <= 1e-6
    assert abs(r["dz"][hi, 1] + 2.0) <= 1e-6
    assert abs(r["ds"][hi, 0] - 1.0) <= 1e-6 and abs(r["ds"][lo, 0] + 1.0) <= 1e-6
    assert abs(r["ds"][hi, 1]) <= 1e-6 and abs(r["ds"][lo, 1]) <= 1e-6
    assert r["info"]["n_neg"] == 0 and r["info"]["n_zero"] == 0
    pm.close()


def test_closed_form_interior_point_nothing_active(m):
    pm = pmod.boxed(m, (0.0, 5.0))
    solved(pm)
    r = pm.p.p.sensitivity()
    print("boxed (0, 5): dx", r["dx"].ravel())
    assert np.max(np.abs(r["dx"])) <= 1e-6
    pm.close()


# ---- 4. units --------------------------------------------------------------------------------------------------------
def test_units(m):
    """mq with the cost times 1000 and the row times 500: the solve runs on scales other than 1 (seen through the scaled
    and the user's multiplier), the sensitivities are those of the model as written: lambda_u = 2 (b - 1 - a)."""
    pm = smod.mq_scaled(m, (2.0, 1.0))
    solved(pm)
    p = pm.p.p
    y_scaled, y_user = p.duals()[1], p.iterate()[2]
    print("mq_scaled: y scaled", y_scaled, "user", y_user, "ratio d_ce / d_f", y_user / y_scaled)
    assert abs(y_user[0] - 2.0 * (1.0 - 1.0 - 2.0)) <= 1e-6
    # y_u = y d_ce / d_f with d_f = 100 / 4000 and d_ce = 100 / 500 at x0 = 0: the scales the solve used are not 1
    assert abs(y_user[0] / y_scaled[0] - (100.0 / 500.0) / (100.0 / 4000.0)) <= 1e-9
    r = p.sensitivity()
    print("mq_scaled dx", r["dx"], "dy", r["dy"], r["info"])
    assert np.max(np.abs(r["dx"] - np.array([[0.5, -0.5], [0.5, 0.5]]))) <= 1e-10
    assert np.max(np.abs(r["dy"] - np.array([[-2.0], [2.0]]))) <= 1e-10
    pm.close()


# ---- 5. M against central differences of the residual ----------------------------------------------------------------
def kkt_residual(sysm, dims, x, s, y, z, params):
    """F = [g - A_e^T y - A_i^T z; c_e; c_i] from a full sweep of `sysm` (unit scaling installed by the caller) with
    `params` installed; and V."""
    n, me, mi = dims
    sysm.set_parameters(params)
    sysm.set_state(x=x, s=s, y=y, z=z)
    sysm.sweep(True)
    V = sysm.get("V")[0].copy()
    I = sysm.info
    F = np.zeros(n + me + mi)
    gcp, _ = sysm.pattern(0)
    for c in range(n):
        for t in range(gcp[c], gcp[c + 1]):
            F[c] += V[I["off_g"] + t]
    for which, off, mult in ((1, I["off_Ae"], y), (2, I["off_Ai"], z)):
        cp, ri = sysm.pattern(which)
        cols = np.repeat(np.arange(n), np.diff(cp))
        np.subtract.at(F, cols, V[off:off + len(ri)] * mult[ri])
    F[n:n + me] = V[1:1 + me]
    F[n + me:] = V[1 + me:1 + me + mi]
    return F, V


@pytest.mark.parametrize("case", list(CHAINS))
def test_unreduced_rhs_against_central_differences(m, case):
    pm = CHAINS[case](m)
    p = pm.p.p
    solved(pm)
    dims = p.dims
    x, s, y, z, mu = p.iterate()
    M = p.sensitivity_rhs()
    params = parameter_values(pm)
    assert M.shape == (len(params), sum(dims))
    sysm = p.system()
    sysm.set_scaling(np.ones(1 + dims[1] + dims[2]))
    FD = np.zeros_like(M)
    for q in range(len(params)):
        h = 1e-5 * max(1.0, abs(params[q]))
        up, dn = params.copy(), params.copy()
        up[q] += h
        dn[q] -= h
        FD[q] = (kkt_residual(sysm, dims, x, s, y, z, up)[0] - kkt_residual(sysm, dims, x, s, y, z, dn)[0]) / (2.0 * h)
    sysm.set_parameters(params)  # (as they were)
    err = float(np.max(np.abs(M - FD)))
    nz = np.abs(M[M != 0.0])
    print(f"{case}: |M - FD| {err:.3e}, max |M| {np.max(np.abs(M)):.3e}, smallest structural |M| {nz.min():.3e}, non-zeros {nz.size}")
    assert err <= 1e-7 * max(1.0, float(np.max(np.abs(M))))
    assert (np.abs(FD) > 1e-6).sum() == (np.abs(M) > 1e-6).sum()  # nothing missing, nothing extra
    pm.close()


# ---- 6. the linear algebra -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mq"] + list(CHAINS))
def test_linear_algebra(m, case):
    pm = pmod.mq(m, (2.0, 1.0)) if case == "mq" else CHAINS[case](m)
    p = pm.p.p
    solved(pm)
    n, me, mi = dims = p.dims
    x, s, y, z, mu = p.iterate()
    n_p = len(pm.params)
    first = p.sensitivity()
    again = p.sensitivity()
    i1, i2 = first["info"], again["info"]
    print(case, i1)
    assert i1["n_neg"] == me and i1["n_zero"] == 0 and i1["n_pos"] == n and i1["solve_status"] == SUCCESS
    assert i1["factorizations"] >= 1 and i2["factorizations"] == 0 and i1["t_compile"] > 0.0 and i2["t_compile"] == 0.0
    assert i1["solves"] >= n_p and i1["n_p"] == n_p
    for k in ("dx", "ds", "dy", "dz"):
        assert bits_equal(first[k], again[k]), k
    rng = np.random.default_rng(5)
    dp, v = rng.uniform(-1.0, 1.0, n_p), rng.uniform(-1.0, 1.0, n)
    jvp = p.sensitivity_jvp(dp)
    grad, vinfo = p.sensitivity_vjp(v)
    assert jvp["info"]["factorizations"] == 0 and vinfo["factorizations"] == 0
    assert jvp["info"]["solves"] >= 1 and vinfo["solves"] >= 1
    M = p.sensitivity_rhs()
    # the system that was factored, and A_i at the iterate (unit scales, the user's units)
    sysm = p.system()
    lhs = sysm.get("lhs")[0].copy()
    cp, ri = sysm.pattern(5)
    sysm.set_scaling(np.ones(1 + me + mi))
    V = kkt_residual(sysm, dims, x, s, y, z, parameter_values(pm))[1]
    acp, ari = sysm.pattern(2)
    off_Ai = sysm.info["off_Ai"]
    Ai = np.zeros((mi, n))
    for c in range(n):
        for t in range(acp[c], acp[c + 1]):
            Ai[ari[t], c] = V[off_Ai + t]
    sigma = z / s
    r_x, r_e, r_i = M[:, :n], M[:, n:n + me], M[:, n + me:]
    R = np.hstack([-r_x - (r_i * sigma) @ Ai, -r_e])
    worst = 0.0
    for q in range(n_p):
        sol = np.concatenate([first["dx"][q], -first["dy"][q]])
        worst = max(worst, backward_error(cp, ri, lhs, n, i1["delta"], i1["gamma"], sol, R[q]))
        ds = Ai @ first["dx"][q] + r_i[q]
        assert cases.max_rel(first["ds"][q], ds) <= 1e-12
        assert cases.max_rel(first["dz"][q], -sigma * first["ds"][q]) <= 1e-12
    tol = 1e-12 if case == "mq" else 1e-6
    rel = lambda got, want: float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), 1e-300)
    e_jvp = max(rel(jvp[k], dp @ first[k]) for k in ("dx", "ds", "dy", "dz") if first[k].size)
    e_vjp = rel(grad, first["dx"] @ v)
    print(f"{case}: backward error {worst:.3e} (delta {i1['delta']:.1e} gamma {i1['gamma']:.1e} berr_max {i1['berr_max']:.1e}); "
          f"jvp against the Jacobian {e_jvp:.3e}, vjp {e_vjp:.3e}")
    assert worst <= 1e-10
    assert e_jvp <= tol and e_vjp <= tol
    pm.close()


# ---- 7. nothing else moved -------------------------------------------------------------------------------------------
BUILD7 = {
    "mq": lambda m: pmod.mq(m, (2.0, 1.0)),
    "boxed": lambda m: pmod.boxed(m, (0.0, 1.0)),
    "chain4": lambda m: chain_case(m, 4, 0),
}


@pytest.mark.parametrize("case", list(BUILD7))
def test_a_following_solve_is_not_affected(m, case):
    with_calls, without = BUILD7[case](m), BUILD7[case](m)
    results = []
    for pm, call in ((with_calls, True), (without, False)):
        p = pm.p.p
        x0 = p.get_x()
        solved(pm)
        if call:
            compiles = p.compile_count()
            n_p = len(pm.params)
            p.sensitivity()
            p.sensitivity_jvp(np.linspace(-1.0, 1.0, n_p))
            p.sensitivity_vjp(np.linspace(1.0, 2.0, p.dims[0]))
            assert p.compile_count() == compiles
        p.set_x(x0)
        status, rep = p.solve()
        results.append((status, rep["iterations"], p.get_x(), *p.duals(), *p.iterate()))
    a, b = results
    assert a[0] == b[0] == SUCCESS and a[1] == b[1], (a[:2], b[:2])
    for u, v in zip(a[2:], b[2:]):
        assert bits_equal(u, v)
    with_calls.close()
    without.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------
def test_errors(m, slpx):
    from tests.support import model

    L = slpx.lib()
    pm = pmod.mq(m, (2.0, 1.0))
    p = pm.p.p
    out = np.zeros(8)
    for call in (lambda: L.slpx_problem_sensitivity(p._h, out.ctypes.data, None, None, None, None),
                 lambda: L.slpx_problem_sensitivity_jvp(p._h, out.ctypes.data, out.ctypes.data, None, None, None, None),
                 lambda: L.slpx_problem_sensitivity_vjp(p._h, out.ctypes.data, out.ctypes.data, None),
                 lambda: L.slpx_problem_sensitivity_rhs(p._h, None)):
        assert call() == -100 and b"has not been solved" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity(None, None, None, None, None, None) == -100 and b"null problem" in L.slpx_last_error()
    solved(pm)
    assert L.slpx_problem_sensitivity(p._h, None, None, None, None, None) == 0  # (every output may be NULL)
    with pytest.raises(SlpxError, match="dp must have 2 entries"):
        p.sensitivity_jvp(np.ones(3))
    assert L.slpx_problem_sensitivity_jvp(p._h, None, out.ctypes.data, None, None, None, None) == -100
    assert b"dp is null" in L.slpx_last_error()
    p.set_parameters([2.0, 1.5])
    assert L.slpx_problem_sensitivity(p._h, out.ctypes.data, None, None, None, None) == -100
    assert b"parameters were changed" in L.slpx_last_error()
    with pytest.raises(SlpxError, match="parameters were changed"):
        p.sensitivity_vjp(np.ones(2))
    solved(pm)
    assert np.max(np.abs(p.sensitivity()["dx"] - np.array([[0.5, -0.5], [0.5, 0.5]]))) <= 1e-12
    pm.close()
    q = model.NlpProblem(m)
    x = q.decision_variable(1.0)
    q.minimize(m.pow(x - 2, 2))
    status, _ = q.p.solve()
    assert status == SUCCESS
    assert L.slpx_problem_sensitivity(q.p._h, out.ctypes.data, None, None, None, None) == -100
    assert b"reaches no parameter" in L.slpx_last_error()
    q.p.close()


# ---- 9. end to end ---------------------------------------------------------------------------------------------------
# Largest disagreement of a qualifying column of dx with central differences of warm re-solves at p +- 1e-4 (tolerance
# 1e-10), relative to the column's largest entry, as measured on the MI355X (profiles/sensitivity.txt); the test asserts
# ten times the figure and never more than CAP.
MEASURED = {"chain4 row 0": 2.048e-08, "chain4 row 1": 5.408e-09}
CAP = 1e-3
# What central differences of re-solves can resolve: each re-solve's x is good to about its tolerance, 1e-10, and the
# difference is divided by 2 h = 2e-4.  A column whose every entry lies below that (row 0: every input sits on its
# bound, so the references r_k move nothing — dx/dr_k is O(mu)) has no "largest entry" to be relative to: it is compared
# absolutely, |dx - fd| <= RESOLUTION, and does not enter the relative figure.
RESOLUTION = 1e-10 / 1e-4


def binding_set(c_i_slack, z):
    """the rows whose multiplier dominates their slack: z_j s_j = mu splits into z_j > s_j (binding) and z_j < s_j"""
    return tuple(np.asarray(z) > np.asarray(c_i_slack))


@pytest.mark.parametrize("case", ["chain4 row 0", "chain4 row 1"])
def test_end_to_end_against_central_differences_of_re_solves(m, case):
    pm = CHAINS[case](m)
    p = pm.p.p
    status, _ = p.solve(tolerance=1e-10)
    assert status == SUCCESS
    x, s, y, z, mu = p.iterate()
    params = parameter_values(pm)
    dx = p.sensitivity()["dx"]
    base_set = binding_set(s, z)
    h = 1e-4
    worst, qualifying = 0.0, 0
    for q in range(len(params)):
        ends = []
        for sign in (+1.0, -1.0):
            row = params.copy()
            row[q] += sign * h
            p.set_parameters(row)
            p.set_x(x)
            st, _ = p.solve(tolerance=1e-10, warm_start=dict(s=s, y=y, z=z, mu=mu))
            it = p.iterate()
            ends.append((st, it[0], binding_set(it[1], it[3])))
        if any(e[0] != SUCCESS for e in ends) or any(e[2] != base_set for e in ends):
            print(f"{case}: column {q} does not qualify (status {[e[0] for e in ends]}, binding set kept {[e[2] == base_set for e in ends]})")
            continue
        qualifying += 1
        fd = (ends[0][1] - ends[1][1]) / (2.0 * h)
        largest, diff = float(max(np.max(np.abs(dx[q])), np.max(np.abs(fd)))), float(np.max(np.abs(dx[q] - fd)))
        if largest < RESOLUTION:
            print(f"{case}: column {q} is zero to what the differences resolve: largest entry {largest:.3e}, |dx - fd| {diff:.3e}")
            assert diff <= RESOLUTION
            continue
        rel = diff / largest
        print(f"{case}: column {q} disagreement {rel:.3e} of its largest entry {largest:.3e}")
        worst = max(worst, rel)
    p.set_parameters(params)
    print(f"{case}: {qualifying} of {len(params)} columns qualify, largest disagreement {worst:.3e}, binding rows {sum(base_set)}")
    assert 4 * qualifying >= 3 * len(params)
    bound = min(CAP, 10.0 * MEASURED[case])
    assert worst <= bound, (worst, bound)
    pm.close()


# ---- 10. the Python and torch surfaces -------------------------------------------------------------------------------
def python_mq(a_val=2.0, b_val=1.0):
    from sleipnir_amd import autodiff, optimization

    p = optimization.Problem()
    x, y = p.decision_variable(), p.decision_variable()
    a, b = autodiff.Variable(), autodiff.Variable()
    a.set_value(a_val)
    b.set_value(b_val)
    p.minimize((x - a) ** 2 + (y - 1) ** 2)
    p.subject_to(x + y == b)
    return p


def test_python_surface(fresh):
    from sleipnir_amd import optimization

    p = python_mq()
    assert p.solve() == optimization.ExitStatus.SUCCESS
    r = p.sensitivity()
    assert isinstance(r, optimization.Sensitivity)
    assert r.dx.shape == (2, 2) and r.dy.shape == (2, 1) and r.ds.shape == (2, 0) and r.dz.shape == (2, 0)
    assert np.max(np.abs(r.dx - np.array([[0.5, -0.5], [0.5, 0.5]]))) <= 1e-12
    assert np.max(np.abs(r.dy - np.array([[-1.0], [1.0]]))) <= 1e-12
    assert r.info["solve_status"] == 0 and r.info["n_neg"] == 1
    grad = p.sensitivity_vjp([1.0, 2.0])
    assert isinstance(grad, np.ndarray) and grad.shape == (2,) and np.max(np.abs(grad - np.array([-0.5, 1.5]))) <= 1e-12
    dp = np.array([0.02, 0.01])
    d = p.sensitivity_jvp(dp)
    assert isinstance(d, optimization.Iterate) and d.mu == 0.0 and p.sensitivity_info["factorizations"] == 0
    it = p.iterate() + d
    p.set_parameters(np.array([2.0, 1.0]) + dp)
    assert p.solve(warm_start=it) == optimization.ExitStatus.SUCCESS
    assert p.warm_start_repaired() == 0
    # (the model is quadratic with a linear row: the tangent lands on the new solution)
    assert p.report["iterations"] <= 1
    a, b = 2.02, 1.01
    assert np.max(np.abs(p.iterate().x - np.array([(a + b - 1) / 2, (b - a + 1) / 2]))) <= 1e-9
    p.close()


def test_torch_layer(fresh):
    import torch

    from sleipnir_amd import torch_layer

    p = python_mq()
    layer = torch_layer.SolveLayer(p)
    params = torch.tensor([2.0, 1.0], dtype=torch.float64, requires_grad=True)
    xs = layer(params)
    assert layer.status == 0 and xs.dtype == torch.float64 and tuple(xs.shape) == (2,)
    assert torch.max(torch.abs(xs.detach() - torch.tensor([1.0, 0.0], dtype=torch.float64))) <= 1e-9
    (xs[0] + 2.0 * xs[1]).backward(retain_graph=True)
    assert torch.max(torch.abs(params.grad - torch.tensor([-0.5, 1.5], dtype=torch.float64))) <= 1e-12
    # a second forward: other values, warm from the first iterate
    params2 = torch.tensor([2.5, 0.5], dtype=torch.float64, requires_grad=True)
    xs2 = layer(params2)
    assert layer.status == 0 and layer.solves == 2
    assert torch.max(torch.abs(xs2.detach() - torch.tensor([1.0, -0.5], dtype=torch.float64))) <= 1e-9
    (3.0 * xs2[0]).backward()
    assert torch.max(torch.abs(params2.grad - torch.tensor([1.5, 1.5], dtype=torch.float64))) <= 1e-12
    with pytest.raises(RuntimeError, match="not the layer's last"):
        (xs[0] * 1.0).backward()
    p.close()
