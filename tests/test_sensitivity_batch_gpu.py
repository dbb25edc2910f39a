"""Batched solution sensitivities on the device (include/slpx.h: batched sensitivities; csrc/sensitivity.hpp:
BatchSensitivity): slpx_problem_sensitivity_batch, _jvp, _vjp, _rhs — B iterates, instance b with respect to its own
parameter row.

Models and rows: tests/support/sens_batch_models.py (m2, mq, boxed, chain(4), chain(8) of param_models.py with five rows
each; chain(51), the smallest chain with dimM = 5 stages + 2 > 256, with three).  Batch sizes 1, 3 and 5.  What is
compared with what:
  1  the single-problem path at the same iterate (set_parameters, solve, iterate, sensitivity*), and the closed forms
  2  the linear algebra per instance on the batch-1 system's lhs at that instance's iterate and row
  3  the same call with the instances permuted: equal bits per instance
  4  a bad instance in the middle: status 1, NaN rows, the others' bits as without it
  5  the kept factorization; a following solve_batch and a kept single-problem factorization are not affected
  6  end to end against central differences of re-solved batches
  7  errors, shapes, optimization.Problem, BatchSolveLayer
Two cases beyond the issue's table: mq at B = 64, where the batch system takes the paths of a large batch, and
chain(85) at B = 3, the smallest chain with n + m_e > 256, where the lanes of the vjp's dot product take a second row.

MEASURED (MI355X, profiles/sensitivity_batch.txt): the largest relative difference between the batched and the
single-problem Jacobian, jvp and vjp per case — the two paths factor with different kernel families, so they agree to
conditioning times rounding — and of test 6.  The tests assert ten times the figure, never more than CAP, and never
less than FLOOR (1000 ulp: a figure of 0 says that both paths ran the same kernels, which the batch system of another
size need not do).  At B = 1 both paths run the same stages on systems of one instance: there test 1 asserts equal
bits as well (profiles/sensitivity_stages.txt).

Figures are printed (run with -s)."""
from __future__ import annotations

import numpy as np
import pytest

from sleipnir_amd import SlpxError
from tests.support import cases
from tests.support import sens_batch_models as sb
from tests.test_configs_gpu import backward_error
from tests.test_sensitivity_gpu import binding_set, bits_equal, kkt_residual

pytestmark = pytest.mark.gpu

SUCCESS = 0
CAP = 1e-6
FLOOR = 1000 * 2.0 ** -53
MEASURED = {"m2": 0.0, "mq": 0.0, "boxed": 0.0, "chain4": 3.417e-21, "chain8": 4.779e-08, "chain51": 2.825e-15, "chain85": 4.466e-16}
# Test 6 runs rows 0, 1 and 3 of chain_rows(4, 5); per instance 8.483e-09, 9.741e-10 and 3.911e-08, the order of the
# single-problem test's 2.0e-8 and 5.4e-9 on rows 0 and 1.  Row 2 is left out on purpose: there the tangent and the
# central difference differ by 2.7e-4 at every h from 1e-3 to 1e-6, and that is the regularization of the policy both
# paths share, not the batch — the factorization of that iterate takes delta = 1e-4 (so do rows 0, 3 and 4), row 2 is
# the only one of them with inputs off their bounds, and a dense host solve of its KKT system agrees with the central
# difference to 7.6e-8 without delta and differs by the same 2.732e-4 with it, while the batched jvp has the bits of
# the host solve WITH delta to 5e-16 (profiles/sensitivity_batch.txt, section 3).
E2E_ROWS = [0, 1, 3]
MEASURED_END_TO_END = (8.483e-09, 9.741e-10, 3.911e-08)  # each instance is held to ten times ITS figure
CAP_END_TO_END = 1e-3  # (the cap of the single-problem end-to-end test)
RESOLUTION = 1e-10 / 1e-4  # what central differences of re-solves at tolerance 1e-10 and h = 1e-4 resolve

OUT = ("dx", "ds", "dy", "dz")


@pytest.fixture
def m(fresh):
    from tests.support import param_models as pmod

    mm = pmod.new_model()
    mm.be.reset()
    return mm


def rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), 1e-300)


def bound_for(case):
    return min(CAP, max(10.0 * MEASURED[case], FLOOR))


def batch_calls(p, it, rows, dp, v):
    """the four batched calls on one set of rows: (rhs, jacobian, jvp, vjp)"""
    return (p.sensitivity_batch_rhs(it, rows), p.sensitivity_batch(it, rows), p.sensitivity_batch_jvp(it, rows, dp),
            p.sensitivity_batch_vjp(it, rows, v))


def instance_bits(calls, b):
    """everything the calls say about instance b, as a list of arrays"""
    rhs, jac, jvp, vjp = calls
    out = [rhs["M"][b], vjp["grad"][b]] + [jac[k][b] for k in OUT] + [jvp[k][b] for k in OUT]
    for r in (jac, jvp, vjp):
        i = r["info"][b]
        out.append(np.array([i["delta"], i["gamma"], i["n_pos"], i["n_neg"], i["n_zero"]], dtype=np.float64))
    return out


# ---- 1. against the single-problem path at the same iterate ----------------------------------------------------------
# (the long chains have three rows: a batch of five takes them over and over, like mq at B = 64.  chain85 — n + m_e = 257,
# the lanes of the vjp's dot product take a second row — is a case beyond the issue's table, like mq at B = 64.)
ALL = [(case, B) for case in ("m2", "mq", "boxed", "chain4", "chain8", "chain51") for B in (1, 3, 5)] + [("chain85", 3), ("mq", 64)]


@pytest.mark.parametrize("case,B", ALL, ids=[f"{c}-B{B}" for c, B in ALL])
def test_against_the_single_problem_path(m, case, B):
    ref = sb.reference(m, case)
    count = ref["rows"].shape[0]
    idx = [b % count for b in range(B)]  # (B = 64: the rows over and over)
    pm, _ = sb.build(m, case)
    p = pm.p.p
    it, rows, dp, v = sb.iterate_rows(ref, idx), ref["rows"][idx], ref["dp"][idx], ref["v"][idx]
    rhs, jac, jvp, vjp = batch_calls(p, it, rows, dp, v)
    n, me, mi = p.dims
    n_p = rows.shape[1]
    assert rhs["M"].shape == (B, n_p, n + me + mi) and jac["dx"].shape == (B, n_p, n) and jac["ds"].shape == (B, n_p, mi)
    assert jac["dy"].shape == (B, n_p, me) and jvp["dx"].shape == (B, n) and vjp["grad"].shape == (B, n_p)
    worst = 0.0
    for r in (rhs, jac, jvp, vjp):
        assert np.array_equal(r["status"], np.zeros(B, dtype=np.int32)), r["status"]
    for b, src in enumerate(idx):
        M = ref["M"][src]
        assert np.max(np.abs(rhs["M"][b] - M)) <= 1e-12 * max(1.0, float(np.max(np.abs(M)))), (case, b)
        assert np.array_equal(rhs["M"][b] != 0.0, M != 0.0), (case, b)
        worst = max([worst, rel(vjp["grad"][b], ref["grad"][src])] + [rel(jac[k][b], ref[k][src]) for k in OUT] +
                    [rel(jvp[k][b], ref["j" + k][src]) for k in OUT])
        # (the inertia of a computed instance is what the policy accepts, (n, m_e, 0), reported as such and not read back
        # from the counters: with status 0 this holds by construction, here and in tests 2 and 3 — what it checks is that
        # no instance reports a factorization the policy did not accept)
        info = jac["info"][b]
        assert (info["n_pos"], info["n_neg"], info["n_zero"]) == (n, me, 0) and info["n_p"] == n_p and info["solve_status"] == 0
        assert info["solves"] >= n_p, info
    print(f"{case} B={B}: batched against single-problem, largest relative difference {worst:.3e} (bound {bound_for(case):.3e})")
    assert worst <= bound_for(case), (worst, bound_for(case))
    if B == 1:
        # the batch system of one instance and the problem's own system run the same stages and the same kernel families:
        # the same bits, not only the measured bound (profiles/sensitivity_stages.txt)
        assert bits_equal(vjp["grad"][0], ref["grad"][idx[0]]), case
        for k in OUT:
            assert bits_equal(jac[k][0], ref[k][idx[0]]) and bits_equal(jvp[k][0], ref["j" + k][idx[0]]), (case, k)
    # closed forms, per instance with different rows in one batch
    if case == "m2":
        assert np.max(np.abs(jac["dx"] - np.array([[1.0, 0.0]]))) <= 1e-12
    if case == "mq":
        assert np.max(np.abs(jac["dx"] - np.array([[0.5, -0.5], [0.5, 0.5]]))) <= 1e-12
        assert np.max(np.abs(jac["dy"] - np.array([[-1.0], [1.0]]))) <= 1e-12
        want = np.array([[0.5 * da + 0.5 * db, -0.5 * da + 0.5 * db] for da, db in dp])
        assert np.max(np.abs(jvp["dx"] - want)) <= 1e-12
    if case == "boxed":
        lo, hi = 0, 1
        for b, src in enumerate(idx):
            if sb.BOXED_ACTIVE[src]:  # x = hi, z_hi = 2 (3 - hi)
                assert abs(jac["dx"][b, hi, 0] - 1.0) <= 1e-6 and abs(jac["dx"][b, lo, 0]) <= 1e-6
                assert abs(jac["dz"][b, hi, 1] + 2.0) <= 1e-6
                assert abs(jac["ds"][b, hi, 0] - 1.0) <= 1e-6 and abs(jac["ds"][b, lo, 0] + 1.0) <= 1e-6
            else:
                assert np.max(np.abs(jac["dx"][b])) <= 1e-6
    pm.close()


# ---- 2. the linear algebra per instance, independent of the single path ----------------------------------------------
@pytest.mark.parametrize("case", ["mq", "chain4", "chain8"])
def test_linear_algebra_per_instance(m, case):
    B = 5
    ref = sb.reference(m, case)
    pm, rows = sb.build(m, case)
    p = pm.p.p
    it = sb.iterate_rows(ref, range(B))
    rhs, jac, jvp, vjp = batch_calls(p, it, rows, ref["dp"], ref["v"])
    n, me, mi = dims = p.dims
    n_p = rows.shape[1]
    sysm = p.system()
    cp, ri = sysm.pattern(5)
    sysm.set_scaling(np.ones(1 + me + mi))
    acp, ari = sysm.pattern(2)
    off_Ai = sysm.info["off_Ai"]
    tol = 1e-12 if case == "mq" else 1e-6
    worst = e_jvp = e_vjp = 0.0
    for b in range(B):
        x, s, y, z = (it[k][b] for k in ("x", "s", "y", "z"))
        V = kkt_residual(sysm, dims, x, s, y, z, rows[b])[1]  # (installs row b and the iterate, sweeps)
        sysm.assemble()
        lhs = sysm.get("lhs")[0].copy()
        Ai = np.zeros((mi, n))
        for c in range(n):
            for t in range(acp[c], acp[c + 1]):
                Ai[ari[t], c] = V[off_Ai + t]
        sigma = z / s
        M = rhs["M"][b]
        r_x, r_e, r_i = M[:, :n], M[:, n:n + me], M[:, n + me:]
        R = np.hstack([-r_x - (r_i * sigma) @ Ai, -r_e])
        info = jac["info"][b]
        assert (info["n_pos"], info["n_neg"], info["n_zero"]) == (n, me, 0), info
        for q in range(n_p):
            sol = np.concatenate([jac["dx"][b, q], -jac["dy"][b, q]])
            worst = max(worst, backward_error(cp, ri, lhs, n, info["delta"], info["gamma"], sol, R[q]))
            assert cases.max_rel(jac["ds"][b, q], Ai @ jac["dx"][b, q] + r_i[q]) <= 1e-12
            assert cases.max_rel(jac["dz"][b, q], -sigma * jac["ds"][b, q]) <= 1e-12
        e_jvp = max([e_jvp] + [rel(jvp[k][b], ref["dp"][b] @ jac[k][b]) for k in OUT if jac[k][b].size])
        e_vjp = max(e_vjp, rel(vjp["grad"][b], jac["dx"][b] @ ref["v"][b]))
    print(f"{case}: per-instance backward error {worst:.3e}; jvp against the Jacobian {e_jvp:.3e}, vjp {e_vjp:.3e}")
    assert worst <= 1e-10
    assert e_jvp <= tol and e_vjp <= tol
    pm.close()


# ---- 3. no cross-talk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chain4", "chain8"])
def test_permuted_instances_keep_their_bits(m, case):
    ref = sb.reference(m, case)
    pm, rows = sb.build(m, case)
    p = pm.p.p
    order = [3, 0, 4, 1, 2]
    straight = batch_calls(p, sb.iterate_rows(ref, range(5)), rows, ref["dp"], ref["v"])
    permuted = batch_calls(p, sb.iterate_rows(ref, order), rows[order], ref["dp"][order], ref["v"][order])
    for pos, b in enumerate(order):
        for u, w in zip(instance_bits(straight, b), instance_bits(permuted, pos)):
            assert bits_equal(u, w), (case, b, pos)
    pm.close()


# ---- 4. a bad instance in the middle ---------------------------------------------------------------------------------
def spoil_x(it, rows, dp, v):
    it["x"][2, 0] = np.nan


def spoil_s(it, rows, dp, v):
    it["s"][2, 0] = 0.0


def spoil_row(it, rows, dp, v):
    rows[2, -1] = np.inf


def spoil_direction(it, rows, dp, v):
    dp[2, 0] = np.nan
    v[2, 0] = np.inf


@pytest.mark.parametrize("spoil", [spoil_x, spoil_s, spoil_row, spoil_direction], ids=lambda f: f.__name__)
@pytest.mark.parametrize("case", ["boxed", "chain4"])
def test_a_bad_instance_in_the_middle(m, case, spoil):
    ref = sb.reference(m, case)
    pm, rows = sb.build(m, case)
    p = pm.p.p
    it, dp, v = sb.iterate_rows(ref, range(5)), np.array(ref["dp"]), np.array(ref["v"])
    healthy = batch_calls(p, it, rows, dp, v)
    spoil(it, rows, dp, v)
    bad = batch_calls(p, it, rows, dp, v)
    for r, name in zip(bad, ("rhs", "jacobian", "jvp", "vjp")):
        if spoil is spoil_direction and name in ("rhs", "jacobian"):  # (these two take neither dp nor vx)
            assert list(r["status"]) == [0, 0, 0, 0, 0], (name, r["status"])
            continue
        assert list(r["status"]) == [0, 0, 1, 0, 0], (name, r["status"])
        for k in ("M", "grad") + OUT:
            if k in r and r[k][2].size:
                assert np.all(np.isnan(r[k][2])), (name, k)
    for b in (0, 1, 3, 4):
        for u, w in zip(instance_bits(healthy, b), instance_bits(bad, b)):
            assert bits_equal(u, w), (case, spoil.__name__, b)
    pm.close()


# ---- 5. kept factorization and nothing else moved --------------------------------------------------------------------
def test_kept_factorization(m):
    ref = sb.reference(m, "chain4")
    pm, rows = sb.build(m, "chain4")
    twin, _ = sb.build(m, "chain4")
    p = pm.p.p
    it = sb.iterate_rows(ref, range(5))
    jac = p.sensitivity_batch(it, rows)
    vjp = p.sensitivity_batch_vjp(it, rows, ref["v"])
    fresh = twin.p.p.sensitivity_batch_vjp(it, rows, ref["v"])
    assert all(i["factorizations"] >= 1 and i["t_compile"] > 0.0 for i in jac["info"])
    assert all(i["factorizations"] == 0 and i["t_compile"] == 0.0 and i["solves"] >= 1 for i in vjp["info"])
    assert all(i["factorizations"] >= 1 for i in fresh["info"])
    assert bits_equal(vjp["grad"], fresh["grad"])
    moved = rows.copy()
    moved[3, 2] = np.nextafter(moved[3, 2], np.inf)  # one bit of one row
    again = p.sensitivity_batch_vjp(it, moved, ref["v"])
    assert all(i["factorizations"] >= 1 for i in again["info"])
    pm.close()
    twin.close()


def test_the_batch_system_s_other_users_drop_the_kept_factorization(m):
    """solve_batch and restoration_steps_batch of the same B run on the batch system the factorization lives in: the
    same vjp on the same rows afterwards factors again, and has the same bits."""
    ref = sb.reference(m, "chain4")
    pm, rows = sb.build(m, "chain4")
    p = pm.p.p
    it = sb.iterate_rows(ref, range(5))
    vjp = lambda: p.sensitivity_batch_vjp(it, rows, ref["v"])
    first, kept = vjp(), vjp()
    assert all(i["factorizations"] >= 1 for i in first["info"]) and all(i["factorizations"] == 0 for i in kept["info"])
    x0 = np.repeat(p.get_x()[None, :], 5, axis=0)
    assert list(p.solve_batch(x0, parameters=rows, warm_start={})["status"]) == [SUCCESS] * 5
    after_solve, kept = vjp(), vjp()
    assert all(i["factorizations"] >= 1 for i in after_solve["info"]) and all(i["factorizations"] == 0 for i in kept["info"])
    p.restoration_steps_batch(it["x"], it["s"], it["y"], it["z"], it["mu"], 1)
    after_restoration = vjp()
    assert all(i["factorizations"] >= 1 for i in after_restoration["info"])
    # a batch of another size runs on another system: the factorization of this one stays
    assert list(p.solve_batch(x0[:3], parameters=rows[:3], warm_start={})["status"]) == [SUCCESS] * 3
    assert all(i["factorizations"] == 0 for i in vjp()["info"])
    for r in (kept, after_solve, after_restoration):
        assert bits_equal(first["grad"], r["grad"])
    pm.close()


def test_an_instance_that_cannot_be_factored(m):
    """Instance 2 with s_0 = 1e-300 and z_0 = 1e300: every input is finite and s > 0, so it is not skipped, but
    Sigma = z / s overflows and no regularization makes its KKT matrix factorable: status 2, NaN rows, and the other
    four instances with the bits of the call in which it is healthy."""
    ref = sb.reference(m, "boxed")
    pm, rows = sb.build(m, "boxed")
    p = pm.p.p
    it, dp, v = sb.iterate_rows(ref, range(5)), np.array(ref["dp"]), np.array(ref["v"])
    healthy = batch_calls(p, it, rows, dp, v)
    it["s"][2, 0], it["z"][2, 0] = 1e-300, 1e300
    bad = batch_calls(p, it, rows, dp, v)
    assert list(bad[0]["status"]) == [0, 0, 0, 0, 0]  # (the right-hand sides need no factorization)
    for r, name in zip(bad[1:], ("jacobian", "jvp", "vjp")):
        assert list(r["status"]) == [0, 0, 2, 0, 0], (name, r["status"])
        for k in ("grad",) + OUT:
            if k in r and r[k][2].size:
                assert np.all(np.isnan(r[k][2])), (name, k)
    print("not factored:", bad[1]["info"][2])
    for b in (0, 1, 3, 4):
        for u, w in zip(instance_bits(healthy, b), instance_bits(bad, b)):
            assert bits_equal(u, w), b
    pm.close()


@pytest.mark.parametrize("case", ["mq", "boxed", "chain4"])
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
            batch_calls(p, it, rows, ref["dp"], ref["v"])
        r = p.solve_batch(x0, parameters=rows, warm_start={})
        assert list(first["status"]) == [SUCCESS] * 5
        results.append(r)
    a, b = results
    for k in ("status", "iterations", "restorations", "x", "s", "y", "z", "mu", "cost", "repaired"):
        assert np.array_equal(a[k], b[k]) and bits_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), k
    with_calls.close()
    without.close()


def test_a_kept_single_problem_factorization_is_not_affected(m):
    ref = sb.reference(m, "chain4")
    pm, rows = sb.build(m, "chain4")
    p = pm.p.p
    status, _ = p.solve()
    assert status == SUCCESS
    x_before, duals_before = p.get_x(), p.duals()
    before = p.sensitivity()
    batch_calls(p, sb.iterate_rows(ref, range(5)), rows, ref["dp"], ref["v"])
    after = p.sensitivity()
    assert before["info"]["factorizations"] >= 1 and after["info"]["factorizations"] == 0
    for k in OUT:
        assert bits_equal(before[k], after[k]), k
    assert bits_equal(x_before, p.get_x())
    for u, w in zip(duals_before, p.duals()):
        assert bits_equal(u, w)
    pm.close()


# ---- 6. end to end against central differences of re-solved batches --------------------------------------------------
def test_end_to_end_against_central_differences_of_re_solved_batches(m):
    pm, rows = sb.build(m, "chain4")
    rows = rows[E2E_ROWS]
    p = pm.p.p
    B, h = 3, 1e-4
    dp = sb.directions("chain4")[0][E2E_ROWS]
    x0 = np.repeat(p.get_x()[None, :], B, axis=0)
    base = p.solve_batch(x0, parameters=rows, warm_start={}, tolerance=1e-10)
    assert list(base["status"]) == [SUCCESS] * B
    jvp = p.sensitivity_batch_jvp(base, rows, dp)
    assert list(jvp["status"]) == [0] * B
    print("regularization of the three factorizations (delta, gamma):", [(i["delta"], i["gamma"]) for i in jvp["info"]])
    warm = {k: base[k] for k in ("s", "y", "z", "mu")}
    ends = [p.solve_batch(base["x"], parameters=rows + sign * h * dp, warm_start=warm, tolerance=1e-10) for sign in (+1.0, -1.0)]
    qualifying = 0
    for b in range(B):
        kept = [e["status"][b] == SUCCESS and binding_set(e["s"][b], e["z"][b]) == binding_set(base["s"][b], base["z"][b]) for e in ends]
        if not all(kept):
            print(f"instance {b} does not qualify (status and binding set kept: {kept})")
            continue
        qualifying += 1
        fd = (ends[0]["x"][b] - ends[1]["x"][b]) / (2.0 * h)
        largest = float(max(np.max(np.abs(jvp["dx"][b])), np.max(np.abs(fd))))
        diff = float(np.max(np.abs(jvp["dx"][b] - fd)))
        if largest < RESOLUTION:
            print(f"instance {b} is zero to what the differences resolve: largest entry {largest:.3e}, |dx - fd| {diff:.3e}")
            assert diff <= RESOLUTION
            continue
        bound = min(CAP_END_TO_END, 10.0 * MEASURED_END_TO_END[b])
        print(f"instance {b}: disagreement {diff / largest:.3e} of its largest entry {largest:.3e} (bound {bound:.3e})")
        assert diff / largest <= bound, (b, diff / largest, bound)
    print(f"chain4 B=3: {qualifying} of {B} instances qualify")
    assert 4 * qualifying >= 3 * B
    pm.close()


# ---- 7. surfaces -----------------------------------------------------------------------------------------------------
def test_errors(m, slpx):
    from tests.support import model

    L = slpx.lib()
    ref = sb.reference(m, "mq")
    pm, rows = sb.build(m, "mq")
    p = pm.p.p
    it = sb.iterate_rows(ref, range(3))
    x, y, mu, par = it["x"], it["y"], it["mu"], np.ascontiguousarray(rows[:3])
    out, status = np.zeros(64), np.zeros(3, dtype=np.int32)
    args = (x.ctypes.data, None, y.ctypes.data, None, mu.ctypes.data, par.ctypes.data)
    assert L.slpx_problem_sensitivity_batch(p._h, 0, *args, out.ctypes.data, None, None, None, status.ctypes.data, None) == -100
    assert b"B must be" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_batch_vjp(p._h, 70000, *args, x.ctypes.data, out.ctypes.data, None, None) == -100
    assert b"B must be" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_batch_rhs(p._h, 3, None, *args[1:], out.ctypes.data, None) == -100
    assert b"null" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_batch_jvp(p._h, 3, *args, None, out.ctypes.data, None, None, None, None, None) == -100
    assert b"dp is null" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_batch(None, 3, *args, None, None, None, None, None, None) == -100
    assert b"null problem" in L.slpx_last_error()
    assert L.slpx_problem_sensitivity_batch(p._h, 3, *args, None, None, None, None, None, None) == 0  # (every output may be NULL)
    # Python: wrong shapes
    for call in (lambda: p.sensitivity_batch(it, rows[:2]), lambda: p.sensitivity_batch(it, rows[:3, :1]),
                 lambda: p.sensitivity_batch_jvp(it, rows[:3], np.ones((3, 3))),
                 lambda: p.sensitivity_batch_vjp(it, rows[:3], np.ones((2, 2))),
                 lambda: p.sensitivity_batch_rhs(dict(it, y=np.ones((3, 2))), rows[:3]),
                 lambda: p.sensitivity_batch_rhs({k: a for k, a in it.items() if k != "mu"}, rows[:3])):
        with pytest.raises(ValueError):
            call()
    pm.close()
    q = model.NlpProblem(m)
    xq = q.decision_variable(1.0)
    q.minimize(m.pow(xq - 2, 2))
    one = np.ones((1, 1))
    assert L.slpx_problem_sensitivity_batch(q.p._h, 1, one.ctypes.data, None, None, None, one.ctypes.data, one.ctypes.data,
                                            out.ctypes.data, None, None, None, None, None) == -100
    assert b"reaches no parameter" in L.slpx_last_error()
    with pytest.raises((SlpxError, ValueError)):
        q.p.sensitivity_batch(dict(x=one, mu=np.ones(1)), np.zeros((1, 0)))
    q.p.close()


def test_optimization_problem_surface(fresh):
    from sleipnir_amd import optimization
    from tests.support import param_models as pmod

    rows = pmod.chain_rows(4, 3)
    p, _ = sb.python_chain(4, rows[0])
    x0 = np.zeros((3, 9))
    r = p.solve_batch(x0, parameters=rows, warm_start=optimization.BatchIterate())
    assert all(s == optimization.ExitStatus.SUCCESS for s in r.status)
    jac = p.sensitivity_batch(r.iterate, rows)
    assert isinstance(jac, optimization.BatchSensitivity) and jac.dx.shape == (3, 11, 9) and list(jac.status) == [0, 0, 0]
    moved = rows * 1.01  # a 1 % move of every parameter
    d = p.sensitivity_batch_jvp(r.iterate, rows, moved - rows)
    assert isinstance(d, optimization.BatchIterate) and d.mu == 0.0 and list(p.sensitivity_status) == [0, 0, 0]
    assert all(i["factorizations"] == 0 for i in p.sensitivity_info)
    assert np.max(np.abs(d.x - np.einsum("bq,bqi->bi", moved - rows, jac.dx))) <= 1e-6 * max(1.0, float(np.max(np.abs(d.x))))
    grad = p.sensitivity_batch_vjp(r.iterate, rows, np.ones((3, 9)))
    assert grad.shape == (3, 11) and np.max(np.abs(grad - jac.dx.sum(axis=2))) <= 1e-6 * max(1.0, float(np.max(np.abs(grad))))
    assert p.sensitivity_batch_rhs(r.iterate, rows).shape == (3, 11, 9 + 5 + 8)
    predicted = r.iterate + d
    from_tangent = p.solve_batch(predicted.x, parameters=moved, warm_start=predicted)
    from_iterate = p.solve_batch(r.iterate.x, parameters=moved, warm_start=r.iterate)
    print("iterations from the tangent", list(from_tangent.iterations), "from the iterate alone", list(from_iterate.iterations))
    assert all(s == optimization.ExitStatus.SUCCESS for s in from_tangent.status)
    assert np.all(from_tangent.iterations <= from_iterate.iterations)
    p.close()


def test_batch_solve_layer(fresh):
    import torch

    from sleipnir_amd import torch_layer
    from tests.test_sensitivity_gpu import python_mq

    p = python_mq()
    layer = torch_layer.BatchSolveLayer(p)
    rows = torch.tensor([[2.0, 1.0], [2.5, 0.5], [-1.0, 0.25]], dtype=torch.float64, requires_grad=True)
    xs = layer(rows)
    a, b = rows.detach()[:, 0], rows.detach()[:, 1]
    want = torch.stack([(a + b - 1) / 2, (b - a + 1) / 2], dim=1)  # x* of mq
    assert tuple(xs.shape) == (3, 2) and xs.dtype == torch.float64 and list(layer.status) == [0, 0, 0]
    assert torch.max(torch.abs(xs.detach() - want)) <= 1e-9
    (xs ** 2).sum().backward(retain_graph=True)
    # d/da = x - y, d/db = x + y at x* (dx/da = (1/2, -1/2), dx/db = (1/2, 1/2))
    x, y = xs.detach()[:, 0], xs.detach()[:, 1]
    assert torch.max(torch.abs(rows.grad - torch.stack([x - y, x + y], dim=1))) <= 1e-10
    assert list(layer.sensitivity_status) == [0, 0, 0] and layer.warm_forwards == 0
    rows2 = torch.tensor([[2.1, 1.0], [2.5, 0.6], [-1.0, 0.3]], dtype=torch.float64, requires_grad=True)
    xs2 = layer(rows2)
    assert layer.warm_forwards == 1 and layer.solves == 2  # (began at the first forward's iterates)
    (3.0 * xs2[:, 0]).sum().backward()
    assert torch.max(torch.abs(rows2.grad - 1.5)) <= 1e-10
    with pytest.raises(RuntimeError, match="not the layer's last"):
        (xs ** 2).sum().backward()
    p.close()
