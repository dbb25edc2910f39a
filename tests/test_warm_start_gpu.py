"""Warm starts, whole solves on the device: solve(warm_start=...) and solve_batch(..., warm_start=...) from the iterate an
earlier solve ended at (include/slpx.h: warm starts; sleipnir_amd/csrc/warm_start.h: units and safeguard).

Models: tests/support/param_models.py.  SCALES: the cost gradients and the constraint Jacobians' rows of boxed, mq, m2,
restoring and chain(4 / 8) stay far below the scaling threshold of 100 at every point these tests solve from (the
largest is the chain's 2 (X - r), a few units), so compute_problem_scaling gives scales of 1 at the cold start AND at
the warm one: the scaled iterate (duals()) and the one in the user's units (iterate()) then have the same bits, which
test 1 asserts, and a round trip returns the iterate's bits.  Non-trivial scales are the kernel tests' ground
(test_warm_start_kernels_gpu.py, test_warm_start_cpu.py).

Iteration counts of every case are printed (run with -s); profiles/warm_start.txt keeps the record."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import param_models as pmod
from tests.support import warmcheck_host as wh

pytestmark = pytest.mark.gpu

SUCCESS, NONFINITE, GLOBALLY_INFEASIBLE = 0, -7, -3
TOLERANCE = 1e-8
BATCH_VS_SINGLE = 1e-6  # tests/test_solve_batch_gpu.py: _compare_with_singles


@pytest.fixture
def m(fresh):
    mm = pmod.new_model()
    mm.be.reset()
    return mm


BUILD = {
    "boxed": (lambda m, row=(0.0, 1.0): pmod.boxed(m, row), (0.0, 1.0)),
    "mq": (lambda m, row=(2.0, 1.0): pmod.mq(m, row), (2.0, 1.0)),
    "m2": (lambda m, row=(2.0,): pmod.m2(m, row), (2.0,)),
    "restoring": (lambda m, row=(1.0,): pmod.restoring(m, row, x0=(2.0, 3.0, 1.0)), (1.0,)),
    "chain4": (lambda m, row=None: pmod.chain(m, 4, pmod.chain_rows(4, 1)[0] if row is None else row), pmod.chain_rows(4, 1)[0]),
    "chain8": (lambda m, row=None: pmod.chain(m, 8, pmod.chain_rows(8, 1)[0] if row is None else row), pmod.chain_rows(8, 1)[0]),
}


def solve(p, x=None, warm=None, **kw):
    """-> dict(status, iterations, x, iterate (x, s, y, z, mu), repaired)"""
    if x is not None:
        p.set_x(np.asarray(x, dtype=np.float64))
    status, rep = p.solve(warm_start=warm, **kw) if warm is not None else p.solve(**kw)
    it = p.iterate()
    return dict(status=status, iterations=rep["iterations"], x=p.get_x(), iterate=it, repaired=p.warm_start_repaired(),
                restorations=rep["restorations"])


def blocks(it, keep=("s", "y", "z", "mu")):
    d = dict(s=it[1], y=it[2], z=it[3], mu=it[4])
    return {k: v for k, v in d.items() if k in keep}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. nothing changed ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["boxed", "mq", "m2", "chain4"])
def test_without_a_warm_start_nothing_changed(m, slpx, case):
    L = slpx.lib()
    pm = BUILD[case][0](m)
    p = pm.p.p
    x0 = p.get_x()
    first = solve(p, x0)
    s, y, z = p.duals()
    assert first["status"] == SUCCESS and first["iterations"] > 0
    # (scales of 1, see the module's docstring: the conversion is the identity)
    assert bits_equal(first["iterate"][1], s) and bits_equal(first["iterate"][2], y) and bits_equal(first["iterate"][3], z)
    # slpx_problem_solve_warm(ws = NULL)
    p.set_x(x0)
    opt, rep = sa.Options(TOLERANCE, 5000, 0.0, 0, 0, 0), sa.Report()
    status = L.slpx_problem_solve_warm(p._h, ctypes.byref(opt), ctypes.sizeof(sa.Options), None, ctypes.byref(rep))
    assert (status, rep.iterations) == (first["status"], first["iterations"]) and bits_equal(p.get_x(), first["x"])
    assert all(bits_equal(a, b) for a, b in zip(p.duals(), (s, y, z)))
    # the batch: all-NULL starts against slpx_problem_solve_batch_parameters
    X0 = np.repeat(x0[None, :], 3, axis=0) + np.array([[0.0], [0.01], [-0.02]])
    rows = np.repeat(np.asarray(BUILD[case][1], dtype=np.float64)[None, :], 3, axis=0)
    plain = p.solve_batch(X0, parameters=rows)
    warm = p.solve_batch(X0, parameters=rows, warm_start={})
    for k in ("status", "iterations", "restorations", "x", "cost"):
        assert bits_equal(plain[k], warm[k]) if plain[k].dtype == np.float64 else np.array_equal(plain[k], warm[k]), k
    for k in ("s", "y", "z"):
        assert bits_equal(plain[k], warm[k]), k  # (scales of 1)
    assert not warm["repaired"].any()
    pm.close()


# ---- 2. round trip: the test that fails without the feature ----------------------------------------------------------
@pytest.mark.parametrize("case", ["boxed", "mq", "restoring", "chain4"])
def test_round_trip_takes_no_iteration(m, case):
    pm = BUILD[case][0](m)
    p = pm.p.p
    cold = solve(p)
    assert cold["status"] == SUCCESS and cold["iterations"] > 0, cold
    it = cold["iterate"]
    warm = solve(p, it[0], blocks(it))
    print(case, "round trip: cold", cold["iterations"], "warm", warm["iterations"], "repaired", warm["repaired"])
    assert warm["status"] == SUCCESS and warm["iterations"] == 0, warm
    assert bits_equal(warm["x"], cold["x"]) and warm["repaired"] == 0
    for a, b in zip(warm["iterate"], it):
        assert bits_equal(a, b)
    # the same through the batch, every instance from the same iterate
    B = 3
    rep3 = lambda v: np.repeat(np.atleast_1d(np.asarray(v, dtype=np.float64))[None, :], B, axis=0)
    r = p.solve_batch(rep3(it[0]), warm_start=dict(s=rep3(it[1]), y=rep3(it[2]), z=rep3(it[3]), mu=np.full(B, it[4])))
    assert list(r["status"]) == [SUCCESS] * B and list(r["iterations"]) == [0] * B and not r["repaired"].any(), r
    for b in range(B):
        assert bits_equal(r["x"][b], cold["x"])
        for k, j in (("s", 1), ("y", 2), ("z", 3)):
            assert bits_equal(r[k][b], it[j]), k
        assert r["mu"][b] == it[4]
    pm.close()


def test_round_trip_through_the_python_surface(fresh):
    from sleipnir_amd import optimization

    p = optimization.Problem()
    x = p.decision_variable()
    x.set_value(0.5)
    p.minimize((x - 3) ** 2)
    p.subject_to(x <= 1)
    p.subject_to(x >= 0)
    assert p.solve() == optimization.ExitStatus.SUCCESS and p.report["iterations"] > 0
    it = p.iterate()
    assert isinstance(it, optimization.Iterate) and it.mu > 0 and abs(it.x[0] - 1.0) <= 1e-6
    assert p.solve(warm_start=it) == optimization.ExitStatus.SUCCESS
    assert p.report["iterations"] == 0 and p.warm_start_repaired() == 0
    r = p.solve_batch(np.array([it.x, it.x]), warm_start=optimization.BatchIterate(
        s=np.array([it.s, it.s]), y=np.zeros((2, 0)), z=np.array([it.z, it.z]), mu=[it.mu, it.mu]))
    assert r.status == [optimization.ExitStatus.SUCCESS] * 2 and list(r.iterations) == [0, 0]
    assert isinstance(r.iterate, optimization.BatchIterate) and list(r.repaired) == [0, 0]
    assert p.solve_batch(np.array([it.x])).iterate is None
    p.close()


# ---- 3., 4. changed parameters ---------------------------------------------------------------------------------------
def closed_form(case, row):
    if case == "boxed":
        return np.array([min(max(3.0, row[0]), row[1])])
    a, b = row
    t = (b - a - 1.0) / 2.0
    return np.array([a + t, 1.0 + t])


@pytest.mark.parametrize("case", ["boxed", "mq"])
@pytest.mark.parametrize("percent", [1, 10])
def test_changed_parameters_closed_form(m, case, percent):
    build, row = BUILD[case]
    pm = build(m)
    p = pm.p.p
    x_start = p.get_x()
    old = solve(p)
    assert old["status"] == SUCCESS
    new_row = np.asarray(row, dtype=np.float64) * (1.0 + percent / 100.0)
    p.set_parameters(new_row)
    cold = solve(p, x_start)
    warm = solve(p, old["iterate"][0], blocks(old["iterate"]))
    want = closed_form(case, new_row)
    d_cold, d_warm = np.max(np.abs(cold["x"] - want)), np.max(np.abs(warm["x"] - want))
    print(f"{case} {percent}%: iterations cold {cold['iterations']} warm {warm['iterations']} repaired {warm['repaired']} "
          f"distance to the closed form cold {d_cold:.3e} warm {d_warm:.3e}")
    assert cold["status"] == SUCCESS and warm["status"] == SUCCESS
    assert d_warm <= max(10.0 * d_cold, TOLERANCE), (d_warm, d_cold)
    if percent == 1:
        assert warm["iterations"] <= cold["iterations"], (warm["iterations"], cold["iterations"])
    pm.close()


def test_changed_parameters_chain8(m):
    build, row = BUILD["chain8"]
    pm = build(m)
    p = pm.p.p
    x_start = p.get_x()
    old = solve(p)
    assert old["status"] == SUCCESS
    new_row = np.array(row, dtype=np.float64)
    new_row[2:3 + 8] *= 1.01  # x_init and the references
    p.set_parameters(new_row)
    cold = solve(p, x_start)
    fine = solve(p, x_start, tolerance=1e-10)
    warm = solve(p, old["iterate"][0], blocks(old["iterate"]))
    sensitivity = np.max(np.abs(cold["x"] - fine["x"]))  # two cold solves at tolerances 1e-8 and 1e-10: the solver's own
    d_warm = np.max(np.abs(warm["x"] - cold["x"]))
    print(f"chain8 1%: iterations cold {cold['iterations']} warm {warm['iterations']} repaired {warm['repaired']} "
          f"warm against cold {d_warm:.3e}, cold 1e-8 against cold 1e-10 {sensitivity:.3e}")
    assert cold["status"] == SUCCESS and fine["status"] == SUCCESS and warm["status"] == SUCCESS
    assert d_warm <= 10.0 * sensitivity, (d_warm, sensitivity)
    assert warm["iterations"] <= cold["iterations"], (warm["iterations"], cold["iterations"])
    pm.close()


# ---- 5. safeguards end to end ----------------------------------------------------------------------------------------
def c_i_at(p, x):
    """c_i(x) at unit scales from the problem's own system"""
    n, me, mi = p.dims
    sy = p.system()
    sy.set_scaling(np.ones(1 + me + mi))
    sy.set_state(x=x)
    sy.sweep(full=False)
    return sy.get("V")[0][1 + me:1 + me + mi].copy()


@pytest.mark.parametrize("what", ["z = 0", "s absent", "mu absent"])
def test_safeguards_still_converge(m, what):
    pm = BUILD["chain4"][0](m)
    p = pm.p.p
    n, me, mi = p.dims
    cold = solve(p)
    assert cold["status"] == SUCCESS
    x, s, y, z, mu = cold["iterate"]
    given = {"z = 0": dict(s=s, y=y, z=np.zeros(mi), mu=mu), "s absent": dict(y=y, z=z, mu=mu),
             "mu absent": dict(s=s, y=y, z=z)}[what]
    ci = c_i_at(p, x)
    ref = wh.instance(np.ones(1 + me + mi), me, ci, x, given.get("s"), given.get("y"), given.get("z"), given.get("mu", 0.0),
                      TOLERANCE / 10.0)
    warm = solve(p, x, given)
    print(f"chain4 {what}: iterations cold {cold['iterations']} warm {warm['iterations']} repaired {warm['repaired']} "
          f"(numpy {ref['repaired']})")
    assert warm["status"] == SUCCESS
    assert warm["repaired"] == ref["repaired"]
    assert np.max(np.abs(warm["x"] - cold["x"])) <= 1e-6
    # the batch counts the same
    r = p.solve_batch(np.array([x, x]), warm_start={k: np.array([v, v]) for k, v in given.items()})
    assert list(r["status"]) == [SUCCESS, SUCCESS] and list(r["repaired"]) == [ref["repaired"]] * 2
    pm.close()


def test_a_nan_ends_its_instance_alone(m):
    """boxed, B = 3: a NaN in instance 1's z gives NONFINITE_INITIAL_GUESS there; the other two return the bits they
    return when instance 1 is kept from running by a conflicting-bounds row instead."""
    pm = BUILD["boxed"][0](m)
    p = pm.p.p
    rows = np.array([[0.0, 1.0], [0.0, 1.2], [-1.0, 0.9]])
    X0 = np.array([[0.5], [0.6], [0.2]])
    first = p.solve_batch(X0, parameters=rows, warm_start={})
    assert list(first["status"]) == [SUCCESS] * 3
    rows2 = rows * 1.01
    ws = dict(s=first["s"].copy(), y=first["y"], z=first["z"].copy(), mu=first["mu"])
    ws["z"][1, 0] = float("nan")
    got = p.solve_batch(first["x"], parameters=rows2, warm_start=ws)
    assert list(got["status"]) == [SUCCESS, NONFINITE, SUCCESS], got["status"]
    assert got["iterations"][1] == 0
    masked_rows = rows2.copy()
    masked_rows[1] = [2.0, 1.0]  # lo > hi
    ws["z"][1, 0] = 1.0
    want = p.solve_batch(first["x"], parameters=masked_rows, warm_start=ws)
    assert list(want["status"]) == [SUCCESS, GLOBALLY_INFEASIBLE, SUCCESS]
    for b in (0, 2):
        for k in ("x", "s", "y", "z", "mu", "cost"):
            assert bits_equal(got[k][b], want[k][b]), (b, k)
        assert got["iterations"][b] == want["iterations"][b] and got["repaired"][b] == want["repaired"][b]
    # the single solve says the same of a NaN, before any iteration
    p.set_parameters(rows2[1])
    bad = solve(p, first["x"][1], dict(s=first["s"][1], z=np.array([float("nan"), 1.0]), mu=float(first["mu"][1])))
    assert bad["status"] == NONFINITE and bad["iterations"] == 0
    bad = solve(p, first["x"][1], dict(s=first["s"][1], z=first["z"][1], mu=float("inf")))
    assert bad["status"] == NONFINITE and bad["iterations"] == 0
    pm.close()


# ---- 6. batch against single -----------------------------------------------------------------------------------------
def test_batch_against_single(m):
    B = 3
    rows = pmod.chain_rows(4, B)
    pm = pmod.chain(m, 4, rows[0])
    p = pm.p.p
    n = p.dims[0]
    first = p.solve_batch(np.zeros((B, n)), parameters=rows, warm_start={})
    assert list(first["status"]) == [SUCCESS] * B
    rows2 = rows.copy()
    rows2[:, 2:3 + 4] *= 1.01
    ws = {k: first[k] for k in ("s", "y", "z", "mu")}
    r = p.solve_batch(first["x"], parameters=rows2, warm_start=ws)
    cold = p.solve_batch(np.zeros((B, n)), parameters=rows2)
    for b in range(B):
        p.set_parameters(rows2[b])
        one = solve(p, first["x"][b], {k: (v[b] if k != "mu" else float(v[b])) for k, v in ws.items()})
        print(f"chain4 row {b} 1%: iterations cold {cold['iterations'][b]} warm batch {r['iterations'][b]} single {one['iterations']} "
              f"repaired {r['repaired'][b]}")
        assert r["status"][b] == one["status"] == SUCCESS
        assert r["iterations"][b] == one["iterations"] and r["repaired"][b] == one["repaired"]
        assert np.max(np.abs(r["x"][b] - one["x"])) <= BATCH_VS_SINGLE
    pm.close()


# ---- 7. SQP and Newton -----------------------------------------------------------------------------------------------
def test_sqp_reads_x_and_y(m):
    pm = BUILD["mq"][0](m)
    p = pm.p.p
    cold = solve(p)
    assert cold["status"] == SUCCESS and cold["iterations"] > 0
    x, s, y, z, mu = cold["iterate"]
    assert s.size == 0 and z.size == 0 and mu == 0.0
    warm = solve(p, x, dict(y=y, mu=5.0))  # (mu is ignored)
    assert warm["status"] == SUCCESS and warm["iterations"] == 0 and bits_equal(warm["x"], cold["x"])
    bad = solve(p, x, dict(y=np.array([float("nan")])))
    assert bad["status"] == NONFINITE and bad["iterations"] == 0
    r = p.solve_batch(np.array([x, x]), warm_start=dict(y=np.array([y, [float("inf")]])))
    assert list(r["status"]) == [SUCCESS, NONFINITE] and r["iterations"][0] == 0
    pm.close()


def test_newton_takes_x_only(m):
    pm = BUILD["m2"][0](m)
    p = pm.p.p
    x0 = np.array([0.3, -0.4])
    cold = solve(p, x0)
    warm = solve(p, x0, dict(mu=1e-3))
    assert cold["status"] == warm["status"] == SUCCESS and warm["iterations"] == cold["iterations"]
    assert bits_equal(warm["x"], cold["x"])
    a, b = p.solve_batch(x0[None, :]), p.solve_batch(x0[None, :], warm_start=dict(mu=[1e-3]))
    assert bits_equal(a["x"], b["x"]) and list(a["iterations"]) == list(b["iterations"])
    pm.close()
