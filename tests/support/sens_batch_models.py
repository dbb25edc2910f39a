"""The cases of the batched sensitivity tests (tests/test_sensitivity_batch_gpu.py): for every model of
param_models.py that the tests use, its builder and five different parameter rows, and the single-problem reference —
row by row set_parameters(), solve(), iterate() and the four single-problem sensitivity calls on ONE problem — computed
once per case and shared by the tests that compare with it.  python_chain() is param_models.chain() written with the
Python modelling classes, for the tests of that surface.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

from . import param_models as pmod

# dimM = n + m_e + m_i = 5 stages + 2 of a chain: 51 is the smallest stage count with dimM > 256 (257), so that rows lie
# past a 256-entry slice of the row axis; n + m_e = 155 there, below the 256 lanes of the vjp's dot product
LONG_CHAIN_STAGES = 51
# n + m_e = 3 stages + 2: 85 is the smallest stage count with n + m_e > 256 (257), so that lane 0 of the vjp's dot
# product (sens_rows.h: sens_vjp_partial) takes a second row, 256 further on
VJP_STRIDE_CHAIN_STAGES = 85

BOXED_ROWS = np.array([[0.0, 2.0], [0.0, 5.0], [1.0, 2.5], [-1.0, 4.0], [0.5, 1.5]])  # upper bound active where hi < 3
BOXED_ACTIVE = (True, False, True, False, True)

CASES = {
    # name: (builder(m, row), rows (5, n_p) — the two long chains: 3 rows, cycled where a batch is larger)
    "m2": (lambda m, row: pmod.m2(m, row), np.array([[2.0], [-1.0], [0.5], [3.0], [1.5]])),
    "mq": (lambda m, row: pmod.mq(m, row), np.array([[2.0, 1.0], [2.5, 0.5], [-1.0, 0.25], [0.5, 3.0], [1.5, -2.0]])),
    "boxed": (lambda m, row: pmod.boxed(m, row), BOXED_ROWS),
    "chain4": (lambda m, row: pmod.chain(m, 4, row), pmod.chain_rows(4, 5)),  # rows 0, 1: those of chain_rows(4, 2)
    "chain8": (lambda m, row: pmod.chain(m, 8, row), pmod.chain_rows(8, 5)),
    "chain51": (lambda m, row: pmod.chain(m, LONG_CHAIN_STAGES, row), pmod.chain_rows(LONG_CHAIN_STAGES, 3)),
    "chain85": (lambda m, row: pmod.chain(m, VJP_STRIDE_CHAIN_STAGES, row), pmod.chain_rows(VJP_STRIDE_CHAIN_STAGES, 3)),
}
assert np.array_equal(pmod.chain_rows(4, 5)[:2], pmod.chain_rows(4, 2))


def build(m, case):
    builder, rows = CASES[case]
    return builder(m, rows[0]), rows.copy()


def directions(case):
    """(dp (rows, n_p), v (rows, n)): one direction and one cotangent per instance, the same in every test"""
    rows = CASES[case][1]
    rng = np.random.default_rng(11)
    n = {"m2": 2, "mq": 2, "boxed": 1}.get(case)
    if n is None:
        n = 2 * int(case[5:]) + 1
    return rng.uniform(-1.0, 1.0, rows.shape), rng.uniform(-1.0, 1.0, (rows.shape[0], n))


_REFERENCE = {}


def reference(m, case, **solve_kw):
    """dict(rows, x, s, y, z, mu (stacked per row), dx, ds, dy, dz (rows, n_p, .), jvp: dict, grad, M, info): the
    single-problem path at every row, computed on first use and read-only afterwards."""
    key = (case, tuple(sorted(solve_kw.items())))
    if key in _REFERENCE:
        return _REFERENCE[key]
    pm, rows = build(m, case)
    p = pm.p.p
    x0 = p.get_x()
    dp, v = directions(case)
    acc = {k: [] for k in ("x", "s", "y", "z", "mu", "dx", "ds", "dy", "dz", "jdx", "jds", "jdy", "jdz", "grad", "M", "info")}
    for b, row in enumerate(rows):
        p.set_parameters(row)
        p.set_x(x0)
        status, _ = p.solve(**solve_kw)
        assert status == 0, (case, b, status)
        for k, a in zip(("x", "s", "y", "z", "mu"), p.iterate()):
            acc[k].append(np.array(a))
        jac = p.sensitivity()
        for k in ("dx", "ds", "dy", "dz"):
            acc[k].append(jac[k])
        acc["info"].append(jac["info"])
        jvp = p.sensitivity_jvp(dp[b])
        for k in ("dx", "ds", "dy", "dz"):
            acc["j" + k].append(jvp[k])
        acc["grad"].append(p.sensitivity_vjp(v[b])[0])
        acc["M"].append(p.sensitivity_rhs())
    pm.close()
    ref = {k: (np.stack(a) if k != "info" else a) for k, a in acc.items()}
    ref["rows"], ref["dp"], ref["v"] = rows, dp, v
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _REFERENCE[key] = ref
    return ref


def iterate_rows(ref, idx):
    """the iterates of the reference's rows `idx` as the batched calls take them"""
    idx = list(idx)
    return {k: np.array(ref[k][idx]) for k in ("x", "s", "y", "z", "mu")}


def python_chain(stages, values):
    """param_models.chain() with optimization.Problem and autodiff.Variable: (problem, parameter Variables)"""
    from sleipnir_amd import autodiff as ad
    from sleipnir_amd import optimization

    values = np.asarray(values, dtype=np.float64)
    assert values.shape == (pmod.chain_parameter_count(stages),)
    p = optimization.Problem()
    X = [p.decision_variable() for _ in range(stages + 1)]
    U = [p.decision_variable() for _ in range(stages)]
    params = []
    for value in values:
        var = ad.Variable()
        var.set_value(float(value))
        params.append(var)
    gain, u_max, x_init = params[:3]
    r, d = params[3:3 + stages], params[3 + stages:]
    cost = None
    for k in range(stages):
        term = (X[k + 1] - r[k]) ** 2 + 0.1 * U[k] ** 2
        cost = term if cost is None else cost + term
    p.minimize(cost)
    p.subject_to(X[0] == x_init)
    for k in range(stages):
        p.subject_to(X[k + 1] == gain * X[k] + 0.2 * ad.sin(U[k]) + 0.1 * ad.cos(X[k]) * U[k] + 0.05 * ad.exp(-0.5 * X[k] * X[k])
                     + 0.02 * ad.tanh(X[k] + U[k]) + d[k])
    for k in range(stages):
        p.subject_to(U[k] >= -u_max)
        p.subject_to(U[k] <= u_max)
    return p, params
