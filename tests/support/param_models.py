"""Small models with PARAMETERS — free variables that are no decision variables — for the tests of parameters as
runtime inputs (slpx_problem_set_parameters, slpx_problem_solve_batch_parameters, slpx_system_set_parameters).

Every builder takes the parameters' values and makes them the variables' values BEFORE anything is compiled: built
with row b, a model is "row b folded in" the way the library has always done it (the tape compiler copies a parameter's
value into its constant slot at compile time).  The tests compare the new entry points with exactly that.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

from . import model


class ParamModel:
    """p: the model.NlpProblem (p.p: sleipnir_amd.Problem); x: decision variables, params: parameter variables, both
    in creation (= ascending node) order."""

    def __init__(self, p, x, params):
        self.p, self.x, self.params = p, x, params

    @property
    def param_ids(self):
        return [v.node for v in self.params]

    def close(self):
        self.p.p.close()


def new_model():
    be = model.ProductBackend("gpu")
    return model.Model(be)


def m2(m, values, x0=(0.0, 0.0)):
    """min (x - a)^2 + (y - 1)^2, parameter a: no constraints, the Newton driver."""
    (a_val,) = values
    p = model.NlpProblem(m)
    x, y = p.decision_variable(x0[0]), p.decision_variable(x0[1])
    a = m.variable(a_val)
    p.minimize(m.pow(x - a, 2) + m.pow(y - 1, 2))
    return ParamModel(p, [x, y], [a])


def mq(m, values, x0=(0.0, 0.0)):
    """m2 plus x + y == b: equality rows only, the SQP driver; b sits in the VALUE of a LINEAR row."""
    a_val, b_val = values
    p = model.NlpProblem(m)
    x, y = p.decision_variable(x0[0]), p.decision_variable(x0[1])
    a, b = m.variable(a_val), m.variable(b_val)
    p.minimize(m.pow(x - a, 2) + m.pow(y - 1, 2))
    p.eq(x + y, b)
    return ParamModel(p, [x, y], [a, b])


def chain_parameter_count(stages):
    return 3 + 2 * stages


def chain(m, stages, values, x0=None):
    """A chain of `stages` stages, states X_0..X_stages, inputs U_0..U_{stages-1}; interior point.

    Parameters, in this order: gain, u_max, x_init, r_0..r_{stages-1}, d_0..d_{stages-1}
      dynamics   X_{k+1} == gain * X_k + phi(X_k, U_k) + d_k   gain * X_k is QUADRATIC (parameter x decision variable),
                                                               d_k is "parameter k of stage k": affine in the stage;
                                                               phi: sin, cos, exp, tanh terms
      cost       sum_k (X_{k+1} - r_k)^2 + 0.1 U_k^2           per-stage references
      bounds     -u_max <= U_k <= u_max                        parametric bounds, LINEAR rows
      start      X_0 == x_init                                 a parameter in the value of a LINEAR row
    With 8 stages the dynamics rows are a family (kTapeFamilyMin = 8): a generated body; with 4 they are interpreted."""
    values = np.asarray(values, dtype=np.float64)
    assert values.shape == (chain_parameter_count(stages),)
    p = model.NlpProblem(m)
    X = [p.decision_variable(0.0) for _ in range(stages + 1)]
    U = [p.decision_variable(0.0) for _ in range(stages)]
    gain, u_max, x_init = (m.variable(v) for v in values[:3])
    r = [m.variable(v) for v in values[3:3 + stages]]
    d = [m.variable(v) for v in values[3 + stages:]]
    cost = None
    for k in range(stages):
        term = m.pow(X[k + 1] - r[k], 2) + 0.1 * m.pow(U[k], 2)
        cost = term if cost is None else cost + term
    p.minimize(cost)
    p.eq(X[0], x_init)
    for k in range(stages):
        # (a stage of 16 or more interior nodes: what the tape compiler gives a task of its own, tape_compiler.cpp)
        p.eq(X[k + 1], gain * X[k] + 0.2 * m.sin(U[k]) + 0.1 * m.cos(X[k]) * U[k] + 0.05 * m.exp(-0.5 * X[k] * X[k])
             + 0.02 * m.tanh(X[k] + U[k]) + d[k])
    for k in range(stages):
        p.ge(U[k], -u_max)
        p.le(U[k], u_max)
    pm = ParamModel(p, X + U, [gain, u_max, x_init] + r + d)
    if x0 is not None:
        p.p.set_x(np.asarray(x0, dtype=np.float64))
    return pm


def chain_rows(stages, count, seed=7):
    """`count` different parameter rows of chain(stages): gains around 0.9, input bounds that bind for some rows and
    not for others, references and disturbances of a size that moves the solution."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((count, chain_parameter_count(stages)))
    for b in range(count):
        rows[b, 0] = 0.8 + 0.1 * b                        # gain
        rows[b, 1] = (0.3, 2.0, 0.7, 1.2)[b % 4]          # u_max
        rows[b, 2] = (-1.0, 0.5, 2.0, 0.0)[b % 4]         # x_init
        rows[b, 3:3 + stages] = rng.uniform(-1.0, 1.0, stages) * (1 + b)
        rows[b, 3 + stages:] = rng.uniform(-0.2, 0.2, stages)
    return rows


def restoring(m, values, x0=(-2.0, 3.0, 1.0)):
    """The 3-variable model of test_restoration_inside_a_batch (tests/test_solve_batch_gpu.py) with the constant of
    its quadratic row turned into the parameter c: min x s.t. x^2 - s1 - c == 0, x - s2 - 0.5 == 0, s1, s2 >= 0."""
    (c_val,) = values
    p = model.NlpProblem(m)
    x, s1, s2 = (p.decision_variable(v) for v in x0)
    c = m.variable(c_val)
    p.minimize(x)
    p.eq(m.pow(x, 2) - s1 - c, 0)
    p.eq(x - s2 - 0.5, 0)
    p.ge(s1, 0)
    p.ge(s2, 0)
    return ParamModel(p, [x, s1, s2], [c])


def boxed(m, values, x0=(0.5,)):
    """min (x - 3)^2 s.t. lo <= x <= hi with both bounds parameters: lo > hi is a conflict of that instance alone."""
    lo_val, hi_val = values
    p = model.NlpProblem(m)
    x = p.decision_variable(x0[0])
    lo, hi = m.variable(lo_val), m.variable(hi_val)
    p.minimize(m.pow(x - 3, 2))
    p.ge(x, lo)
    p.le(x, hi)
    return ParamModel(p, [x], [lo, hi])


BATCH_KEYS = ("status", "iterations", "x", "s", "y", "z", "cost")


def folded_instance(build, row, x0, batch, **solve_kw):
    """Instance 0 of solve_batch(batch copies of x0) on the model built with `row` folded in: what the library computed
    for "this model with these parameter values" before parameters were runtime inputs."""
    pm = build(row)
    r = pm.p.p.solve_batch(np.repeat(np.asarray(x0, dtype=np.float64)[None, :], batch, axis=0), **solve_kw)
    pm.close()
    return {k: np.array(r[k][0]) for k in BATCH_KEYS + ("restorations",)}


def assert_instance_equal(got, b, want, what=""):
    for k in BATCH_KEYS:
        assert np.array_equal(np.asarray(got[k][b]), want[k]), (what, b, k, got[k][b], want[k])
