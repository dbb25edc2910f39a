"""Models for the tests of the solution sensitivities, beside those of param_models.py (which they build on).

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

from . import model
from .param_models import ParamModel

COST_FACTOR, ROW_FACTOR = 1000.0, 500.0


def mq_scaled(m, values, x0=(0.0, 0.0)):
    """param_models.mq with the cost multiplied by 1000 and the equality row by 500: the same solution
    x = (a + b - 1) / 2, y = (b - a + 1) / 2, but gradients of thousands and a Jacobian row of 500 at x0, so that
    compute_problem_scaling (threshold 100) gives d_f = 100 / 4000 and d_ce = 100 / 500 — scales other than 1.  The
    multiplier of the row as written is lambda_u = 1000 * 2 (x - a) / 500 = 2 (b - 1 - a)."""
    a_val, b_val = values
    p = model.NlpProblem(m)
    x, y = p.decision_variable(x0[0]), p.decision_variable(x0[1])
    a, b = m.variable(a_val), m.variable(b_val)
    p.minimize(COST_FACTOR * (m.pow(x - a, 2) + m.pow(y - 1, 2)))
    p.eq(ROW_FACTOR * (x + y), ROW_FACTOR * b)
    return ParamModel(p, [x, y], [a, b])
