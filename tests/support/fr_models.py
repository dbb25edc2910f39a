"""General models for the kernel-by-kernel tests of feasibility restoration (tests/test_restoration_kernels_gpu.py), on
either backend of tests.support.model.  Unlike the benchmark models (simple bounds only) their inequality rows have two
or three entries, the cost's Hessian shares entries with the constraints', and chain(n) has a hub variable whose columns
of A_e and A_i have more than sixteen entries.  Smooth, with independent constraint gradients at the starts below.

TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

from tests.support import model


def _sum(terms):
    it = iter(terms)
    acc = next(it)
    for t in it:
        acc = acc + t
    return acc


def tiny(m):
    """n = 4, m_e = 1, m_i = 2: x0^2 + x1^2 <= 1.5 (two entries), x0 + 2 x1 - x2 >= -1 (three), x0 x2 + x1^2 = 0.8; x3 is in
    the cost only.  H_f and H_c share (0, 0), (1, 1) and the off-diagonal (2, 0)."""
    p = model.NlpProblem(m)
    x = [p.decision_variable(v) for v in tiny_start()]
    p.minimize(_sum([(x[k] - 1.0) * (x[k] - 1.0) for k in range(4)]) + 0.5 * (x[0] * x[2]) + 0.25 * (x[0] * x[1]))
    p.le(x[0] * x[0] + x[1] * x[1], 1.5)
    p.ge(x[0] + 2.0 * x[1] - x[2], -1.0)
    p.eq(x[0] * x[2] + x[1] * x[1], 0.8)
    return p


def tiny_start():
    return np.array([0.6, 0.5, 0.4, 0.3])


def ineq_only(m):
    """n = 5, m_e = 0, m_i = 4, rows of two to three entries."""
    p = model.NlpProblem(m)
    x = [p.decision_variable(v) for v in ineq_only_start()]
    p.minimize(_sum([(x[k] - 1.0) * (x[k] - 1.0) for k in range(5)]) + x[0] * x[1] + x[2] * x[3])
    p.le(x[0] * x[0] + x[1] * x[1], 2.0)
    p.ge(x[1] + x[2] - 2.0 * x[3], -3.0)
    p.ge(x[2] * x[3] + x[4], -1.0)
    p.ge(x[3] - x[4] * x[4], -2.0)
    return p


def ineq_only_start():
    return np.array([0.5, 0.6, 0.7, 0.4, 0.3])


def eq_only(m):
    """n = 6, m_e = 3, m_i = 0 (the kernels' empty inequality blocks)."""
    p = model.NlpProblem(m)
    x = [p.decision_variable(v) for v in eq_only_start()]
    p.minimize(_sum([(x[k] - 0.5) * (x[k] - 0.5) for k in range(6)]) + x[0] * x[1])
    p.eq(x[0] * x[1] + x[2], 1.0)
    p.eq(x[2] * x[2] + x[3] - x[4], 0.5)
    p.eq(x[4] * x[5] - x[0], 0.2)
    return p


def eq_only_start():
    return np.array([0.3, 0.4, 0.5, 0.6, 0.7, 0.8])


CHAIN_HUB_ROWS = 24  # rows of each kind the hub variable appears in


def chain_start(n):
    x = 0.5 + 0.3 * np.sin(0.7 * np.arange(n))
    x[n - 1] = 0.4  # the hub
    return x


def chain(m, n):
    """n variables, the last one the hub.
    Equalities, about n / 2 rows: x_k x_{k+1} + x_{k+2} = c_k for even k <= n - 5, the first CHAIN_HUB_ROWS of them with
    + 0.05 hub^2 (column k + 1 is in row k only and x_k != 0 at the start: independent gradients).
    Inequalities, m_i >= n: for k < n - 2 in turn x_k^2 + x_{k+1}^2 <= 4, x_{k-1} + x_k - 2 x_{k+1} >= -5, x_k >= -3;
    CHAIN_HUB_ROWS rows hub^2 + x_{5j+1}^2 <= 4; x_k <= 3 for every k (plain bounds).
    Cost: sum (x_k - sin(k) / 2)^2 + 0.1 sum x_k x_{k+1}: H_f shares the entries (k + 1, k) with H_c."""
    assert n >= 5 * CHAIN_HUB_ROWS + 8
    p = model.NlpProblem(m)
    x = [p.decision_variable(v) for v in chain_start(n)]
    hub = x[n - 1]
    p.minimize(_sum([(x[k] - 0.5 * math.sin(k)) * (x[k] - 0.5 * math.sin(k)) for k in range(n)])
               + 0.1 * _sum([x[k] * x[k + 1] for k in range(n - 1)]))
    for j, k in enumerate(range(0, n - 4, 2)):
        row = x[k] * x[k + 1] + x[k + 2]
        if j < CHAIN_HUB_ROWS:
            row = row + 0.05 * (hub * hub)
        p.eq(row, 0.3 + 0.2 * math.cos(k))
    for k in range(n - 2):
        if k % 3 == 0:
            p.le(x[k] * x[k] + x[k + 1] * x[k + 1], 4.0)
        elif k % 3 == 1:
            p.ge(x[k - 1] + x[k] - 2.0 * x[k + 1], -5.0)
        else:
            p.ge(x[k], -3.0)
    for j in range(CHAIN_HUB_ROWS):
        p.le(hub * hub + x[5 * j + 1] * x[5 * j + 1], 4.0)
    for k in range(n):
        p.le(x[k], 3.0)
    return p


MODELS = {"tiny": (tiny, tiny_start), "ineq_only": (ineq_only, ineq_only_start), "eq_only": (eq_only, eq_only_start)}


def make(m, name):
    """(problem, start) of "tiny", "ineq_only", "eq_only" or "chain<n>" on the backend of Model m"""
    if name.startswith("chain"):
        n = int(name[5:])
        return chain(m, n), chain_start(n)
    build, start = MODELS[name]
    return build(m), start()


def cost_terms(name, x):
    """The cost of model `name` at x as its terms in longdouble, each square and each product one term: an independent
    value of f (their sum) and of the magnitude a summation error is relative to (the sum of their absolute values)."""
    x = np.asarray(x, dtype=np.longdouble)
    h = np.longdouble
    if name == "tiny":
        return np.concatenate([(x - 1) ** 2, [h(0.5) * x[0] * x[2], h(0.25) * x[0] * x[1]]])
    if name == "ineq_only":
        return np.concatenate([(x - 1) ** 2, [x[0] * x[1], x[2] * x[3]]])
    if name == "eq_only":
        return np.concatenate([(x - h(0.5)) ** 2, [x[0] * x[1]]])
    if name.startswith("cart_pole"):  # the benchmark model (tests/support/models.py): J = sum u_k^2, u the last N variables
        N = int(name[9:])
        return x[4 * (N + 1):] ** 2
    n = int(name[5:])
    half_sin = np.array([0.5 * math.sin(k) for k in range(n)], dtype=np.longdouble)
    return np.concatenate([(x - half_sin) ** 2, h(0.1) * x[:-1] * x[1:]])
