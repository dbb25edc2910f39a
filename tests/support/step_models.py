"""General models for the tests of the fused Newton step (tests/test_step_general_models_cpu.py, _gpu.py), on either
backend of tests.support.model: fr_models.chain(n), and hub(n, he, hi), whose last variable is in `he` equality rows and
`hi` inequality rows.  The hub's row of the right-hand side then sums one gradient term, `he` terms of A_e^T y and `hi`
of A_i^T; the matrix entry (hub, hub) its direct terms and `hi` products; and the hub's column of A_i sends `hi`
back-substitution rows into whatever task owns the hub.  With he and hi the models stand on either side of the limits
of the packers (csrc/device_images.cpp).  Smooth, with independent constraint gradients at the start.

TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

from tests.support import fr_models, model


def hub_start(n):
    x = 0.5 + 0.3 * np.sin(0.7 * np.arange(n))
    x[n - 1] = 0.4  # the hub
    return x


def hub(m, n, he, hi):
    """n variables, the last one the hub h.
    Equalities, j < he: x_2j x_{2j+1} + x_{2j+2} + 0.05 h^2 = 0.3 + 0.2 cos(2j) (column 2j + 1 is in row j only and
    x_2j != 0 at the start: independent gradients).
    Inequalities: h^2 + x_j^2 <= 4 for j < hi, then x_k <= 3 for every k < n - 1 (plain bounds): m_i = hi + n - 1.
    Cost: sum (x_k - sin(k) / 2)^2 + 0.1 sum x_k x_{k+1}."""
    assert 2 * he + 2 <= n - 1 and hi <= n - 1
    p = model.NlpProblem(m)
    x = [p.decision_variable(v) for v in hub_start(n)]
    h = x[n - 1]
    p.minimize(fr_models._sum([(x[k] - 0.5 * math.sin(k)) * (x[k] - 0.5 * math.sin(k)) for k in range(n)])
               + 0.1 * fr_models._sum([x[k] * x[k + 1] for k in range(n - 1)]))
    for j in range(he):
        p.eq(x[2 * j] * x[2 * j + 1] + x[2 * j + 2] + 0.05 * (h * h), 0.3 + 0.2 * math.cos(2 * j))
    for j in range(hi):
        p.le(h * h + x[j] * x[j], 4.0)
    for k in range(n - 1):
        p.le(x[k], 3.0)
    return p


def make(m, name):
    """(problem, start) of "chain<n>" (fr_models) or "hub<n>_<he>_<hi>" on the backend of Model m"""
    if name.startswith("chain"):
        return fr_models.make(m, name)
    n, he, hi = (int(v) for v in name[3:].split("_"))
    return hub(m, n, he, hi), hub_start(n)


# Models and seeds of indefinite_state: states at which the oracle's loop climbs to delta = 1 (the chains, six
# factorizations) or 10 (the hubs, seven).  tests/test_step_general_models_cpu.py shows that none stands on a borderline.
INDEFINITE = {"chain130": 1, "chain300": 1, "hub40_3_3": 0, "hub530_255_127": 0, "hub530_256_127": 0, "hub2300_1100_1000": 0}


def indefinite_state(name, x0, n, m_e, m_i, d_f):
    """cases.newton_state's interior state of seed cases.SEED + INDEFINITE[name] with the multipliers of the equality
    rows eight times as large: the rows' Hessians, y_j [[0, 1], [1, 0]] on (x_2j, x_2j+1), then outweigh the cost's 2 d_f
    on the diagonal, the Lagrangian's Hessian is indefinite and the policy loop has to climb its ladder."""
    from tests.support import cases

    x, s, y, z, mu = cases.newton_state("interior", x0, n, m_e, m_i, d_f, seed=cases.SEED + INDEFINITE[name])
    return x, s, 8.0 * y, z, mu


def build_both(name):
    """model `name` in the oracle and in the product, each on a graph of its own just reset"""
    mo = model.Model(model.OracleBackend())
    mo.be.reset()
    mp = model.Model(model.ProductBackend("hostcheck"))
    mp.be.reset()
    return make(mo, name)[0], make(mp, name)[0]
