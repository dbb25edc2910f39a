"""The models of the batched SQP / Newton tests (no inequality constraints), on either backend of tests.support.model:
small ones for the dense factorization branch, chains of about 300 variables for the sparse one.  Each builder returns
the NlpProblem; the starts are functions of a seed so that a test and the oracle check that chose the seeds agree."""
import numpy as np

from tests.support import model


def rosenbrock(m):
    """Unconstrained Rosenbrock in two variables; optimum (1, 1)."""
    p = model.NlpProblem(m)
    x, y = p.decision_variable(), p.decision_variable()
    p.minimize(100 * m.pow(y - m.pow(x, 2), 2) + m.pow(1 - x, 2))
    return p


def rosenbrock_starts():
    g = np.linspace(-1.5, 1.5, 6)
    return np.array([(a, b) for a in g for b in g])


def newton_chain(m, n=300):
    """min sum_k (x_k - sin k)^2 + sum_k cosh(x_{k+1} - x_k): strictly convex, tridiagonal Hessian."""
    p = model.NlpProblem(m)
    x = p.decision_variables(n)
    cost = m.pow(x[0] - np.sin(0.0), 2)
    for k in range(1, n):
        cost = cost + m.pow(x[k] - float(np.sin(k)), 2)
    for k in range(n - 1):
        cost = cost + m.cosh(x[k + 1] - x[k])
    p.minimize(cost)
    return p


def newton_chain_starts(B, n=300, seed=None):
    rng = np.random.default_rng(B if seed is None else seed)
    return 0.5 * rng.standard_normal((B, n))


def circle(m):
    """min (x - 2)^2 + (y - 1)^2 on the unit circle; optimum (2, 1) / sqrt 5."""
    p = model.NlpProblem(m)
    x, y = p.decision_variable(), p.decision_variable()
    p.minimize(m.pow(x - 2, 2) + m.pow(y - 1, 2))
    p.eq(m.pow(x, 2) + m.pow(y, 2), 1)
    return p


def circle_starts():
    g = [0.5, 1.0, 1.5, 2.0]
    return np.array([(a, b) for a in g for b in g])


def pendulum(m, N=100, dt=0.05):
    """Pendulum swing of N steps: theta_{k+1} = theta_k + dt omega_k, omega_{k+1} = omega_k + dt (u_k - sin theta_k),
    from rest at 0 to rest at theta = 1, cost sum u^2.  Variables [theta_0..N | omega_0..N | u_0..N-1]:
    n = 3 N + 2, m_e = 2 N + 4."""
    p = model.NlpProblem(m)
    th = p.decision_variables(N + 1)
    om = p.decision_variables(N + 1)
    u = p.decision_variables(N)
    for k in range(N):
        p.eq(th[k + 1], th[k] + dt * om[k])
        p.eq(om[k + 1], om[k] + dt * (u[k] - m.sin(th[k])))
    p.eq(th[0], 0)
    p.eq(om[0], 0)
    p.eq(th[N], 1)
    p.eq(om[N], 0)
    cost = u[0] * u[0]
    for k in range(1, N):
        cost = cost + u[k] * u[k]
    p.minimize(cost)
    return p


def pendulum_starts(B, N=100, seed=None):
    rng = np.random.default_rng(B if seed is None else seed)
    return 1e-2 * rng.standard_normal((B, 3 * N + 2))
