"""What parameters as runtime inputs cost and save (profiles/parameters_cost.txt):

  sweep   the full tape sweep of 512 x cart-pole N=1000 with the shared constant pool against a pool per instance
          holding identical values (slpx_system_set_parameters): time per sweep (device events, slpx_system_time_step),
          the ratio, and the size of the per-instance pool;
  resolve wall time of set_parameters + solve() against set_value + solve() (the recompile) on cart-pole N=100 and
          N=1000 with the initial state as parameters: median of 6 after a warm-up (both paths solve the same two
          initial states three times each), every solve from the same start.

The model is the cart-pole swing-up of the benchmarks (tests/support/models/bench_models.hpp: the same dynamics, RK4
defects, bounds and cost) written through the expression C-ABI, with the four initial-state constants as parameters.

    python profiles/parameters_cost.py [sweep] [resolve]
"""
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tests.support import model  # noqa: E402


def dynamics(m, x, u):
    """bench_models.hpp cart_pole_dynamics: M(q) q'' = tau_g - C q' + B u, the 2 x 2 solve by Cramer's rule."""
    m_c, m_p, l, g = 5.0, 0.5, 0.5, 9.806
    theta, xdot, thetadot = x[1], x[2], x[3]
    m00, m01, m11 = m_c + m_p, m_p * l * m.cos(theta), m_p * l * l
    r0 = m_p * l * thetadot * m.sin(theta) * thetadot + u
    r1 = -m_p * g * l * m.sin(theta)
    det = m00 * m11 - m01 * m01
    return [xdot, thetadot, (r0 * m11 - m01 * r1) / det, (m00 * r1 - m01 * r0) / det]


def rk4(m, x, u, h):
    def axpy(a, k):
        return [xi + a * ki for xi, ki in zip(x, k)]
    k1 = dynamics(m, x, u)
    k2 = dynamics(m, axpy(0.5 * h, k1), u)
    k3 = dynamics(m, axpy(0.5 * h, k2), u)
    k4 = dynamics(m, axpy(h, k3), u)
    return [xi + h / 6.0 * (a + 2.0 * b + 2.0 * c + d) for xi, a, b, c, d in zip(x, k1, k2, k3, k4)]


def cart_pole(N, initial=(0.0, 0.0, 0.0, 0.0)):
    """-> (NlpProblem, parameter Vars): X (4 x N+1) row-major, then U (N), like the benchmark's model."""
    be = model.ProductBackend("gpu")
    be.reset()
    m = model.Model(be)
    p = model.NlpProblem(m)
    dt = 5.0 / N
    x_final = (1.0, math.pi, 0.0, 0.0)
    X = [[p.decision_variable(0.0) for _ in range(N + 1)] for _ in range(4)]
    for k in range(N + 1):
        X[0][k].set_value(k / N * x_final[0])
        X[1][k].set_value(k / N * x_final[1])
    U = [p.decision_variable(0.0) for _ in range(N)]
    x_initial = [m.variable(v) for v in initial]
    for i in range(4):
        p.eq(X[i][0], x_initial[i])
    for i in range(4):
        p.eq(X[i][N], x_final[i])
    for k in range(N + 1):
        p.bounds(0.0, X[0][k], 2.0)
    for k in range(N):
        p.bounds(-20.0, U[k], 20.0)
    for k in range(N):
        nxt = rk4(m, [X[i][k] for i in range(4)], U[k], dt)
        for i in range(4):
            p.eq(X[i][k + 1], nxt[i])
    J = None
    for k in range(N):
        J = U[k] * U[k] if J is None else J + U[k] * U[k]
    p.minimize(J)
    return p, x_initial


def sweep_cost(N=1000, B=512, iters=20):
    import sleipnir_amd as sa

    p, params = cart_pole(N)
    n, me, mi = p.p.dims
    system = sa.System(p.p, batch=B)
    rng = np.random.default_rng(20260928)
    x0 = p.p.get_x()
    x = x0[None, :] + 1e-2 * rng.uniform(-1, 1, (B, n))
    system.set_state(x=x, s=np.exp(rng.uniform(-2, 2, (B, mi))), y=rng.uniform(-1, 1, (B, me)),
                     z=np.exp(rng.uniform(-2, 2, (B, mi))), mu=np.full(B, 0.1))
    values = np.array([v.value() for v in params])
    n_p = len(values)
    assert p.p.parameters() == [v.node for v in params]
    shared, per = [], []
    for rep in range(5):  # alternating
        system.set_parameters(values, per_instance=False)
        shared.append(system.time_step(iters)["sweep"])
        V_shared = system.get("V")
        system.set_parameters(np.repeat(values[None, :], B, 0), per_instance=True)
        per.append(system.time_step(iters)["sweep"])
        assert np.array_equal(system.get("V"), V_shared)
    print(f"sweep {B} x cart-pole N={N} ({n_p} parameters): ms per sweep, {iters} sweeps per figure, alternating")
    print("  shared pool      :", " ".join(f"{t:.4f}" for t in shared), f" median {statistics.median(shared):.4f}")
    print("  pool per instance:", " ".join(f"{t:.4f}" for t in per), f" median {statistics.median(per):.4f}")
    print(f"  ratio per-instance / shared (medians): {statistics.median(per) / statistics.median(shared):.4f}")
    print(f"  spread of the shared figures: {(max(shared) - min(shared)) / statistics.median(shared):.2%}")
    print(f"  per-instance pools (full + values-only program): {system.parameter_pool_bytes()} bytes = "
          f"{system.parameter_pool_bytes() // (8 * B)} constants x {B} instances x 8 B")
    print(f"  tape nodes {system.info['tape_nodes']}, tasks {system.info['tape_tasks']}")
    system.close()
    p.p.close()


def resolve_cost(N, repeats=6):  # (even: both paths then solve r0 and r1 equally often)
    p, params = cart_pole(N)
    x_start = p.p.get_x()

    def solve():
        p.p.set_x(x_start)
        return p.p.solve()

    # Two initial states, r0 and r1, and both paths solve BOTH, so that the two medians are over the same solves (the
    # swing-up's iteration count moves a lot with the initial state).  The two whose solves succeed first among a few
    # candidates (these solves compile, load the code objects and warm up); where fewer than two succeed, the first two.
    tried = []
    for k in range(8):
        row = np.array([0.02 * k, 0.0, 0.0, 0.0])
        p.p.set_parameters(row)
        status, rep = solve()
        tried.append((status != 0, k, row, status, rep["iterations"]))
        if sum(1 for t in tried if not t[0]) == 2:
            break
    r0, r1 = (t[2] for t in sorted(tried, key=lambda t: t[:2])[:2])
    print(f"re-solve cart-pole N={N}, initial state = 4 parameters; candidates (cart position, status, iterations):",
          [(float(t[2][0]), t[3], t[4]) for t in tried])

    def by_parameters(row):
        p.p.set_parameters(row)

    def by_value(row):
        for v, value in zip(params, row):
            v.set_value(value)

    # every operation changes the values (r1, r0, r1, r0, ...), so every set_value compiles again; each path gets r0
    # and r1 in turn.  The first period is the warm-up.
    period = [(by_parameters, r1), (by_value, r0), (by_value, r1), (by_parameters, r0)]
    times = {by_parameters: [], by_value: []}
    records = {by_parameters: [], by_value: []}
    for k in range(1 + (repeats + 1) // 2):
        for change, row in period:
            count = p.p.compile_count()
            t0 = time.perf_counter()
            change(row)
            status, rep = solve()
            el = time.perf_counter() - t0
            assert p.p.compile_count() == count + (1 if change is by_value else 0)
            if k > 0:
                times[change].append(1e3 * el)
                records[change].append((float(row[0]), status, rep["iterations"]))
    t_param, t_value = times[by_parameters][:repeats], times[by_value][:repeats]
    print(f"  wall ms (host clock around a solve that ends synchronized), median of {repeats} after a warm-up, alternating")
    print("  set_parameters + solve:", " ".join(f"{t:.2f}" for t in t_param), f" median {statistics.median(t_param):.2f}",
          " (cart position, status, iterations)", records[by_parameters][:repeats])
    print("  set_value + solve     :", " ".join(f"{t:.2f}" for t in t_value), f" median {statistics.median(t_value):.2f}",
          " (cart position, status, iterations)", records[by_value][:repeats])
    print(f"  saved per re-solve (medians): {statistics.median(t_value) - statistics.median(t_param):.2f} ms, "
          f"ratio {statistics.median(t_value) / statistics.median(t_param):.2f}")
    p.p.close()


if __name__ == "__main__":
    what = sys.argv[1:] or ["sweep", "resolve"]
    if "sweep" in what:
        sweep_cost()
    if "resolve" in what:
        resolve_cost(100)
        resolve_cost(1000)
