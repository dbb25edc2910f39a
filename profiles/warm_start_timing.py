"""What a warm start saves on the re-solve of an MPC loop (profiles/warm_start.txt):

  cart-pole swing-up N = 100 and N = 1000 (the benchmark's dynamics, RK4 defects, bounds and cost), the initial state
  four parameters.  One solve at the base initial state; then set_parameters() moves the initial state by 1 % and the
  problem is solved again, five times:
    cold  from the model's own start, as every solve did before warm starts (this mode uses nothing a build without
          them lacks: run it on the parent commit's build for the cold figures, `--root` names that checkout);
    warm  from the iterate the base solve ended at: solve(warm_start=problem.iterate()).
  Per re-solve: exit status, iterations, restorations, wall milliseconds around the solve (it ends synchronized); the
  median of the five.

The model is written through the public Python surface (sleipnir_amd.optimization, sleipnir_amd.autodiff).

    python profiles/warm_start_timing.py [--root DIR] [--base x,theta,xdot,thetadot] [cold] [warm] [N ...]
"""
import math
import statistics
import sys
import time
from pathlib import Path

args = sys.argv[1:]
root = Path(__file__).resolve().parents[1]
if "--root" in args:
    k = args.index("--root")
    root = Path(args[k + 1]).resolve()
    del args[k:k + 2]
base_arg = None
if "--base" in args:  # the base initial state: cart position, pole angle, their rates
    k = args.index("--base")
    base_arg = [float(v) for v in args[k + 1].split(",")]
    del args[k:k + 2]
sys.path.insert(0, str(root))

import numpy as np  # noqa: E402

from sleipnir_amd import autodiff as ad  # noqa: E402
from sleipnir_amd import optimization  # noqa: E402

BASE = np.array(base_arg if base_arg is not None else [0.1, 0.1, 0.0, 0.0])
MOVED = 1.01 * BASE
REPEATS = 5


def dynamics(x, u):
    m_c, m_p, l, g = 5.0, 0.5, 0.5, 9.806
    theta, xdot, thetadot = x[1], x[2], x[3]
    m00, m01, m11 = m_c + m_p, m_p * l * ad.cos(theta), m_p * l * l
    r0 = m_p * l * thetadot * ad.sin(theta) * thetadot + u
    r1 = -m_p * g * l * ad.sin(theta)
    det = m00 * m11 - m01 * m01
    return [xdot, thetadot, (r0 * m11 - m01 * r1) / det, (m00 * r1 - m01 * r0) / det]


def rk4(x, u, h):
    def axpy(a, k):
        return [xi + a * ki for xi, ki in zip(x, k)]
    k1 = dynamics(x, u)
    k2 = dynamics(axpy(0.5 * h, k1), u)
    k3 = dynamics(axpy(0.5 * h, k2), u)
    k4 = dynamics(axpy(h, k3), u)
    return [xi + h / 6.0 * (a + 2.0 * b + 2.0 * c + d) for xi, a, b, c, d in zip(x, k1, k2, k3, k4)]


def cart_pole(N):
    """-> (problem, its variables in order, their start values)"""
    p = optimization.Problem()
    dt = 5.0 / N
    x_final = (1.0, math.pi, 0.0, 0.0)
    X = [[p.decision_variable() for _ in range(N + 1)] for _ in range(4)]
    U = [p.decision_variable() for _ in range(N)]
    variables = [v for row in X for v in row] + U
    start = np.zeros(len(variables))
    for k in range(N + 1):
        start[k] = k / N * x_final[0]
        start[(N + 1) + k] = k / N * x_final[1]
    x_initial = []
    for v in BASE:
        q = ad.Variable()  # a free variable that is no decision variable: a parameter
        q.set_value(v)
        x_initial.append(q)
    for i in range(4):
        p.subject_to(X[i][0] == x_initial[i])
    for i in range(4):
        p.subject_to(X[i][N] == x_final[i])
    for k in range(N + 1):
        p.subject_to(X[0][k] >= 0.0)
        p.subject_to(X[0][k] <= 2.0)
    for k in range(N):
        p.subject_to(U[k] >= -20.0)
        p.subject_to(U[k] <= 20.0)
    for k in range(N):
        nxt = rk4([X[i][k] for i in range(4)], U[k], dt)
        for i in range(4):
            p.subject_to(X[i][k + 1] == nxt[i])
    J = None
    for k in range(N):
        J = U[k] * U[k] if J is None else J + U[k] * U[k]
    p.minimize(J)
    assert [v.node for v in p.parameters()] == [v.node for v in x_initial]
    return p, variables, start


def set_x(variables, values):
    for v, value in zip(variables, values):
        v.set_value(value)


def timed(solve):
    t0 = time.perf_counter()
    status = solve()
    return 1e3 * (time.perf_counter() - t0), status


def line(name, runs):
    ms = [r[0] for r in runs]
    print(f"  {name}: ms", " ".join(f"{t:.2f}" for t in ms), f" median {statistics.median(ms):.2f};",
          "(status, iterations, restorations)", [r[1:] for r in runs])


def run(N, modes):
    p, variables, start = cart_pole(N)
    record = lambda status: (int(status), p.report["iterations"], p.report["restorations"])
    p.set_parameters(BASE)
    set_x(variables, start)
    ms, status = timed(p.solve)
    print(f"cart-pole N={N}: base solve (compiles, loads the code objects): {ms:.1f} ms, (status, iterations, restorations) "
          f"{record(status)}")
    base_iterate = p.iterate() if hasattr(p, "iterate") else None
    if "cold" in modes:
        runs = []
        for _ in range(REPEATS + 1):
            p.set_parameters(MOVED)
            set_x(variables, start)
            ms, status = timed(p.solve)
            runs.append((ms,) + record(status))
        line("cold re-solve, initial state moved by 1 %", runs[1:])
    if "warm" in modes:
        runs = []
        for _ in range(REPEATS + 1):
            p.set_parameters(MOVED)
            ms, status = timed(lambda: p.solve(warm_start=base_iterate))
            runs.append((ms,) + record(status) + (p.warm_start_repaired(),))
        line("warm re-solve from the base solve's iterate (.., repaired)", runs[1:])
    p.close()


if __name__ == "__main__":
    modes = [a for a in args if a in ("cold", "warm")] or ["cold", "warm"]
    sizes = [int(a) for a in args if a.isdigit()] or [100, 1000]
    print("package:", root, " modes:", modes, " base initial state:", BASE.tolist())
    for N in sizes:
        run(N, modes)
