"""What the solution sensitivities cost and what the tangent predictor saves (profiles/sensitivity.txt):

  the cart-pole swing-up of profiles/warm_start_timing.py, the initial state four parameters, N = 100 and N = 1000.
  Per size, the median of five (after one round that is not counted):
    compile   the first sensitivity call of a fresh problem: t_compile of its info (the extended structure: the model
              compiled once more with the parameters as variables, its tape kernels, the plan), a new problem per round
    factor    t_factor of a Jacobian call after a solve (the policy loop on the KKT system at the iterate)
    Jacobian, jvp, vjp   wall time of the call right after a solve (sweeps, assembly, factorization, solves) and of
              the same call again (on the kept factorization: the solves alone)
    central differences   wall time of the 2 n_p warm re-solves (p +- 1e-4 e_q from the base iterate, tolerance as the
              base solve) that the same Jacobian costs without this feature, on the same build
    predictor iterations of the re-solve after a 1 % move of the initial state, warm from the plain iterate and warm
              from iterate + jvp(dp)
  Wall times are host clocks around calls that end synchronized (every one downloads its result).

    python profiles/sensitivity_timing.py [N ...]
"""
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import numpy as np  # noqa: E402

_argv, sys.argv = sys.argv, sys.argv[:1]
import warm_start_timing as wst  # noqa: E402  (the model; it reads the command line on import)
sys.argv = _argv

REPEATS = 5
# the base initial states whose cold solves succeed (profiles/warm_start.txt)
BASES = {100: [0.1, 0.1, 0.0, 0.0], 1000: [0.101, 0.101, 0.0, 0.0]}


def wall_ms(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def med(values):
    return statistics.median(values)


def fmt(values):
    return " ".join(f"{v:.3f}" for v in values) + f"   median {med(values):.3f}"


def fresh_solved(N, base):
    wst.BASE = np.array(base)
    p, variables, start = wst.cart_pole(N)
    p.set_parameters(base)
    wst.set_x(variables, start)
    status = p.solve()
    return p, variables, int(status)


def run(N):
    base = np.array(BASES.get(N, BASES[100]))
    n_p = len(base)
    compile_ms, first_total_ms = [], []
    for r in range(REPEATS + 1):
        p, variables, status = fresh_solved(N, base)
        ms, s = wall_ms(p.sensitivity)
        if r > 0:
            compile_ms.append(1e3 * s.info["t_compile"])
            first_total_ms.append(ms)
        if r < REPEATS:
            p.close()
    it = p.iterate()
    print(f"cart-pole N={N}: n, m_e, m_i = {p._p.dims}, n_p = {n_p}; base solve status {status}, iterations {p.report['iterations']}")
    print(f"  first call, compile of the extended structure (ms): {fmt(compile_ms)}")
    print(f"  first call, whole Jacobian call (ms):               {fmt(first_total_ms)}")
    print(f"  info of the last: {s.info}")

    def again():  # a solve from its own iterate (no iteration): the kept factorization is dropped
        assert int(p.solve(warm_start=it)) == status

    dp = 0.01 * base
    v = np.linspace(-1.0, 1.0, len(it.x))
    rows = {k: [] for k in ("factor", "jac", "jac kept", "jvp", "jvp kept", "vjp", "vjp kept")}
    for r in range(REPEATS + 1):
        again()
        ms, s = wall_ms(p.sensitivity)
        ms2, _ = wall_ms(p.sensitivity)
        again()
        j1, _ = wall_ms(lambda: p.sensitivity_jvp(dp))
        j2, _ = wall_ms(lambda: p.sensitivity_jvp(dp))
        again()
        v1, _ = wall_ms(lambda: p.sensitivity_vjp(v))
        v2, _ = wall_ms(lambda: p.sensitivity_vjp(v))
        if r > 0:
            for k, t in zip(rows, (1e3 * s.info["t_factor"], ms, ms2, j1, j2, v1, v2)):
                rows[k].append(t)
    print(f"  factor (t_factor of the Jacobian call, ms):         {fmt(rows['factor'])}")
    print(f"  Jacobian, {n_p} solves: after a solve (ms)             {fmt(rows['jac'])}")
    print(f"                      on the kept factorization (ms)  {fmt(rows['jac kept'])}")
    print(f"  jvp, one solve:     after a solve (ms)              {fmt(rows['jvp'])}")
    print(f"                      on the kept factorization (ms)  {fmt(rows['jvp kept'])}")
    print(f"  vjp, one solve:     after a solve (ms)              {fmt(rows['vjp'])}")
    print(f"                      on the kept factorization (ms)  {fmt(rows['vjp kept'])}")
    print(f"  last info: delta {s.info['delta']:.1e} gamma {s.info['gamma']:.1e} inertia ({s.info['n_pos']}, {s.info['n_neg']}, {s.info['n_zero']}) "
          f"berr_max {s.info['berr_max']:.1e} solves {s.info['solves']} refine_steps {s.info['refine_steps']}")

    # the same Jacobian by central differences of warm re-solves
    fd_ms, fd_counts = [], None
    h = 1e-4
    for r in range(REPEATS + 1):
        counts = []
        t0 = time.perf_counter()
        ends = []
        for q in range(n_p):
            for sign in (1.0, -1.0):
                row = base.copy()
                row[q] += sign * h
                p.set_parameters(row)
                st = p.solve(warm_start=it)
                counts.append((int(st), p.report["iterations"]))
                ends.append(p.iterate().x)
        total = 1e3 * (time.perf_counter() - t0)
        if r > 0:
            fd_ms.append(total)
        fd_counts = counts
    fd = np.array([(ends[2 * q] - ends[2 * q + 1]) / (2 * h) for q in range(n_p)])
    p.set_parameters(base)
    again()
    jac = p.sensitivity()
    scale = np.max(np.abs(jac.dx), axis=1)
    print(f"  central differences, {2 * n_p} warm re-solves (ms):       {fmt(fd_ms)}   (status, iterations) {fd_counts}")
    print(f"  dx against them, per parameter, relative to the column's largest entry: "
          f"{' '.join(f'{e:.1e}' for e in np.max(np.abs(jac.dx - fd), axis=1) / scale)}")

    # the predictor: the initial state moves by 1 %
    moved = 1.01 * base
    again()
    tangent = p.sensitivity_jvp(moved - base)
    p.set_parameters(moved)
    st_plain = int(p.solve(warm_start=it))
    plain = (st_plain, p.report["iterations"], p.warm_start_repaired())
    x_plain = p.iterate().x
    p.set_parameters(moved)
    st_pred = int(p.solve(warm_start=it + tangent))
    pred = (st_pred, p.report["iterations"], p.warm_start_repaired())
    print(f"  re-solve after a 1 % move, warm from the iterate:        (status, iterations, repaired) {plain}")
    print(f"  re-solve after a 1 % move, warm from iterate + jvp(dp):  (status, iterations, repaired) {pred}; "
          f"|x - x of the other| {np.max(np.abs(p.iterate().x - x_plain)):.2e}; "
          f"the predictor's own distance to it {np.max(np.abs((it + tangent).x - x_plain)):.2e}, the plain iterate's {np.max(np.abs(it.x - x_plain)):.2e}")
    p.close()


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [100, 1000]
    for N in sizes:
        run(N)
