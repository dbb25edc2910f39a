"""What the full vjp — cotangents on x, s, y, z and the optimal cost — costs beside the vjp on x alone
(profiles/sensitivity_adjoint.txt):

  the cart-pole swing-up of profiles/warm_start_timing.py with N = 100, the initial state four parameters.  Medians of
  five (after one round that is not counted) of the wall time of
    sensitivity_vjp(array)            the cotangent on x alone (the old entry point, now the full vjp with vx alone)
    sensitivity_vjp(Cotangent(...))   all five cotangents
    cost_gradient()                   the cotangent 1 on the cost alone
    sensitivity()                     the Jacobian, n_p solves: the route to d cost/dp without the full vjp
  right after a solve and on the kept factorization, and of the batched pair at B = 64 and 512.
  Wall times are host clocks around calls that end synchronized (every one downloads its result).

    python profiles/sensitivity_adjoint_timing.py [B ...]
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

from sleipnir_amd import optimization  # noqa: E402

REPEATS = 5
N = 100
BASE = np.array([0.1, 0.1, 0.0, 0.0])


def wall_ms(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def fmt(values):
    return " ".join(f"{v:.3f}" for v in values) + f"   median {statistics.median(values):.3f}"


def single():
    wst.BASE = BASE
    p, variables, start = wst.cart_pole(N)
    p.set_parameters(BASE)
    wst.set_x(variables, start)
    status = p.solve()
    it = p.iterate()
    n, me, mi = p._p.dims
    print(f"cart-pole N={N}: n, m_e, m_i = {(n, me, mi)}, n_p = {len(BASE)}; base solve status {int(status)}, iterations {p.report['iterations']}")
    rng = np.random.default_rng(3)
    vx = np.linspace(-1.0, 1.0, n)
    full = optimization.Cotangent(x=vx, s=rng.uniform(-1, 1, mi), y=rng.uniform(-1, 1, me), z=rng.uniform(-1, 1, mi), cost=0.5)
    p.sensitivity()  # (the compile of the extended structure is not timed here)

    def again():  # a solve from its own iterate (no iteration): the kept factorization is dropped
        assert int(p.solve(warm_start=it)) == int(status)

    calls = {"vjp, x alone": lambda: p.sensitivity_vjp(vx), "vjp, all five cotangents": lambda: p.sensitivity_vjp(full),
             "cost_gradient": p.cost_gradient, "Jacobian (the n_p-solve route)": p.sensitivity}
    t = {(k, kept): [] for k in calls for kept in (False, True)}
    info = {}
    for rep in range(REPEATS + 1):
        for k, call in calls.items():
            again()
            a, _ = wall_ms(call)
            b, _ = wall_ms(call)
            if k != "Jacobian (the n_p-solve route)":
                assert p.sensitivity_info["factorizations"] == 0
                info[k] = p.sensitivity_info
            if rep > 0:
                t[(k, False)].append(a)
                t[(k, True)].append(b)
    for k in calls:
        print(f"  {k:32s} after a solve (ms)              {fmt(t[(k, False)])}")
        print(f"  {'':32s} on the kept factorization (ms)  {fmt(t[(k, True)])}")
    for k, i in info.items():
        print(f"  {k}: solves {i['solves']} refine_steps {i['refine_steps']} berr_max {i['berr_max']:.1e}")
    return p, it


def batched(p, it1, B):
    rng = np.random.default_rng(17)
    rows = np.repeat(BASE[None, :], B, axis=0)
    rows[:, :2] *= 1.0 + 0.01 * rng.uniform(-1.0, 1.0, (B, 2))
    n, me, mi = p._p.dims
    tile = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None, :], B, axis=0)
    warm = optimization.BatchIterate(x=tile(it1.x), s=tile(it1.s), y=tile(it1.y), z=tile(it1.z), mu=np.full(B, it1.mu))
    r = p.solve_batch(warm.x, parameters=rows, warm_start=warm)
    it = r.iterate
    print(f"B={B}: {sum(int(s) == 0 for s in r.status)} of {B} instances succeed")
    vx = np.repeat(np.linspace(-1.0, 1.0, n)[None, :], B, axis=0)
    full = optimization.Cotangent(x=vx, s=rng.uniform(-1, 1, (B, mi)), y=rng.uniform(-1, 1, (B, me)), z=rng.uniform(-1, 1, (B, mi)),
                                  cost=np.full(B, 0.5))
    calls = {"batched vjp, x alone": lambda: p.sensitivity_batch_vjp(it, rows, vx),
             "batched vjp, all five": lambda: p.sensitivity_batch_vjp(it, rows, full),
             "cost_gradient_batch": lambda: p.cost_gradient_batch(it, rows)}
    calls["batched vjp, x alone"]()  # (the compile of the extended batch system is not timed here)
    t = {(k, kept): [] for k in calls for kept in (False, True)}
    for rep in range(REPEATS + 1):
        for k, call in calls.items():
            p.solve_batch(it.x, parameters=rows, warm_start=it)  # (drops the kept factorization)
            a, _ = wall_ms(call)
            b, _ = wall_ms(call)
            assert p.sensitivity_info[0]["factorizations"] == 0
            if rep > 0:
                t[(k, False)].append(a)
                t[(k, True)].append(b)
    for k in calls:
        print(f"  {k:24s} after a solve_batch (ms)   {fmt(t[(k, False)])}")
        print(f"  {'':24s} kept factorization (ms)    {fmt(t[(k, True)])}")
    st = np.array(p.sensitivity_status)
    print(f"  status: {int(np.sum(st == 0))} computed, {int(np.sum(st == 1))} skipped, {int(np.sum(st == 2))} not factored")


if __name__ == "__main__":
    problem, iterate = single()
    for size in [int(a) for a in sys.argv[1:] if a.isdigit()] or [64, 512]:
        batched(problem, iterate, size)
    problem.close()
