"""What the batched solution sensitivities cost against the route without them (profiles/sensitivity_batch.txt):

  the cart-pole swing-up of profiles/warm_start_timing.py with N = 100, the initial state four parameters; B = 64 and 512
  instances whose initial states are spread by up to 1 % around the base.  Per B, the median of five (after one round
  that is not counted):
    compile     the first batched call of a fresh problem: t_compile of its info (the extended system compiled for B)
    solve_batch the batch the iterates come from (warm from the previous batch's iterates), for scale
    vjp, jvp, Jacobian   wall time of the batched call right after a solve_batch (sweeps, assembly, factorization, one
                round of solves — n_p rounds for the Jacobian) and of the same call again (on the kept factorization)
    sequential  B times (set_parameters, warm solve, sensitivity_vjp) on one problem: the route that exists without
                the batched calls
  and a check that the batched vjp agrees with the sequential one on every instance.
  Wall times are host clocks around calls that end synchronized (every one downloads its result).

    python profiles/sensitivity_batch_timing.py [B ...]
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

REPEATS = 5  # (medians of five; the smallest is printed beside them)
N = 100
BASE = np.array([0.1, 0.1, 0.0, 0.0])


def wall_ms(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def fmt(values):
    return " ".join(f"{v:.2f}" for v in values) + f"   median {statistics.median(values):.2f}  min {min(values):.2f}"


def rows_for(B):
    rng = np.random.default_rng(17)
    rows = np.repeat(BASE[None, :], B, axis=0)
    rows[:, :2] *= 1.0 + 0.01 * rng.uniform(-1.0, 1.0, (B, 2))
    return rows


def run(B):
    wst.BASE = BASE
    rows = rows_for(B)
    n_p = rows.shape[1]
    p, variables, start = wst.cart_pole(N)
    p.set_parameters(BASE)
    wst.set_x(variables, start)
    status = p.solve()
    it1 = p.iterate()
    n = len(it1.x)
    print(f"cart-pole N={N}, B={B}: n, m_e, m_i = {p._p.dims}, n_p = {n_p}; base solve status {int(status)}, iterations {p.report['iterations']}")
    # the batch, warm from the base iterate in every instance
    tile = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None, :], B, axis=0)
    warm = optimization.BatchIterate(x=tile(it1.x), s=tile(it1.s), y=tile(it1.y), z=tile(it1.z), mu=np.full(B, it1.mu))
    r = p.solve_batch(warm.x, parameters=rows, warm_start=warm)
    ok = sum(int(s) == 0 for s in r.status)
    print(f"  solve_batch: {ok} of {B} instances succeed, iterations {int(np.min(r.iterations))}..{int(np.max(r.iterations))}")
    it = r.iterate
    v = np.repeat(np.linspace(-1.0, 1.0, n)[None, :], B, axis=0)
    dp = 0.01 * rows

    def again():  # the batch from its own iterates: the kept factorization is dropped
        return p.solve_batch(it.x, parameters=rows, warm_start=it)

    t = {k: [] for k in ("compile", "solve_batch", "vjp", "vjp kept", "jvp", "jvp kept", "jac", "jac kept", "factor")}
    first_ms, g = wall_ms(lambda: p.sensitivity_batch_vjp(it, rows, v))
    t_compile = 1e3 * p.sensitivity_info[0]["t_compile"]
    print(f"  first batched call (ms): {first_ms:.1f}, of which the compile of the extended batch system {t_compile:.1f}")
    for rep in range(REPEATS + 1):
        sb_ms, _ = wall_ms(again)
        v1, grad = wall_ms(lambda: p.sensitivity_batch_vjp(it, rows, v))
        info = p.sensitivity_info[0]
        v2, _ = wall_ms(lambda: p.sensitivity_batch_vjp(it, rows, v))
        assert p.sensitivity_info[0]["factorizations"] == 0
        again()
        j1, _ = wall_ms(lambda: p.sensitivity_batch_jvp(it, rows, dp))
        j2, _ = wall_ms(lambda: p.sensitivity_batch_jvp(it, rows, dp))
        again()
        a1, jac = wall_ms(lambda: p.sensitivity_batch(it, rows))
        a2, _ = wall_ms(lambda: p.sensitivity_batch(it, rows))
        if rep > 0:
            for k, ms in zip(t, (0.0, sb_ms, v1, v2, j1, j2, a1, a2, 1e3 * info["t_factor"])):
                t[k].append(ms)
    status = np.array(p.sensitivity_status)
    print(f"  solve_batch from its own iterates (ms):              {fmt(t['solve_batch'])}")
    print(f"  factor (t_factor of the vjp call, ms):               {fmt(t['factor'])}")
    print(f"  batched vjp, one round:  after a solve_batch (ms)    {fmt(t['vjp'])}")
    print(f"                           kept factorization (ms)     {fmt(t['vjp kept'])}")
    print(f"  batched jvp, one round:  after a solve_batch (ms)    {fmt(t['jvp'])}")
    print(f"                           kept factorization (ms)     {fmt(t['jvp kept'])}")
    print(f"  batched Jacobian, {n_p} rounds: after a solve_batch (ms) {fmt(t['jac'])}")
    print(f"                           kept factorization (ms)     {fmt(t['jac kept'])}")
    print(f"  status: {int(np.sum(status == 0))} computed, {int(np.sum(status == 1))} skipped, {int(np.sum(status == 2))} not factored; "
          f"info of instance 0: delta {info['delta']:.1e} gamma {info['gamma']:.1e} inertia ({info['n_pos']}, {info['n_neg']}, {info['n_zero']}) "
          f"berr_max {info['berr_max']:.1e} solves {info['solves']} refine_steps {info['refine_steps']} factorizations {info['factorizations']}")

    # the route without the batched calls: instance by instance on the one problem
    seq_ms, seq_grad = [], None
    for rep in range(2 if B > 64 else REPEATS + 1):  # (B = 512: one counted round is 512 solves)
        grads = np.zeros((B, n_p))
        t0 = time.perf_counter()
        for b in range(B):
            p.set_parameters(rows[b])
            p.solve(warm_start=it1)
            grads[b] = p.sensitivity_vjp(v[b])
        total = 1e3 * (time.perf_counter() - t0)
        if rep > 0:
            seq_ms.append(total)
        seq_grad = grads
    p.set_parameters(BASE)
    med_seq, med_vjp = statistics.median(seq_ms), statistics.median(t["vjp"])
    print(f"  sequential, {B} x (set_parameters, warm solve, sensitivity_vjp) (ms): {fmt(seq_ms)}   = {med_seq / B:.3f} per instance")
    print(f"  ratio sequential / (solve_batch + batched vjp): {med_seq / (statistics.median(t['solve_batch']) + med_vjp):.1f}; "
          f"sequential / batched vjp alone: {med_seq / med_vjp:.1f}")
    scale = np.maximum(np.max(np.abs(seq_grad), axis=1), 1e-300)
    print(f"  batched vjp against the sequential one, worst instance, relative to its largest entry: "
          f"{np.max(np.max(np.abs(grad - seq_grad), axis=1) / scale):.2e}")
    p.close()


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [64, 512]
    for B in sizes:
        run(B)
