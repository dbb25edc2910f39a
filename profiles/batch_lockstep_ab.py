"""A/B record of Problem.solve_batch for a refactor of the batched drivers that must not change a bit: a fixed list of
batches of every driver (interior point, SQP, Newton), every output array and integer counter of each, two single
Newton solves, and the wall time of the larger batches.

    python profiles/batch_lockstep_ab.py run OUT.npz        # on each of the two commits, same machine
    python profiles/batch_lockstep_ab.py compare A.npz B.npz  # A = parent, B = head -> the text of batch_lockstep_ab.txt

`compare` wants every array equal element for element (NaNs equal to NaNs); the timers of the report and the wall
times (keys under time/) are not compared.  Speed: median, min, max of 5 solve_batch calls after one warm-up, no
profiler attached; the head's median may exceed the parent's by at most the parent's own spread (max - min)."""
import hashlib
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

FIELDS = ("status", "x", "s", "y", "z", "cost", "iterations", "restorations")
STATS = ("rounds", "handoffs", "driver")
REPORT = ("iterations", "factorizations", "solves", "value_sweeps", "restorations", "restoration_iterations", "delta", "gamma",
          "final_error")


def _grid(lo, hi, step):
    out, k = [], 0
    while lo + k * step < hi - 1e-12:
        out.append(lo + k * step)
        k += 1
    return out


def _with_nans(x0):
    x0 = x0.copy()
    x0[[3, 5]] = np.nan
    return x0


def _cases():
    """(name, Problem, starts, solve_batch keywords, timed)"""
    import sleipnir_amd
    from tests.support import eq_models, model, models

    sleipnir_amd.lib().slpx_graph_reset()
    be = model.ProductBackend("gpu")
    be.reset()
    m = model.Model(be)
    out = []

    # interior point
    N, dt = 50, 0.005
    fly = models.flywheel(N, dt)
    base = fly.get_x()

    def fly_starts(B):
        return base + 1e-3 * np.random.default_rng(B).standard_normal((B, base.size))

    out += [("ipm/flywheel_B7", fly, fly_starts(7), {}, False), ("ipm/flywheel_B70", fly, fly_starts(70), {}, True)]
    p = model.NlpProblem(m)
    x, s1, s2 = p.decision_variable(-2), p.decision_variable(3), p.decision_variable(1)
    p.minimize(x)
    p.eq(m.pow(x, 2) - s1 - 1, 0)
    p.eq(x - s2 - 0.5, 0)
    p.ge(s1, 0)
    p.ge(s2, 0)
    out.append(("ipm/restoration_6", p.p, np.array([[x0, 3.0, 1.0] for x0 in (-4.0, -3.0, -2.0, -1.5, 0.0, 2.0)]), {}, False))
    p = model.NlpProblem(m)
    x, y = p.decision_variable(), p.decision_variable()
    p.minimize(m.pow(1 - x, 2) + 100 * m.pow(y - m.pow(x, 2), 2))
    p.le(m.pow(x, 2) + m.pow(y, 2), 2)
    g = _grid(-1.5, 1.5, 0.1)
    out.append(("ipm/rosenbrock_disk_900", p.p, np.array([(a, b) for a in g for b in g]), {}, True))

    # SQP
    pend = eq_models.pendulum(m).p
    out += [("sqp/pendulum_B7", pend, eq_models.pendulum_starts(7), {}, False),
            ("sqp/pendulum_B70", pend, eq_models.pendulum_starts(70), {}, True),
            ("sqp/circle_16", eq_models.circle(m).p, eq_models.circle_starts(), {}, False)]

    # Newton
    chain, kw = eq_models.newton_chain(m).p, {"tolerance": 1e-6}
    rosen = eq_models.rosenbrock(m).p
    out += [("newton/chain_B7", chain, eq_models.newton_chain_starts(7), kw, False),
            ("newton/chain_B70", chain, eq_models.newton_chain_starts(70), kw, True),
            ("newton/rosenbrock_36", rosen, eq_models.rosenbrock_starts(), {}, False)]

    # NaN starts at slots 3 and 5 of 7
    out += [("ipm/flywheel_B7_nan", fly, _with_nans(fly_starts(7)), {}, False),
            ("sqp/pendulum_B7_nan", pend, _with_nans(eq_models.pendulum_starts(7)), {}, False),
            ("newton/chain_B7_nan", chain, _with_nans(eq_models.newton_chain_starts(7)), kw, False)]
    singles = [("single/newton_rosenbrock", rosen, eq_models.rosenbrock_starts()[0], {}),
               ("single/newton_chain", chain, eq_models.newton_chain_starts(7)[0], kw)]
    return out, singles


def run(path):
    cases, singles = _cases()
    rec = {}
    for name, p, x0, kw, timed in cases:
        r = p.solve_batch(x0, **kw)  # (the warm-up of the timed runs: it compiles the batch system)
        for k in FIELDS:
            rec[f"{name}/{k}"] = np.asarray(r[k])
        for k in STATS:
            rec[f"{name}/{k}"] = np.asarray(r[k])
        for k in REPORT:
            rec[f"{name}/report.{k}"] = np.asarray(r["report"][k])
        print(f"{name:<26} B {len(x0):>4}  ok {int(np.sum(r['status'] == 0)):>4}  rounds {r['rounds']:>4}  "
              f"handoffs {r['handoffs']}", flush=True)
        if timed:
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                p.solve_batch(x0, **kw)
                t.append(1e3 * (time.perf_counter() - t0))
            rec[f"time/{name}"] = np.array(t)
    for name, p, x0, kw in singles:
        p.set_x(x0)
        status, rep = p.solve(**kw)
        rec[f"{name}/status"] = np.asarray(status)
        rec[f"{name}/x"] = p.get_x()
        for k in ("iterations", "factorizations", "value_sweeps"):
            rec[f"{name}/{k}"] = np.asarray(rep[k])
        print(f"{name:<26} status {status}  iterations {rep['iterations']}", flush=True)
    np.savez(path, **rec)
    _print_times(rec)


def _print_times(rec):
    print(f"{'case':<26}{'median ms':>12}{'min ms':>10}{'max ms':>10}")
    for k in sorted(rec):
        if k.startswith("time/"):
            t = rec[k]
            print(f"{k[5:]:<26}{statistics.median(t):>12.2f}{min(t):>10.2f}{max(t):>10.2f}")


def _digest(rec):
    """sha256 of the compared arrays (an .npz file's own hash moves with the time stamps inside it)"""
    h = hashlib.sha256()
    for k in sorted(rec):
        if not k.startswith("time/"):
            a = np.ascontiguousarray(rec[k])
            h.update(f"{k}:{a.dtype}:{a.shape}".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def compare(path_a, path_b):
    a, b = dict(np.load(path_a)), dict(np.load(path_b))
    for tag, path, rec in (("parent", path_a, a), ("head", path_b, b)):
        print(f"{tag}: {Path(path).name}  sha256 {hashlib.sha256(Path(path).read_bytes()).hexdigest()}")
        print(f"{'':<{len(tag)}}  compared arrays: sha256 {_digest(rec)}")
    keys = sorted(k for k in set(a) | set(b) if not k.startswith("time/"))
    different = [k for k in keys if k not in a or k not in b or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or
                 not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]
    print(f"\n{len(keys)} arrays compared, {len(different)} different")
    for k in different:
        print(f"  DIFFERENT: {k}")
    print("VERDICT (bits): " + ("every array equal element for element" if not different else "NOT EQUAL"))
    slower = []
    for tag, rec in (("parent", a), ("head", b)):
        print(f"\nwall time of solve_batch, {tag}:")
        _print_times(rec)
    print()
    for k in sorted(k for k in a if k.startswith("time/") and k in b):
        spread = float(np.max(a[k]) - np.min(a[k]))
        excess = statistics.median(b[k]) - statistics.median(a[k])
        print(f"{k[5:]:<26} head median - parent median {excess:>8.2f} ms; parent's spread {spread:>8.2f} ms")
        if excess > spread:
            slower.append(k[5:])
    print("VERDICT (speed): " + ("no case slower than the parent by more than the parent's spread" if not slower else
                                 "SLOWER: " + ", ".join(slower)))
    return 1 if different or slower else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
