"""Wall time of Problem.solve_batch on batches whose instances enter feasibility restoration, under both restoration modes:
"handoff" (an instance runs its restoration on the batch-1 system while the batch waits; the default) and "lockstep" (the
instances that ask in one round share one restoration phase on the batch system), with the sum of the single solves of the
same starts beside them.

    python profiles/batch_restoration_timing.py [OUT.txt]        # -> the text of profiles/batch_restoration_timing.txt

Workloads: the model and the six starts of tests/test_solve_batch_gpu.py::test_restoration_inside_a_batch tiled to B = 96;
the cart-pole swing-up at N = 200 (bench.py's model) from the benchmark's guess with 1e-3 perturbations, B = 16 and B = 64.
Per run: median, min and max of 3 solve_batch calls after one warm-up (which compiles the batch system), no profiler
attached; the statuses, how many instances restored and how often, the iterations, and the lockstep layer's own counters
(instances, phases, rounds, fallbacks to the batch-1 system)."""
import statistics
import sys
import time
from collections import Counter
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

REPEATS = 3


def _workloads():
    import sleipnir_amd
    from tests.support import model, models

    sleipnir_amd.lib().slpx_graph_reset()
    be = model.ProductBackend("gpu")
    be.reset()
    m = model.Model(be)
    p = model.NlpProblem(m)
    x, s1, s2 = p.decision_variable(-2), p.decision_variable(3), p.decision_variable(1)
    p.minimize(x)
    p.eq(m.pow(x, 2) - s1 - 1, 0)
    p.eq(x - s2 - 0.5, 0)
    p.ge(s1, 0)
    p.ge(s2, 0)
    six = np.array([[x0, 3.0, 1.0] for x0 in (-4.0, -3.0, -2.0, -1.5, 0.0, 2.0)])
    out = [("six starts x 16", p.p, np.tile(six, (16, 1)))]
    N = 200
    cart = models.cart_pole(N, 5.0 / N)
    base = cart.get_x()
    for B in (16, 64):
        out.append((f"cart-pole N={N}", cart, base * (1.0 + 1e-3 * np.random.default_rng(B).standard_normal((B, base.size)))))
    return out


def _statuses(status):
    return ", ".join(f"{k}: {v}" for k, v in sorted(Counter(int(s) for s in status).items(), reverse=True))


def main(path=None):
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("solve_batch on restoring batches: restoration by hand-off and in lockstep (ms; median, min, max of "
        f"{REPEATS} after a warm-up)")
    for name, p, x0 in _workloads():
        B = len(x0)
        say()
        say(f"{name}, B = {B}")
        results = {}
        for mode in ("handoff", "lockstep"):
            r = p.solve_batch(x0, restoration=mode)  # (the warm-up)
            t = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                r = p.solve_batch(x0, restoration=mode)
                t.append(1e3 * (time.perf_counter() - t0))
            results[mode] = r
            fr = r["restoration_lockstep"]
            say(f"  {mode:<9}{statistics.median(t):>10.1f}{min(t):>10.1f}{max(t):>10.1f}   statuses {{{_statuses(r['status'])}}}  "
                f"instances that restored {int(np.sum(r['restorations'] > 0))}, restorations {int(np.sum(r['restorations']))}, "
                f"iterations {int(np.sum(r['iterations']))} (restoration {r['report']['restoration_iterations']}), outer rounds {r['rounds']}, "
                f"hand-offs {r['handoffs']}; lockstep: instances {fr['instances']}, phases {fr['phases']}, rounds {fr['rounds']}, "
                f"fallbacks {fr['fallbacks']}")
        a, b = results["handoff"], results["lockstep"]
        say(f"  the two modes: statuses {'equal' if np.array_equal(a['status'], b['status']) else 'DIFFERENT'}, restoration counts "
            f"{'equal' if np.array_equal(a['restorations'], b['restorations']) else 'DIFFERENT'}, iteration counts "
            f"{'equal' if np.array_equal(a['iterations'], b['iterations']) else 'DIFFERENT'}, max |x_lockstep - x_handoff| "
            f"{float(np.nanmax(np.abs(a['x'] - b['x']))):.3g}")
        t_single, st_single, restored = 0.0, [], 0
        p.set_x(x0[0])
        p.solve()  # (the warm-up)
        for row in x0:
            p.set_x(row)
            t0 = time.perf_counter()
            status, rep = p.solve()
            t_single += 1e3 * (time.perf_counter() - t0)
            st_single.append(status)
            restored += int(rep.get("restorations", 0) > 0)
        say(f"  singles  {t_single:>10.1f}   the sum of {B} single solves, one run each; statuses {{{_statuses(st_single)}}}, "
            f"instances that restored {restored}")
    if path:
        Path(path).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
