"""Wall time of Problem.solve_batch on models without inequality constraints: the n = 300 Newton chain (solved to
1e-6, see tests/test_solve_batch_eq_gpu.py) and the N = 100 pendulum SQP chain, at B in {1, 16, 64, 512}.  Median of
5 runs after one warm-up run (which also compiles the batch system), no profiler attached.

    python profiles/eq_batch_timing.py          # prints one table

Run on two commits, the tables side by side are profiles/eq_batch_timing.txt."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tests.support import eq_models, model  # noqa: E402


def main():
    be = model.ProductBackend("gpu")
    be.reset()
    m = model.Model(be)
    cases = [("newton n=300", eq_models.newton_chain(m).p, eq_models.newton_chain_starts, {"tolerance": 1e-6}),
             ("sqp N=100", eq_models.pendulum(m).p, eq_models.pendulum_starts, {})]
    print(f"{'model':<14}{'B':>5}{'median ms':>12}{'min ms':>10}{'max ms':>10}{'iterations':>12}{'ok':>5}")
    for name, p, starts, kw in cases:
        for B in (1, 16, 64, 512):
            x0 = starts(B)
            r = p.solve_batch(x0, **kw)  # warm-up
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                r = p.solve_batch(x0, **kw)
                t.append(1e3 * (time.perf_counter() - t0))
            ok = int(np.sum(np.asarray(r["status"]) == 0))
            print(f"{name:<14}{B:>5}{statistics.median(t):>12.2f}{min(t):>10.2f}{max(t):>10.2f}"
                  f"{int(np.sum(r['iterations'])):>12}{ok:>5}", flush=True)


if __name__ == "__main__":
    main()
