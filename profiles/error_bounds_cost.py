#!/usr/bin/env python3
"""What slpx_ldlt_error_bounds and slpx_ldlt_condest cost, next to one slpx_ldlt_solve on the same system: cart-pole
N = 1000 at the suite's interior state, one problem and a batch of 512.  The expected cost is (solves x one solve) plus
the launches of a round (fill, reduce, fold) and its download; berr alone takes no solve.  Also berr / ferr / cond1
before and after refine(1) at that state — the state behind VERDICT.md's "19.6x farther from the refined solution".
    PYTHONPATH=$PWD python profiles/error_bounds_cost.py > profiles/error_bounds_cost.txt"""
import time

import numpy as np

import sleipnir_amd as sa
from tests.support import cases, models

N = 1000


def best_of(fn, reps, inner=1):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            out = fn()
        best = min(best, (time.perf_counter() - t0) / inner)
    return best, out


for B in (1, 512):
    sa.lib().slpx_graph_reset()
    pp = models.cart_pole(N, 5.0 / N)
    sy = sa.System(pp, batch=B, device=0)
    n, me, mi = sy.info["n"], sy.info["m_e"], sy.info["m_i"]
    x, s, y, z, mu = cases.newton_state("interior", pp.get_x(), n, me, mi, 1.0)
    sy.set_scaling(np.ones(1 + me + mi))
    sy.set_state(np.tile(x, B), np.tile(s, B), np.tile(y, B), np.tile(z, B), np.full(B, mu))
    sy.reset_regularization()
    assert np.all(sy.newton_step(True) == 0)
    reg = sy.regularization()[0]
    for _ in range(3):  # (first calls allocate)
        sy.error_bounds()
        sy.condest()
    inner = 100 if B == 1 else 10

    def solves():
        sy.solve()
        sy.sync()

    sy.get("rhs")  # (the system materialized: a solve of the right-hand side in memory from here on)
    for _ in range(10):
        sy.solve()
    sy.sync()
    t_solve, _ = best_of(solves, 5, inner)
    t_berr, _ = best_of(lambda: sy.error_bounds(forward=False), 5, 10)
    t_eb, eb = best_of(sy.error_bounds, 5, 3)
    t_ce, ce = best_of(sy.condest, 5, 3)
    k_eb, k_ce = int(eb["solves"][0]), int(ce["solves"][0])
    print(f"cart-pole N={N}, batch {B}, dim {n + me}, (delta, gamma) = ({reg[0]:g}, {reg[1]:g})")
    print(f"  one slpx_ldlt_solve (launch + wait)        {1e6 * t_solve:10.1f} us")
    print(f"  error_bounds, berr alone (no solve)        {1e6 * t_berr:10.1f} us")
    print(f"  error_bounds with ferr: {k_eb:2d} solves          {1e6 * t_eb:10.1f} us = {k_eb} x solve + {1e6 * (t_eb - t_berr - k_eb * t_solve) / k_eb:.1f} us per round")
    print(f"  condest:                {k_ce:2d} solves          {1e6 * t_ce:10.1f} us = {k_ce} x solve + {1e6 * (t_ce - k_ce * t_solve) / k_ce:.1f} us per round")
    if B == 1:
        over = (t_ce - k_ce * t_solve) / k_ce
        print(f"  per-round overhead {'EXCEEDS' if over > t_solve else 'is below'} the solve itself at batch 1 ({1e6 * over:.1f} us against {1e6 * t_solve:.1f} us)")
        cp, ri = sy.pattern(5)
        Kreg = cases.regularized(cp, ri, sy.get("lhs")[0], n, reg[0], reg[1])
        p_true = cases.refined_solution(cp, ri, Kreg, sy.get("rhs")[0], steps=6)
        true = lambda: float(np.max(np.abs(sy.get("p")[0] - p_true)) / np.max(np.abs(sy.get("p")[0])))
        sy.solve()  # (p of the right-hand side in memory again)
        for label in ("raw solve", "after refine(1)"):
            eb, ce = sy.error_bounds(), sy.condest()
            print(f"  {label:16s} berr {eb['berr'][0]:.3e}  ferr {eb['ferr'][0]:.3e} ({int(eb['solves'][0])} solves)  true error {true():.3e}  "
                  f"norm1 {ce['norm1'][0]:.3e}  inv_norm1 {ce['inv_norm1'][0]:.3e}  cond1 {ce['cond1'][0]:.3e} ({int(ce['solves'][0])} solves)")
            if label == "raw solve":
                norms, accepted = sy.refine(1)
                print(f"  refine(1): residual norms {norms[0]}, accepted {int(accepted[0])}")
        print(f"  scipy's yardstick (cases.cond_inf_estimate) {cases.cond_inf_estimate(cp, ri, Kreg):.3e}")
    sy.close()
    pp.close()
