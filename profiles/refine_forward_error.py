#!/usr/bin/env python3
"""What iterative refinement buys at the suite's seeded interior state of cart-pole N=1000 (kappa ~ 1e10): the
residual norm |r|_inf of slpx_ldlt_residual before and after 1, 2 and 3 steps of slpx_ldlt_refine, and the distance of
the step to the refined solution of tests/support/cases.py (sparse LU + long-double residuals) before and after, beside
the oracle's own distance.  Needs a GPU.
    python profiles/refine_forward_error.py [N] > profiles/refine_forward_error.txt"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402

import sleipnir_amd as slpx  # noqa: E402
from tests.support import cases, oracle as orc, parity  # noqa: E402


def main(N=1000):
    orc.lib().orc_reset()
    slpx.lib().slpx_graph_reset()
    pp, op = cases.build_pair("cart_pole", N, slpx, orc)
    n, me, mi = pp.dims
    system = slpx.System(pp, batch=1, device=0)
    be = parity.GpuBackend(system)
    scales = op.scaling()
    be.set_scaling(scales)
    lcp, lri = be.pattern(5)
    x, s, y, z, mu = cases.newton_state("interior", op.get_x(), n, me, mi, scales[0])
    info, _ = op.newton_step(x, s, y, z, mu, True, be.perm())
    assert info == 0
    delta, gamma, _, _ = op.reg()
    be.sweep(x, y, z, True)
    lhs = be.assemble(s, z)
    rhs = be.rhs(s, y, z, mu)
    Kreg = cases.regularized(lcp, lri, lhs, n, delta, gamma)
    p_true = cases.refined_solution(lcp, lri, Kreg, rhs)
    kappa = cases.cond_inf_estimate(lcp, lri, Kreg)
    po = cases.max_rel(op.vec("p"), p_true)
    print(f"# cart-pole N={N}, seeded interior state, (delta, gamma) = ({delta:g}, {gamma:g}), kappa_inf {kappa:.2e}, "
          f"multifrontal {system.info['ldlt_multifrontal']}; oracle's distance to the refined solution {po:.3e}")
    print("# steps asked  accepted  |r|_inf before  |r|_inf after  p_vs_true before  p_vs_true after  after / oracle's")
    for steps in (1, 2, 3):
        be.factor(delta, gamma)
        p0 = be.solve()
        norms, accepted = system.refine(steps)
        k = int(accepted[0])
        p = system.get("p")[0]
        before, after = cases.max_rel(p0, p_true), cases.max_rel(p, p_true)
        print(f"  {steps:11d}  {k:8d}  {norms[0, 0]:14.3e}  {norms[0, k]:13.3e}  {before:16.3e}  {after:15.3e}  {after / po:16.2f}",
              flush=True)
        print("#   norms:", " ".join(f"{v:.3e}" for v in norms[0]))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1000)
