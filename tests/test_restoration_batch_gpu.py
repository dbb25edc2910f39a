"""GPU tier, the seam of restoration in lockstep: slpx_problem_restoration_steps_batch — B iterates, `steps` iterations of
feasibility restoration each, in lockstep on the batch system (csrc/fr_batch_lockstep.cpp) — against the ORACLE's
feasibility_restoration (util/feasibility_restoration.hpp:347-628 + lagrange_multiplier_estimate.hpp:56-133) from the same
iterate, instance by instance.

Cases: steps 1 and 2 from cases.newton_state("interior", start (1 + 1e-3 noise_b)) on tiny, ineq_only, eq_only (m_e = 0 and
m_i = 0: the SQP driver's restoration problem among them) and chain300 at B = 3, and chain300 at B = 64 (the
batch-interleaved factorization).  The agreement asked is that of test_restoration_steps_match_oracle_on_general_models
(tests/test_restoration_gpu.py): 10 times the oracle's own sensitivity to a 1e-15 relative perturbation of x, computed here
per instance, floored at 1e-10 for x, s and at 1e-8 for y, z.  Every instance must return status 0 and must have moved.

Measured when this was written (worst instance, product vs oracle, steps 1 / 2; the floors are what holds):
  tiny B=3       x 3.3e-16 / 2.0e-15, s 2.0e-16 / 2.1e-15, y 8.9e-16 / 9.0e-16, z 4.2e-17 / 2.6e-16
  ineq_only B=3  x 5.6e-14 / 3.7e-14, s 5.0e-14 / 9.5e-14,                      z 3.5e-13 / 1.6e-13
  eq_only B=3    x 1.8e-16 / 2.5e-15,                      y 4.3e-16 / 1.4e-15
  chain300 B=3   x 2.6e-15 / 3.2e-15, s 2.8e-16 / 5.8e-16, y 7.0e-15 / 1.2e-14, z 1.1e-14 / 7.5e-15
  chain300 B=64  x 5.2e-15 / 1.2e-14, s 4.0e-16 / 1.6e-15, y 1.6e-14 / 1.7e-14, z 1.8e-14 / 3.2e-14
the oracle's own sensitivity being of the same size (2.5e-16 .. 2.3e-13).  One phase per call, `steps` lockstep rounds, no
fallback to the batch-1 system.
"""
import numpy as np
import pytest

from tests.support import cases, fr_models, model

pytestmark = pytest.mark.gpu

SHAPES = [("tiny", 3), ("ineq_only", 3), ("eq_only", 3), ("chain300", 3), ("chain300", 64)]


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("name,B", SHAPES)
def test_restoration_steps_batch_match_oracle(fresh, slpx, orc, name, B, steps):
    pp_, start = fr_models.make(model.Model(model.ProductBackend("gpu")), name)
    op_, _ = fr_models.make(model.Model(model.OracleBackend()), name)
    pp, op = pp_.p, op_.p
    n, me, mi = pp.dims
    assert (n, me, mi) == op.dims
    scales = op.scaling()
    rng = np.random.default_rng(cases.SEED + B)
    X, S, Y, Z, MU = [], [], [], [], []
    for b in range(B):
        x, s, y, z, mu = cases.newton_state("interior", start * (1.0 + 1e-3 * rng.uniform(-1, 1, n)), n, me, mi, scales[0])
        X.append(x), S.append(s), Y.append(y), Z.append(z), MU.append(mu)
    X, S, Y, Z, MU = (np.array(v) for v in (X, S, Y, Z, MU))
    status, xp, s_p, yp, zp = pp.restoration_steps_batch(X, S.reshape(B, mi), Y.reshape(B, me), Z.reshape(B, mi), MU, steps)
    stats = pp.batch_restoration_stats()
    assert stats[0] == B and stats[1] == 1 and stats[2] >= steps, stats
    pert = np.random.default_rng(cases.SEED).uniform(-1, 1, n)
    worst = {k: 0.0 for k in "xsyz"}
    worst_sens = {k: 0.0 for k in "xsyz"}
    for b in range(B):
        so, xo, s_o, yo, zo = op.restoration_steps(X[b], S[b], Y[b], Z[b], MU[b], steps)
        sq, xq, s_q, yq, zq = op.restoration_steps(X[b] * (1.0 + 1e-15 * pert), S[b], Y[b], Z[b], MU[b], steps)
        sens = {k: cases.max_rel(a, c) for k, a, c in (("x", xq, xo), ("s", s_q, s_o), ("y", yq, yo), ("z", zq, zo))}
        assert status[b] == so == sq == 0, (b, status[b], so, sq)
        assert not np.allclose(xp[b], X[b], rtol=0, atol=1e-6), b  # the restoration moved the iterate
        errs = {k: cases.max_rel(a, c) for k, a, c in (("x", xp[b], xo), ("s", s_p[b], s_o), ("y", yp[b], yo), ("z", zp[b], zo))}
        tol = {k: max(10.0 * sens[k], 1e-10 if k in "xs" else 1e-8) for k in sens}
        for k in errs:
            worst[k], worst_sens[k] = max(worst[k], errs[k]), max(worst_sens[k], sens[k])
        for k in errs:
            assert errs[k] <= tol[k], (b, k, errs, tol)
    print(f"{name} B={B} steps={steps}: worst product vs oracle", {k: f"{v:.2e}" for k, v in worst.items()},
          "oracle's own sensitivity", {k: f"{v:.2e}" for k, v in worst_sens.items()}, "stats", stats)
    pp.close()
