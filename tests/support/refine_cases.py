"""Shared by the GPU tests of the residual / refinement path (tests/test_refine_gpu.py, test_refine_batch_gpu.py):
systems brought to "factors and a solution in memory", and the host references — the host body of row_residual
(refinecheck) for bits, numpy in extended precision for accuracy."""
from __future__ import annotations

from pathlib import Path

import numpy as np

import sleipnir_amd as sa
from tests.support import cases, models, parity, refinecheck

GOLDEN = Path(__file__).resolve().parents[1] / "golden"
FIXTURES = ["cart_pole_N8_indefinite", "cart_pole_N6_interior", "flywheel_N5_interior"]
# cart-pole N = 30: n = 5 N + 4 = 154, m_e = 4 N + 8 = 128, dim = 282 = 256 + 26 = 4 x 64 + 26 — two workgroups of the
# residual kernel, the second with one ragged wave
BIG_N, BIG_DIM = 30, 282
# The pair given to slpx_ldlt_factor where a test picks one: the first regularized rung of the policy's ladder.  With
# delta = 0 the unpivoted elimination meets structurally zero pivots of H at the cart-pole states used here; with this
# pair the counters are (n, m_e, 0, 0) — every test asserts them from the device.
REG = (1e-4, 1e-10)


def fixture_system(name, batch=1):
    """A problem's System at the fixture's state, lhs and rhs assembled; returns (problem, system, chosen (delta, gamma))."""
    fx = dict(np.load(GOLDEN / f"{name}.npz"))
    kind = "flywheel" if name.startswith("flywheel") else "cart_pole"
    N = int(fx["N"])
    sa.lib().slpx_graph_reset()
    pp = getattr(models, kind)(N, 5.0 / N)
    system = sa.System(pp, batch=batch, device=0)
    system.set_scaling(np.r_[fx["d_f"], fx["d_ce"], fx["d_ci"]])
    rep = lambda a: np.tile(np.atleast_1d(a), batch)
    system.set_state(rep(fx["x"]), rep(fx["s"]), rep(fx["y"]), rep(fx["z"]), rep(fx["mu"]))
    system.sweep(True)
    system.assemble()
    system.rhs()
    return pp, system, (float(fx["chosen"][0]), float(fx["chosen"][1]))


def seeded_system(kind, N, batch=1, seeds=None):
    """A problem's System, problem b at the suite's seeded interior state of seed seeds[b]; lhs and rhs assembled."""
    sa.lib().slpx_graph_reset()
    pp = getattr(models, kind)(N, 5.0 / N)
    n, me, mi = pp.dims
    system = sa.System(pp, batch=batch, device=0)
    system.set_scaling(np.ones(1 + me + mi))
    seeds = [cases.SEED + b for b in range(batch)] if seeds is None else seeds
    st = [cases.newton_state("interior", pp.get_x(), n, me, mi, 1.0, seed=s) for s in seeds]
    system.set_state(*(np.concatenate([np.atleast_1d(s[k]) for s in st]) for k in range(5)))
    system.sweep(True)
    system.assemble()
    system.rhs()
    return pp, system


def host_residual(system, reg, b=0):
    """The host body of row_residual on what the device holds for problem b: (r, lhs, rhs, p)."""
    cp, ri = system.pattern(5)
    lhs, rhs, p = system.get("lhs")[b], system.get("rhs")[b], system.get("p")[b]
    r, _ = refinecheck.residual(cp, ri, lhs, rhs, p, system.info["n"], reg[0], reg[1])
    return r, lhs, rhs, p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def eta(cp, ri, Kreg, rhs, p):
    """The componentwise-scaled backward error |r|_inf / (| |Kreg| |p| |_inf + |b|_inf), r in extended precision."""
    r = parity.residual_longdouble(cp, ri, Kreg, rhs, p)
    scale = float(np.max(cases.lower_csc_matvec(cp, ri, np.abs(Kreg), np.abs(p)))) + float(np.max(np.abs(rhs)))
    return float(np.max(np.abs(r))) / scale


def numpy_refinement(cp, ri, Kreg, rhs, p, steps):
    """The restatement: `steps` steps from p, residual in extended precision, correction by a double dense solve."""
    K = cases.lower_csc_to_dense_sym(cp, ri, Kreg, len(rhs))
    p = np.array(p, copy=True)
    for _ in range(steps):
        p = p + np.linalg.solve(K, parity.residual_longdouble(cp, ri, Kreg, rhs, p))
    return p
