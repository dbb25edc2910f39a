"""GPU tier: whole batched solves with feasibility restoration in lockstep (Problem.solve_batch(..., restoration="lockstep"),
slpx_problem_set_batch_restoration): every instance that asks for restoration in a round of the outer loop enters one
restoration phase on the batch system together (csrc/fr_batch_lockstep.cpp), instead of being handed to the batch-1 system
one after the other.

The model and the six starts are those of test_restoration_inside_a_batch (tests/test_solve_batch_gpu.py), and so are the
assertions — the ones the hand-off mode meets: every status SUCCESS, restorations[b] equal to the single solve's, x within
1e-6 of the single solve and of (1, 0, 0.5).

The SQP driver: the search recorded in tests/test_solve_batch_eq_gpu.py found no equality-only model that restores AND
succeeds, so no whole solve covers the SQP driver's restoration in lockstep.  It is covered by the seam test on `eq_only`
(tests/test_restoration_batch_gpu.py: the restoration problem of a model without inequality rows, m_i = 0) and by sharing the
loop: lockstep<Driver> enters restoration_phase the same way for both drivers, with the driver's restoration_mu.
"""
import numpy as np
import pytest

from tests.support import model

pytestmark = pytest.mark.gpu

SUCCESS = 0
STARTS = np.array([[x0, 3.0, 1.0] for x0 in (-4.0, -3.0, -2.0, -1.5, 0.0, 2.0)])


@pytest.fixture
def m(fresh):
    be = model.ProductBackend("gpu")
    be.reset()
    return model.Model(be)


def build(m):
    p = model.NlpProblem(m)
    x, s1, s2 = p.decision_variable(-2), p.decision_variable(3), p.decision_variable(1)
    p.minimize(x)
    p.eq(m.pow(x, 2) - s1 - 1, 0)
    p.eq(x - s2 - 0.5, 0)
    p.ge(s1, 0)
    p.ge(s2, 0)
    return p


def _single(p, x0):
    p.set_x(np.asarray(x0, dtype=np.float64))
    status, rep = p.solve()
    return status, p.get_x(), rep["iterations"], rep.get("restorations", 0)


def test_restoration_in_lockstep_inside_a_batch(m):
    p = build(m)
    r = p.p.solve_batch(STARTS, restoration="lockstep")
    assert int(np.sum(r["restorations"])) > 0
    for b, x0 in enumerate(STARTS):
        status, xs, _, restorations = _single(p.p, x0)
        assert r["status"][b] == status == SUCCESS, (x0, r["status"][b], status)
        assert r["restorations"][b] == restorations, (x0, r["restorations"][b], restorations)
        assert np.max(np.abs(r["x"][b] - xs)) <= 1e-6, (x0, r["x"][b], xs)
        assert np.max(np.abs(r["x"][b] - [1.0, 0.0, 0.5])) <= 1e-6, (x0, r["x"][b])
    fr = r["restoration_lockstep"]
    print("lockstep:", fr, "restorations", r["restorations"], "iterations", r["iterations"], "rounds", r["rounds"])
    assert fr["instances"] > 0 and fr["instances"] == int(np.sum(r["restorations"])) and fr["phases"] > 0 and fr["rounds"] > 0
    assert r["handoffs"] == 0
    assert p.p.batch_restoration_stats() == (fr["instances"], fr["phases"], fr["rounds"], fr["fallbacks"])


def test_both_modes_agree(m):
    """The same batch under "handoff" (the default) and "lockstep": the same statuses and restoration counts; the hand-off
    mode counts its hand-offs and no lockstep restoration, the lockstep mode the other way round; the mode is read by the
    NEXT solve_batch and stays until it is set again."""
    p = build(m)
    lock = p.p.solve_batch(STARTS, restoration="lockstep")
    hand = p.p.solve_batch(STARTS, restoration="handoff")
    default = p.p.solve_batch(STARTS)
    assert np.array_equal(lock["status"], hand["status"]) and np.array_equal(lock["restorations"], hand["restorations"])
    assert hand["handoffs"] == int(np.sum(hand["restorations"])) > 0 and lock["handoffs"] == 0
    assert all(v == 0 for v in hand["restoration_lockstep"].values())
    assert lock["restoration_lockstep"]["instances"] == int(np.sum(lock["restorations"]))
    for k in ("status", "x", "iterations", "restorations"):
        assert np.array_equal(default[k], hand[k]), k
    assert default["handoffs"] == hand["handoffs"]
    print("iterations: lockstep", lock["iterations"], "handoff", hand["iterations"])
    print("max |x_lockstep - x_handoff|", float(np.max(np.abs(lock["x"] - hand["x"]))))


def test_isolation_of_restoring_instances(m):
    """A restoring instance's x, iteration count and status are bit-identical (a) with the six starts in order, (b) with them
    permuted, (c) with the restoring starts alone, permuted, padded to the same B with starts that never restore: who shares a
    restoration phase, and in which slot, changes nothing."""
    p = build(m)
    base = p.p.solve_batch(STARTS, restoration="lockstep")
    restoring = [b for b in range(len(STARTS)) if base["restorations"][b] > 0]
    quiet = [b for b in range(len(STARTS)) if base["restorations"][b] == 0]
    assert restoring
    print("restoring starts:", [float(STARTS[b][0]) for b in restoring], "never restoring:", [float(STARTS[b][0]) for b in quiet])
    perm = [3, 5, 0, 4, 2, 1]
    arrangements = [perm]
    if quiet:
        padded = list(reversed(restoring)) + [quiet[k % len(quiet)] for k in range(len(STARTS) - len(restoring))]
        arrangements.append(padded)
    for order in arrangements:
        r = p.p.solve_batch(STARTS[order], restoration="lockstep")
        for slot, b in enumerate(order):
            if b not in restoring:
                assert r["restorations"][slot] == 0
                continue
            assert r["status"][slot] == base["status"][b] == SUCCESS, (order, slot)
            assert r["iterations"][slot] == base["iterations"][b], (order, slot, r["iterations"][slot], base["iterations"][b])
            assert r["restorations"][slot] == base["restorations"][b]
            assert np.array_equal(r["x"][slot].view(np.uint64), base["x"][b].view(np.uint64)), (order, slot, r["x"][slot], base["x"][b])
