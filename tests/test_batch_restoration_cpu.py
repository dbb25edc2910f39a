"""Restoration in lockstep for batches, what needs no device: the three symbols of the public interface (additions within
ABI version 6), the default mode, the refusals — and the regularization policy loop of a batch whose system the caller
writes: ldlt_run_batch (csrc/ldlt_policy.hpp) with per-problem extra pivots, scripted the way tests/test_reg_policy_cpu.py
scripts the other drivers (tests/support/regbatchcheck.cpp; the reference is hostcheck.reg_policy)."""
import ctypes
import itertools

import numpy as np
import pytest

import sleipnir_amd as sa
from sleipnir_amd.optimization import Problem
from tests.support import hostcheck, regbatchcheck

SYMBOLS = ["slpx_problem_set_batch_restoration", "slpx_problem_batch_restoration_stats", "slpx_problem_restoration_steps_batch"]


def _problem():
    sa.lib().slpx_graph_reset()
    p = Problem()
    x = p.decision_variable()
    p.minimize(x * x)
    p.subject_to(x >= 1)
    return p


def test_symbols_are_additions_within_abi_6():
    L = sa.lib()
    assert L.slpx_abi_version() == 6
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_default_mode_is_the_handoff():
    p = _problem()
    L, h = sa.lib(), p._p._h
    assert L.slpx_problem_set_batch_restoration(h, -1) == 0  # a query: the mode in force
    assert L.slpx_problem_set_batch_restoration(h, 1) == 0
    assert L.slpx_problem_set_batch_restoration(h, -1) == 1
    assert L.slpx_problem_set_batch_restoration(h, 0) == 0
    assert L.slpx_problem_set_batch_restoration(h, -1) == 0
    assert L.slpx_problem_set_batch_restoration(h, 2) == -100
    assert "mode" in L.slpx_last_error().decode()
    assert L.slpx_problem_set_batch_restoration(h, -1) == 0  # (a refused mode changes nothing)
    assert L.slpx_problem_set_batch_restoration(None, 0) == -100
    assert "null problem" in L.slpx_last_error().decode()
    out = np.zeros(4, dtype=np.int64)
    assert L.slpx_problem_batch_restoration_stats(h, out.ctypes.data) == -1  # no batch has been solved
    with pytest.raises(ValueError):
        p._p.solve_batch([[0.5]], restoration="both")
    p.close()


def _steps(p, batch, x, mu, status, s=None, z=None):
    L = sa.lib()
    ptr = lambda a: None if a is None else a.ctypes.data
    return L.slpx_problem_restoration_steps_batch(p._p._h, None, 0, batch, ptr(x), ptr(s), None, ptr(z), ptr(mu), 1, ptr(status))


def test_bad_arguments_refused():
    p = _problem()
    x, one, mu, st = np.array([0.5, 2.0]), np.ones(2), np.full(2, 0.1), np.zeros(2, dtype=np.int32)
    assert _steps(p, 0, x, mu, st, one, one) == -100
    assert "batch" in sa.lib().slpx_last_error().decode()
    assert _steps(p, 2, None, mu, st, one, one) == -100
    assert _steps(p, 2, x, None, st, one, one) == -100
    assert _steps(p, 2, x, mu, None, one, one) == -100
    assert "null" in sa.lib().slpx_last_error().decode()
    p.add_callback(lambda info: False)
    assert _steps(p, 2, x, mu, st, one, one) == -100
    assert "callback" in sa.lib().slpx_last_error().decode()
    p.close()


@pytest.mark.skipif(sa.lib().slpx_device_count() > 0, reason="this machine has a device")
def test_no_device_is_an_error():
    p = _problem()
    x, one, mu, st = np.array([0.5, 2.0]), np.ones(2), np.full(2, 0.1), np.zeros(2, dtype=np.int32)
    assert _steps(p, 2, x, mu, st, one, one) == -100
    assert "no HIP device" in sa.lib().slpx_last_error().decode()
    with pytest.raises(sa.SlpxError):
        p._p.restoration_steps_batch(x.reshape(2, 1), one.reshape(2, 1), np.zeros((2, 0)), one.reshape(2, 1), mu, 1)
    with pytest.raises(sa.SlpxError):
        p.solve_batch([[0.5], [2.0]], restoration="lockstep")
    assert sa.lib().slpx_problem_set_batch_restoration(p._p._h, -1) == 1  # (the mode was set before the solve was refused)
    p.close()


# ---------------------------------------------------------------------------------------------------------------------
# ldlt_run_batch with per-problem extra pivots
# ---------------------------------------------------------------------------------------------------------------------
N, ME = 7, 3
IDEAL = (N, ME, 0, 0)


def response(ok_delta, ok_gamma=0.0, min_abs=1.0, wrong=(N - 1, ME + 1, 0, 0)):
    """ideal inertia once delta >= ok_delta and gamma >= ok_gamma, `wrong` below (rows: the first that matches answers)"""
    rows = []
    if ok_delta > 0:
        rows.append((ok_delta, np.inf, 0, *wrong, 1.0))
    if ok_gamma > 0:
        rows.append((np.inf, ok_gamma, 0, N + 1, ME - 1, 0, 0, 1.0))
    rows.append((np.inf, np.inf, 0, *IDEAL, min_abs))
    return rows


def test_extra_pivots_reject_the_unregularized_attempt_per_problem():
    """Every problem answers its unregularized attempt with the ideal inertia and |D| >= 1e-4: without extras all are
    accepted at (0, 0); with extras exactly the problems whose eliminated pivot is below 1e-4 (or NaN) are rejected and
    climb from delta = 1e-4 — the attempts, the memory and the verdict of ldlt_run_twin(.., extra) for that problem
    alone (the hooked driver of hostcheck, every launch a single attempt)."""
    extras = [1.0, 9.9e-5, 1e-4, 0.0, np.inf, np.nan, 5e-5]
    memories = [(0.0, 0.0), (0.0, 0.0), (1e-2, 0.0), (4e-3, 1e-10), (0.0, 0.0), (0.0, 0.0), (8.0, 0.0)]
    # regularized attempts: ideal from delta 1e-3 on for the odd problems, at once for the even ones
    problems = [(memories[b], [(1e-300, 1e-300, 0, *IDEAL, 1.0)] + response(1e-3 if b % 2 else 0.0)) for b in range(len(extras))]
    plain = regbatchcheck.reg_policy_batch(N, ME, problems, gamma_min=0.0)
    assert plain["launches"] == 1 and all(a == [(0.0, 0.0)] for a in plain["attempts"])
    assert all(m == (0.0, 0.0) for m in plain["memory"])
    got = regbatchcheck.reg_policy_batch(N, ME, problems, gamma_min=0.0, extra=extras)
    rejected = [b for b, a in enumerate(got["attempts"]) if len(a) > 1]
    assert rejected == [b for b, e in enumerate(extras) if not (e >= 1e-4)] == [1, 3, 5, 6]
    for b, (mem, resp) in enumerate(problems):
        # (hostcheck's script reads NaN as "no extra pivot": a NaN pivot fails the test as any pivot below 1e-4 does, 0 here)
        extra = None if np.isinf(extras[b]) else (0.0 if np.isnan(extras[b]) else extras[b])
        want = hostcheck.reg_policy(N, ME, [(mem, resp)], driver="hooked", gamma_min=0.0, decline=0xffffffff, eliminated_min_pivot=extra)
        assert got["attempts"][b] == want["attempts"][0], b
        assert got["memory"][b] == want["memory"][0] and got["info"][b] == want["info"][0], b
        assert got["launch_of"][b] == list(range(len(got["attempts"][b]))), b  # one attempt per launch, from the first launch on
    assert got["launches"] == max(len(a) for a in got["attempts"])
    # the climb of a rejected problem: delta = max(prev / 2, eps) or 1e-4 first, then x 10 while the inertia is wrong
    assert got["attempts"][1][:3] == [(0.0, 0.0), (1e-4, 0.0), (1e-4 * 10.0, 0.0)]
    assert got["attempts"][6][:2] == [(0.0, 0.0), (4.0, 0.0)]


def test_without_extras_the_loop_is_todays():
    """A grid of responses (what the unregularized attempt shows x where the ladder ends x the memory x a mask): the
    attempts of every problem, the launches, the verdicts and the memory are those of the sequential driver of hostcheck —
    ldlt_run_batch as NewtonSystem::compute runs it — with and without the optional argument given as "none"."""
    firsts = [IDEAL + (1.0,), IDEAL + (1e-5,), (N - 1, ME + 1, 0, 0, 1.0), (N + 1, ME - 1, 0, 0, 1.0), (N - 1, ME, 1, 0, 1.0),
              (N, ME, 0, 1, 1.0)]
    ends = [(0.0, 0.0), (1e-2, 0.0), (0.0, 1e-8), (1e30, 0.0)]
    mems = [(0.0, 0.0), (2e-3, 1e-9)]
    cases = list(itertools.product(firsts, ends, mems))
    problems = []
    for first, (ok_d, ok_g), mem in cases:
        problems.append((mem, [(1e-300, 1e-300, 0, *first)] + response(ok_d, ok_g)))
    for mask in (None, [b % 3 != 1 for b in range(len(problems))]):
        for skip_first in (False, True):
            want = hostcheck.reg_policy(N, ME, problems, driver="sequential", skip_first=skip_first, mask=mask)
            got = regbatchcheck.reg_policy_batch(N, ME, problems, skip_first=skip_first, launch_for_nobody=not skip_first, mask=mask)
            assert got["attempts"] == want["attempts"]
            assert got["memory"] == want["memory"] and got["info"] == want["info"]
            assert got["launches"] == want["factorizations"]
            inf = regbatchcheck.reg_policy_batch(N, ME, problems, skip_first=skip_first, launch_for_nobody=not skip_first, mask=mask,
                                                 extra=[np.inf] * len(problems))
            assert inf == got
    assert any(i == 1 for i in got["info"]) and any(len(a) > 3 for a in got["attempts"])  # give-ups and ladders are in the grid
