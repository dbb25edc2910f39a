"""The early exits of the pipelined interior-point driver (sleipnir_amd/csrc/ipm_resident.cpp: ResidentIpm): a solve
stopped by max_iterations or by the timeout while the next iteration's step may be enqueued ahead of its verdict, what
such a solve leaves behind on its system, and the feasible-IPM option, which keeps the trial-values chain.

Every comparison is between drivers that run the same arithmetic in the same order — the device deciding the common
iteration (default), the host deciding every iteration (SLPX_IPM_PIPELINE=0), the deciding launch in front of a gated
step (SLPX_IPM_RIDE=0) — so it is to the bit and to the count; there is no tolerance in this file.
"""
import os

import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import cases
from tests.support import models

pytestmark = pytest.mark.gpu

MAX_ITERATIONS_EXCEEDED, TIMEOUT = -9, -10  # csrc/ipm.hpp: ExitStatus

ENVS = [{}, {"SLPX_IPM_PIPELINE": "0"}, {"SLPX_IPM_RIDE": "0"}]
COUNTS = ("iterations", "factorizations", "solves", "value_sweeps")


def cart_pole():
    # the smallest model of test_iterations_decided_on_the_device_are_the_hosts_bit_for_bit: it pipelines, regularizes,
    # and a solve takes milliseconds
    return models.cart_pole(50, 0.1)


def _solve_with_env(make, env, **options):
    """One solve of a NEW problem under `env` (the switches are read when its system is built)."""
    env = dict(env, SLPX_TWIN_VERBOSE="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pp = make()
        status, rep = pp.solve(**options)
        out = status, rep, pp.get_x(), pp.duals()
        pp.close()
        return out
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _same_iterate(a, b):
    (_, _, x_a, duals_a), (_, _, x_b, duals_b) = a, b
    assert np.array_equal(x_a, x_b)
    for u, v in zip(duals_a, duals_b):  # s, y, z
        assert np.array_equal(u, v)


def _decided_on_the_device(err):
    lines = [l for l in err.splitlines() if l.startswith("slpx pipelined iterations:")]
    return sum(int(l.split()[3]) for l in lines)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 9])
def test_max_iterations_with_a_step_enqueued_ahead(k, capfd):
    """A step is enqueued ahead only while iterations + 2 < max_iterations: k = 1, 2 never enqueue one, k = 3, 4 close
    the guard after one or two iterations, k = 9 follows the device for several iterations first.  Whatever was in
    flight, the three drivers stop at the same iterate with the same counts."""
    capfd.readouterr()
    runs = []
    for env in ENVS:
        runs.append(_solve_with_env(cart_pole, env, max_iterations=k))
        err = capfd.readouterr().err
        if not env and k == 9 and not cases.OUTER_SWITCHES:
            assert _decided_on_the_device(err) >= 1, err
    for status, rep, _, _ in runs:
        assert status == MAX_ITERATIONS_EXCEEDED and rep["iterations"] == k
    for run in runs[1:]:
        for key in COUNTS:
            assert run[1][key] == runs[0][1][key], key
        _same_iterate(run, runs[0])


@pytest.fixture(scope="module")
def uncapped():
    """A fresh problem's whole solve: what a solve on a clean system gives."""
    return _solve_with_env(cart_pole, {})


@pytest.mark.parametrize("stop,status,iterations", [
    (dict(max_iterations=9), MAX_ITERATIONS_EXCEEDED, 9),
    # (no iteration takes under a microsecond: the solve stops after its first — under the default switches with the
    # second iteration's step in flight)
    (dict(timeout=1e-6), TIMEOUT, 1),
])
def test_the_same_system_after_an_early_exit_is_clean(stop, status, iterations, uncapped, capfd, monkeypatch, request):
    """A capped solve, the variables back at the initial guess, an uncapped solve: the second solve is a fresh problem's,
    to the bit.

    Known gap: where the first solve is stopped WITH a step in flight — only the timeout does that, and
    only where an iteration was decided on the device — the second solve takes another path: 131 iterations where a
    fresh problem takes 309, both ending in SUCCESS.  The driver before ResidentIpm did the same; that case is an
    expected failure until the step in flight is accounted for, and a strict one, so that a fix shows."""
    monkeypatch.setenv("SLPX_TWIN_VERBOSE", "1")
    pp = cart_pole()
    x0 = pp.get_x()
    capfd.readouterr()
    st_stopped, rep_stopped = pp.solve(**stop)
    assert st_stopped == status and rep_stopped["iterations"] == iterations
    if "timeout" in stop and _decided_on_the_device(capfd.readouterr().err) >= 1:
        request.applymarker(pytest.mark.xfail(strict=True, reason="a solve stopped with a step in flight leaves its system unclean"))
    pp.set_x(x0)
    st_again, rep_again = pp.solve()
    again = st_again, rep_again, pp.get_x(), pp.duals()
    pp.close()
    assert st_again == uncapped[0]
    for key in ("iterations", "factorizations"):
        assert rep_again[key] == uncapped[1][key], key
    _same_iterate(again, uncapped)


def test_timeout_agrees_across_the_switches():
    runs = [_solve_with_env(cart_pole, env, timeout=1e-6) for env in ENVS]
    for status, rep, _, _ in runs:
        assert status == TIMEOUT and rep["iterations"] == 1
    for run in runs[1:]:
        _same_iterate(run, runs[0])


def flywheel():
    # feasible_ipm takes the trial s from the trial c_i only where every c_i is positive.  The cart-pole's initial guess
    # has the cart AT its lower bound (c_i = 0 there); the flywheel's inequality rows are -12 <= u <= 12 alone and its
    # guess is u = 0, so every c_i is 12 at the start: the smallest model of tests/support the option acts on.
    return models.flywheel(50, 0.005)


def test_feasible_ipm_resident_and_host_decided_agree():
    """feasible_ipm=True turns the pipeline off and keeps the trial-values chain (ahead == false) while c_i > 0."""
    pp = flywheel()
    n, me, mi = pp.dims
    system = sa.System(pp)
    system.set_state(pp.get_x(), np.ones(mi), np.zeros(me), np.ones(mi), np.array([0.1]))
    system.sweep(False)
    c_i = system.get("V")[0][1 + me:1 + me + mi]  # V = [f | c_e | c_i | ...] (nlp.hpp)
    system.close()
    pp.close()
    assert mi > 0 and (c_i > 0).all()

    resident = _solve_with_env(flywheel, {}, feasible_ipm=True)
    host_decided = _solve_with_env(flywheel, {"SLPX_IPM_PIPELINE": "0"}, feasible_ipm=True)
    assert resident[0] == host_decided[0]
    for key in COUNTS + ("restorations",):
        assert resident[1][key] == host_decided[1][key], key
    _same_iterate(resident, host_decided)
