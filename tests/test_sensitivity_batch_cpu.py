"""Batched solution sensitivities, the parts that need no device (include/slpx.h: batched sensitivities): the instance
classification as a pure host function (csrc/sens_plan.hpp: sens_classify_instances), the presence of the four entry
points in libslpx.so, and their loud failure where there is no HIP device."""
from __future__ import annotations

import ctypes

import numpy as np

import sleipnir_amd
from tests.support import sensbatchcheck

ENTRY_POINTS = ("slpx_problem_sensitivity_batch", "slpx_problem_sensitivity_batch_jvp", "slpx_problem_sensitivity_batch_vjp",
                "slpx_problem_sensitivity_batch_rhs")


def healthy(B=5, n=3, m_e=2, m_i=2, n_p=2):
    rng = np.random.default_rng(3)
    return dict(x=rng.uniform(-1, 1, (B, n)), s=rng.uniform(0.1, 1, (B, m_i)), y=rng.uniform(-1, 1, (B, m_e)),
                z=rng.uniform(0.1, 1, (B, m_i)), mu=np.full(B, 1e-9), params=rng.uniform(-1, 1, (B, n_p)))


def classify(rows, extra=None):
    return list(sensbatchcheck.classify(rows["x"], rows["s"], rows["y"], rows["z"], rows["mu"], rows["params"], extra))


def test_classification_of_healthy_rows():
    assert classify(healthy()) == [0, 0, 0, 0, 0]
    assert classify(healthy(B=1)) == [0]
    # negative multipliers and a zero z are no reason to skip: only s divides
    rows = healthy()
    rows["z"][1, 0] = 0.0
    rows["y"][2, 1] = -5.0
    assert classify(rows) == [0, 0, 0, 0, 0]


def test_classification_finds_every_kind_of_bad_row():
    for key, (b, j), value in (("x", (2, 0), np.nan), ("x", (0, 2), np.inf), ("s", (1, 1), np.nan), ("y", (3, 0), -np.inf),
                               ("z", (4, 1), np.nan), ("params", (2, 1), np.inf), ("params", (0, 0), np.nan),
                               ("s", (2, 0), 0.0), ("s", (3, 1), -1e-300), ("s", (1, 0), np.inf)):
        rows = healthy()
        rows[key][b, j] = value
        want = [0] * 5
        want[b] = 1
        assert classify(rows) == want, (key, b, j, value)
    rows = healthy()
    rows["mu"][3] = np.nan
    assert classify(rows) == [0, 0, 0, 1, 0]
    # several at once, and the first and the last instance
    rows = healthy()
    rows["x"][0, 1] = np.nan
    rows["s"][4, 0] = 0.0
    assert classify(rows) == [1, 0, 0, 0, 1]


def test_classification_of_dp_and_vx():
    rows = healthy()
    extra = np.ones((5, 4))
    assert classify(rows, extra) == [0, 0, 0, 0, 0]
    extra[2, 3] = np.nan
    extra[4, 0] = -np.inf
    assert classify(rows, extra) == [0, 0, 1, 0, 1]
    rows["x"][1, 0] = np.inf
    assert classify(rows, extra) == [0, 1, 1, 0, 1]


def test_classification_with_empty_blocks():
    # m_i = 0: no slack to be positive, s and z are NULL
    rows = healthy(m_i=0)
    assert rows["s"].shape == (5, 0) and classify(rows) == [0, 0, 0, 0, 0]
    rows["y"][2, 0] = np.nan
    assert classify(rows) == [0, 0, 1, 0, 0]
    # m_e = 0
    rows = healthy(m_e=0)
    assert classify(rows) == [0, 0, 0, 0, 0]
    rows["s"][0, 1] = 0.0
    assert classify(rows) == [1, 0, 0, 0, 0]
    # neither (the Newton driver's models)
    rows = healthy(m_e=0, m_i=0)
    rows["params"][4, 1] = np.nan
    assert classify(rows) == [0, 0, 0, 0, 1]


def test_the_entry_points_exist():
    L = sleipnir_amd.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is ctypes.c_int


def test_without_a_device_they_fail_loudly(fresh):
    """-100 and a message that names the missing device — for the argument errors that need none, their own message."""
    from sleipnir_amd import autodiff, optimization

    L = sleipnir_amd.lib()
    if L.slpx_device_count() >= 1:
        return  # (with a device the calls run: tests/test_sensitivity_batch_gpu.py)
    problem = optimization.Problem()
    x, a = problem.decision_variable(), autodiff.Variable()
    a.set_value(2.0)
    problem.minimize((x - a) ** 2)
    assert len(problem.parameters()) == 1  # (from the host graph)
    h = problem._p._h
    one, out, status = np.ones((1, 1)), np.zeros(4), np.zeros(1, dtype=np.int32)
    rows = (one.ctypes.data, None, None, None, one.ctypes.data, one.ctypes.data)
    calls = {
        "slpx_problem_sensitivity_batch": lambda B, r: L.slpx_problem_sensitivity_batch(h, B, *r, out.ctypes.data, None, None, None, status.ctypes.data, None),
        "slpx_problem_sensitivity_batch_jvp": lambda B, r: L.slpx_problem_sensitivity_batch_jvp(h, B, *r, one.ctypes.data, out.ctypes.data, None, None, None, status.ctypes.data, None),
        "slpx_problem_sensitivity_batch_vjp": lambda B, r: L.slpx_problem_sensitivity_batch_vjp(h, B, *r, one.ctypes.data, out.ctypes.data, status.ctypes.data, None),
        "slpx_problem_sensitivity_batch_rhs": lambda B, r: L.slpx_problem_sensitivity_batch_rhs(h, B, *r, out.ctypes.data, status.ctypes.data),
    }
    for name, call in calls.items():
        assert call(1, rows) == -100, name
        assert b"no HIP device" in L.slpx_last_error(), (name, L.slpx_last_error())
        assert call(0, rows) == -100 and b"B must be" in L.slpx_last_error(), name
        assert call(1, (None,) + rows[1:]) == -100 and b"null" in L.slpx_last_error(), name
    # Python: the same failure as an exception
    import pytest

    with pytest.raises(sleipnir_amd.SlpxError, match="no HIP device"):
        problem.sensitivity_batch_vjp(optimization.BatchIterate(x=one, mu=np.ones(1)), one, one)
    problem.close()
