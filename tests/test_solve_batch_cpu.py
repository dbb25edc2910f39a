"""slpx_problem_solve_batch without a device: arguments are checked before any device work, the call
fails cleanly where there is no device, and the ABI version stays 6 (the symbol is an addition)."""
import ctypes

import numpy as np
import pytest

import sleipnir_amd as sa
from sleipnir_amd.optimization import Problem


def _status_only(p, batch, x0):
    L = sa.lib()
    st = np.zeros(max(batch, 1), dtype=np.int32)
    return L.slpx_problem_solve_batch(p._p._h, batch, x0, None, 0, st.ctypes.data, None, None, None, None, None,
                                      None, None, None)


def _problem():
    sa.lib().slpx_graph_reset()
    p = Problem()
    x = p.decision_variable()
    p.minimize(x * x)
    p.subject_to(x >= 1)
    return p


def test_abi_version_stays_6():
    assert sa.lib().slpx_abi_version() == 6
    assert hasattr(sa.lib(), "slpx_problem_solve_batch")


def test_bad_arguments_refused():
    p = _problem()
    x0 = np.array([0.5, 2.0])
    assert _status_only(p, 0, x0.ctypes.data) == -100
    assert "batch" in sa.lib().slpx_last_error().decode()
    assert _status_only(p, -3, x0.ctypes.data) == -100
    assert _status_only(p, 2, None) == -100
    assert "x0" in sa.lib().slpx_last_error().decode()
    p.add_callback(lambda info: False)
    assert _status_only(p, 2, x0.ctypes.data) == -100
    assert "callback" in sa.lib().slpx_last_error().decode()
    p.close()


@pytest.mark.skipif(sa.lib().slpx_device_count() > 0, reason="this machine has a device")
def test_no_device_is_an_error():
    p = _problem()
    x0 = np.array([0.5, 2.0])
    assert _status_only(p, 2, x0.ctypes.data) == -100
    assert "no HIP device" in sa.lib().slpx_last_error().decode()
    with pytest.raises(sa.SlpxError):
        p.solve_batch([[0.5], [2.0]])
    with pytest.raises(sa.SlpxError):
        p.multistart([[0.5], [2.0]])
    p.close()


def test_python_shape_checked():
    p = _problem()
    with pytest.raises(ValueError):
        p.solve_batch([0.5, 2.0])
    with pytest.raises(KeyError):
        p.solve_batch([[0.5]], bogus=1)
    p.close()
