"""slpx_problem_batch_stats and the batched SQP / Newton path without a device: the symbol is an addition within ABI
version 6, it reports -1 before any batch, and models without inequality constraints fail a batch cleanly where there
is no device, as the others do."""
import numpy as np
import pytest

import sleipnir_amd as sa
from sleipnir_amd.optimization import Problem


def _equality_only():
    sa.lib().slpx_graph_reset()
    p = Problem()
    x, y = p.decision_variable(), p.decision_variable()
    p.minimize((x - 2) ** 2 + (y - 1) ** 2)
    p.subject_to(x * x + y * y == 1)
    return p


def _unconstrained():
    sa.lib().slpx_graph_reset()
    p = Problem()
    x, y = p.decision_variable(), p.decision_variable()
    p.minimize(100 * (y - x * x) ** 2 + (1 - x) ** 2)
    return p


def test_symbol_is_an_addition_within_abi_6():
    assert hasattr(sa.lib(), "slpx_problem_batch_stats")
    assert sa.lib().slpx_abi_version() == 6


def test_no_batch_solved_yet():
    p = _equality_only()
    out = np.full(4, -7, dtype=np.int64)
    assert sa.lib().slpx_problem_batch_stats(p._p._h, out.ctypes.data) == -1
    assert list(out) == [-7] * 4
    with pytest.raises(sa.SlpxError):
        p._p.batch_stats()
    p.close()


@pytest.mark.skipif(sa.lib().slpx_device_count() > 0, reason="this machine has a device")
@pytest.mark.parametrize("make", [_equality_only, _unconstrained])
def test_no_device_is_an_error(make):
    p = make()
    with pytest.raises(sa.SlpxError, match="no HIP device"):
        p.solve_batch([[0.5, 1.0], [2.0, 0.5]])
    out = np.zeros(4, dtype=np.int64)
    assert sa.lib().slpx_problem_batch_stats(p._p._h, out.ctypes.data) == -1
    p.close()
