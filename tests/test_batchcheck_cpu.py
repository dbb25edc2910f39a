"""The test-only probe of the batched interior-point driver (tests/support/batchcheck.cpp) builds and loads without a
device, refuses a missing system cleanly, and is not part of the product."""
import subprocess

import sleipnir_amd as sa
from tests.support import batchcheck as bc


def test_probe_loads_and_fails_cleanly():
    L = bc.lib()
    assert L.bc_create(None) is None
    assert b"no system" in L.bc_last_error()
    assert L.bc_get(None, 0, None) == -1
    assert b"no probe" in L.bc_last_error()


def test_probe_is_not_in_the_product():
    out = subprocess.run(["nm", "-D", "--defined-only", str(sa.LIB_PATH)], capture_output=True, text=True, check=True)
    assert " bc_" not in out.stdout
    assert "BatchIpmProbe" not in out.stdout
