"""The test-only probe of feasibility restoration (tests/support/frcheck.cpp) builds and loads without a device, refuses
a missing system cleanly, and is not part of the product."""
import subprocess

import sleipnir_amd as sa
from tests.support import frcheck as fc


def test_probe_loads_and_fails_cleanly():
    L = fc.lib()
    assert L.fc_create(None) is None
    assert b"no system" in L.fc_last_error()
    assert L.fc_get(None, 0, None) == -1
    assert b"no probe" in L.fc_last_error()
    assert L.fc_build(None, 0.0, 0.1, 0, 0, 0) == -1
    assert b"no probe" in L.fc_last_error()


def test_probe_is_not_in_the_product():
    out = subprocess.run(["nm", "-D", "--defined-only", str(sa.LIB_PATH)], capture_output=True, text=True, check=True)
    assert " fc_" not in out.stdout
    assert "FrProbe" not in out.stdout
