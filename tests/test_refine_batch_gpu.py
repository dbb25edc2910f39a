"""GPU tier: the residual and the refinement on batches — one problem (the fronts), three (the pair lists) and 64 (the
interleaved kernels, SLPX_IL_MIN_BATCH), every problem with values of its own.

An instance's r and norm depend on nothing but its own lhs, rhs, p and (delta, gamma): at every batch size every slot
equals the host body of row_residual on what that slot holds, bit for bit, and two slots of a batch that hold the
same values — and so, by the batched factorizations' own contract, the same p — give the same bits.  Under a mask the
other instances' r, norm and p keep their bits."""
import numpy as np
import pytest

from tests.support import cases
from tests.support import refine_cases as rc

pytestmark = pytest.mark.gpu

N = 6
REG = rc.REG  # (counters (n, m_e, 0, 0) at all 64 states on the host interpreter; asserted here from the device's)


def _batch(B):
    """Problem b at the seeded state of seed SEED + b, the LAST slot a copy of slot 0's values."""
    seeds = [cases.SEED + b for b in range(B)]
    if B > 1:
        seeds[-1] = seeds[0]
    pp, system = rc.seeded_system("cart_pole", N, batch=B, seeds=seeds)
    n, m_e = system.info["n"], system.info["m_e"]
    stats = system.factor(*REG)
    assert np.all(stats[:, :4] == np.array([n, m_e, 0, 0])), stats
    system.solve()
    return pp, system


@pytest.mark.parametrize("B", [1, 3, 64])
def test_every_slot_equals_the_host_body_and_equal_values_give_equal_bits(B):
    pp, system = _batch(B)
    r, norm = system.residual()
    for b in sorted({0, 1 % B, B // 2, B - 1}):
        r_host, _, _, _ = rc.host_residual(system, REG, b)
        assert rc.same_bits(r[b], r_host), (B, b)
        assert rc.same_bits(norm[b], np.max(np.abs(r_host))), (B, b)
    if B > 1:
        assert rc.same_bits(system.get("p")[0], system.get("p")[B - 1])
        assert rc.same_bits(r[0], r[B - 1]) and rc.same_bits(norm[0], norm[B - 1])
        assert not rc.same_bits(r[0], r[1])  # (distinct values in between)
    system.close()
    pp.close()


@pytest.mark.parametrize("B", [3, 64])
def test_mask_leaves_the_other_instances_alone(B):
    pp, system = _batch(B)
    p0, rhs0 = system.get("p"), system.get("rhs")
    r_all, norm_all = system.residual()
    mask = np.zeros(B, dtype=np.uint8)
    mask[[1, B - 1]] = 1
    sentinel = (np.full_like(r_all, 7.0), np.full(B, 7.0))
    r, norm = system.residual(mask=mask, out=sentinel)
    for b in range(B):
        if mask[b]:
            assert rc.same_bits(r[b], r_all[b]) and rc.same_bits(norm[b], norm_all[b])
        else:
            assert np.all(r[b] == 7.0) and norm[b] == 7.0
    norms, accepted = system.refine(2, mask=mask)
    p1 = system.get("p")
    for b in range(B):
        if mask[b]:
            assert rc.same_bits(norms[b, 0], norm_all[b]) and accepted[b] >= 1 and not rc.same_bits(p1[b], p0[b])
        else:
            assert np.all(np.isnan(norms[b])) and accepted[b] == 0 and rc.same_bits(p1[b], p0[b])
    assert rc.same_bits(system.get("rhs"), rhs0)
    # what the masked run did to an active instance is what the unmasked run does to it
    system.set_rhs(rhs0)
    system.factor(*REG)
    system.solve()
    norms_all, accepted_all = system.refine(2)
    p2 = system.get("p")
    for b in np.nonzero(mask)[0]:
        assert rc.same_bits(norms_all[b], norms[b]) and accepted_all[b] == accepted[b] and rc.same_bits(p2[b], p1[b])
    system.close()
    pp.close()


@pytest.mark.parametrize("B", [3, 64])
def test_refinement_of_a_batch_is_instance_by_instance(B):
    """Every instance: norms decrease over the steps taken, at least one is taken, and the p left behind has the norm
    reported last; the two slots with equal values end with equal bits."""
    pp, system = _batch(B)
    norms, accepted = system.refine(3)
    _, norm_after = system.residual()
    for b in range(B):
        k = int(accepted[b])
        assert k >= 1, (b, norms[b])
        assert np.all(np.diff(norms[b, :k + 1]) < 0)
        assert rc.same_bits(norm_after[b], norms[b, k])
    assert rc.same_bits(norms[0], norms[B - 1]) and rc.same_bits(system.get("p")[0], system.get("p")[B - 1])
    system.close()
    pp.close()
