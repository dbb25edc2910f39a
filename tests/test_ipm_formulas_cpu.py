"""The interior-point row formulas (sleipnir_amd/csrc/ipm_formulas.h), host instantiation, bit for bit against
Python-float restatements of the reference lines they transcribe (util/fraction_to_the_boundary_rule.hpp:19-43,
interior_point.hpp:797-801, :590-600, :611-616, :625-630), and two properties in exact rational arithmetic.

Python floats are IEEE doubles with one rounding per operation and no fused multiply-add — what the x86 host
build of the bodies does.  (The device instantiation fuses; its bits are pinned by the GPU tier.)"""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests.support import formulacheck

KAPPA = 1e10
TINY = 5e-324  # the smallest subnormal
NAN = float("nan")
INF = float("inf")


def div(a, b):
    """a / b as the hardware does it (Python raises where IEEE gives inf or NaN)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return min(a, b)


def ref_ftb_candidate(acc, tau, p, v):
    return fmin(acc, div(-tau, p) * v) if p < 0.0 else acc


def z_bounds(mu, s):
    return div(1.0 / KAPPA * mu, s), div(KAPPA * mu, s)


def ref_z_reset(z, mu, s):
    lo, hi = z_bounds(mu, s)
    return lo if z < lo else (hi if z > hi else z)  # std::clamp(z, lo, hi)


def ref_soc_rhs_multiplier(mu, s, z, c):
    sinv = div(1.0, s)
    return mu * sinv - (sinv * z) * c


def ref_backsub_pz(mu, s, z, p_s):
    sinv = div(1.0, s)
    return mu * sinv - z - (sinv * z) * p_s


def ref_soc_accumulate(alpha, prev, trial):
    return alpha * prev + trial


def row(acc=1.0, tau=0.99, p=-0.5, v=0.25, z=1.0, mu=0.1, s=0.7, c=0.3, p_s=-0.2, alpha=0.5, prev=0.1, trial=-0.4):
    return [acc, tau, p, v, z, mu, s, c, p_s, alpha, prev, trial]


def table():
    rng = np.random.default_rng(20261019)
    rows = []
    # ordinary values, products that do not round to short decimals
    for _ in range(16):
        u = rng.uniform(0.05, 3.0, 12)
        sg = rng.choice([-1.0, 1.0], 12)
        rows.append(row(acc=min(1.0, u[0]), tau=0.99 + 0.00999 * rng.random(), p=sg[2] * u[2], v=u[3], z=u[4],
                        mu=10.0 ** rng.uniform(-12, 0), s=u[6], c=sg[7] * u[7], p_s=sg[8] * u[8], alpha=u[9] / 3.0,
                        prev=sg[10] * u[10], trial=sg[11] * u[11]))
    # fraction to the boundary: no candidate from p = 0, -0.0, p > 0; a candidate above acc; subnormal p (candidate
    # overflows to +inf: acc stands); a tiny candidate; v = 0
    for p in (0.0, -0.0, 2.5, TINY):
        rows.append(row(p=p))
    rows.append(row(acc=0.125, p=-1e-3, v=5.0))
    rows.append(row(p=-TINY, v=1.0))
    rows.append(row(p=-2e-310, v=1e-300))
    rows.append(row(p=-4.0, v=1e-12))
    rows.append(row(p=-4.0, v=0.0))
    rows.append(row(acc=0.3, tau=0.995, p=-1.0 / 3.0, v=0.1))
    # z reset around [mu / (kappa s), kappa mu / s]: below, above, inside, on each end, one ulp outside each end
    for mu, s in ((0.1, 0.7), (2.0 / 3.0 * 1e-9, 3e-5)):
        lo, hi = z_bounds(mu, s)
        for z in (lo / 2, hi * 2, math.sqrt(lo * hi), lo, hi, math.nextafter(lo, -INF), math.nextafter(lo, INF),
                  math.nextafter(hi, INF), math.nextafter(hi, -INF), -1.0, 0.0):
            rows.append(row(z=z, mu=mu, s=s))
    rows.append(row(z=NAN))                    # returned as it is
    rows.append(row(z=NAN, mu=1e-9, s=12.0))
    rows.append(row(z=1.0, mu=0.0))            # lo = hi = 0
    rows.append(row(z=-1.0, mu=0.0))
    rows.append(row(z=0.0, mu=0.0))
    rows.append(row(z=-0.0, mu=0.0))           # equal to both ends: z itself comes back, sign and all
    rows.append(row(z=1.0, mu=0.1, s=TINY))    # hi (and lo) overflow to +inf
    rows.append(row(z=1.0, mu=1e-300, s=1e-310))  # hi = +inf, lo finite
    rows.append(row(z=INF, mu=1e-300, s=1e-310))
    rows.append(row(z=1.0, mu=0.1, s=-0.7))    # lo > hi: the first comparison that holds decides
    rows.append(row(z=-1e30, mu=0.1, s=-0.7))
    return np.array(rows)


TABLE = table()


@pytest.fixture(scope="module")
def HOST():
    """The host results of the table, computed once."""
    return formulacheck.evaluate(TABLE)


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (a != a and b != b)


def test_the_table_holds_the_special_inputs():
    assert len(TABLE) == 59
    p, z = TABLE[:, 2], TABLE[:, 4]
    assert np.any((p == 0.0) & ~np.signbit(p)) and np.any((p == 0.0) & np.signbit(p))
    assert np.any((p < 0.0) & (np.abs(p) < 2.3e-308)) and np.any(np.isnan(z))
    assert np.any(TABLE[:, 5] == 0.0) and np.any((TABLE[:, 6] > 0.0) & (TABLE[:, 6] < 2.3e-308))


def test_host_bodies_are_the_reference_expressions_bit_for_bit(HOST):
    refs = (lambda r: ref_ftb_candidate(r[0], r[1], r[2], r[3]), lambda r: ref_z_reset(r[4], r[5], r[6]),
            lambda r: ref_soc_rhs_multiplier(r[5], r[6], r[4], r[7]), lambda r: ref_backsub_pz(r[5], r[6], r[4], r[8]),
            lambda r: ref_soc_accumulate(r[9], r[10], r[11]))
    for i, r in enumerate(TABLE):
        r = [float(v) for v in r]
        for k, ref in enumerate(refs):
            with np.errstate(all="ignore"):
                want = float(ref([np.float64(v) for v in r]))
            assert same_bits(HOST[i, k], want), (formulacheck.COLUMNS_OUT[k], i, r, float(HOST[i, k]), want)


def test_z_reset_returns_its_z_or_an_end_of_the_interval_exactly(HOST):
    seen = set()
    for r, out in zip(TABLE, HOST):
        z, got = float(r[4]), float(out[1])
        lo, hi = z_bounds(float(r[5]), float(r[6]))
        which = [name for name, v in (("z", z), ("lo", lo), ("hi", hi)) if same_bits(got, v)]
        assert which, (z, lo, hi, got)
        if z != z:
            assert got != got
            continue
        seen.update(which)
        if lo <= hi and all(math.isfinite(v) for v in (z, lo, hi)):
            assert Fraction(got) == min(max(Fraction(z), Fraction(lo)), Fraction(hi))
    assert seen == {"z", "lo", "hi"}


def test_ftb_candidate_never_exceeds_acc(HOST):
    lowered = 0
    for r, out in zip(TABLE, HOST):
        acc, p, got = float(r[0]), float(r[2]), float(out[0])
        assert Fraction(got) <= Fraction(acc)
        if not p < 0.0:
            assert same_bits(got, acc)
        lowered += got < acc
    assert lowered >= 10


def test_sanitized_probe_runs_clean(HOST):
    """The probe built with -fsanitize=address,undefined (a stand-alone program), once: same answers."""
    san = formulacheck.evaluate(TABLE, sanitized=True)
    same = (san.view(np.uint64) == HOST.view(np.uint64)) | (np.isnan(san) & np.isnan(HOST))
    assert same.all()
