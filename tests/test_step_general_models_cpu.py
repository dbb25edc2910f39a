"""CPU tier: the plans of the general models of tests/support/step_models.py — fr_models.chain(n), and hub(n, he, hi),
whose last variable is in `he` equality and `hi` inequality rows — against the oracle's Newton step, and the limits of
the packers (csrc/device_images.cpp) from both sides:

  * the source word of a multifrontal task image holds an entry of n_a < 256 direct or A_e^T y terms and n_b < 128
    A_i^T or product terms (device_layout.h: mf_term_code_fits); one more of either and build_mf_images declines — the
    pair-list step kernel serves, with the inline terms and back-substitution rows it keeps;
  * build_inline_kkt gives up at an entry of 2048 terms: the stand-alone assembly kernels serve.

What the host checker computes (tests/support/hostcheck.cpp) is the CPU statement that the PLANS of these models are
right whatever kernels serve them; tests/test_step_general_models_gpu.py runs the kernels."""
import pytest

from tests.support import parity, step_models

STEP_MODELS = ["chain130", "chain300", "chain900", "hub530_255_127", "hub530_256_127", "hub530_255_128", "hub2300_1100_1000"]
DIMS = {"chain130": (130, 63, 282), "chain300": (300, 148, 622), "chain900": (900, 448, 1822), "hub40_3_3": (40, 3, 42),
        "hub530_255_127": (530, 255, 656), "hub530_256_127": (530, 256, 656), "hub530_255_128": (530, 255, 657),
        "hub2300_1100_1000": (2300, 1100, 3299)}


@pytest.fixture()
def under_mf(monkeypatch):
    """the plan options of a single problem's system (system_choice.cpp: the fronts), whatever the suite was started under"""
    monkeypatch.setenv("SLPX_LDLT_MF", "1")


# (kkt.ok / bs.ok None: not stated)
@pytest.mark.parametrize("name,declined,kkt_ok,bs_ok", [
    ("hub530_255_127", 0, 1, 1),        # 1 + 255 + 127 terms in the hub's row of the right-hand side: the word is full
    ("hub530_256_127", 1, 1, 1),        # one A_e^T y term more
    ("hub530_255_128", 1, 1, 1),        # one A_i^T term more
    ("hub2300_1100_1000", 1, 0, None),  # 1 + 1100 + 1000 >= 2048 terms: no inline terms at all, so no image either
])
def test_limits_of_the_packers_from_both_sides(fresh, hostcheck, under_mf, name, declined, kkt_ok, bs_ok):
    from tests.support import imagecheck

    _, pp = step_models.build_both(name)
    hc = hostcheck.HostCheck(pp.p)
    im = imagecheck.Images(hc)
    try:
        assert (hc.n, hc.m_e, hc.m_i) == DIMS[name] and not hc.dense
        assert im.scalar("l.mf") == 1  # (the plan has fronts: what declines is the image)
        assert im.scalar("mf.declined") == declined
        assert im.scalar("kkt.ok") == kkt_ok
        assert bs_ok is None or im.scalar("bs.ok") == bs_ok
        if kkt_ok:
            vsrc = im.array("kkt.vsrc", "i4").astype("i8")
            most = int((-(vsrc[vsrc < -1] + 2) >> 20).max())
            n, me, mi = DIMS[name]
            assert most == 1 + me + (mi - (n - 1))  # the hub's row: its gradient term, every equality row, every hub row
    finally:
        im.close()
        hc.close()


@pytest.mark.parametrize("name", sorted(step_models.INDEFINITE))
def test_indefinite_states_climb_the_ladder_clear_of_any_borderline(fresh, hostcheck, under_mf, name):
    """The states of step_models.indefinite_state, at which the GPU tier compares the product's (delta, gamma) with the
    oracle's: the oracle's loop (sparse_regularized_ldlt.hpp:64-152) ends at delta = 1 or 10, and on the host checker's
    factorization of every rung of that ladder — (0, 0), then delta = 1e-4 x 10^k with gamma = 1e-10 — the inertia is
    wrong by whole pivots up to the last rung and right there, with no pivot below 1e-8 anywhere: the pivots are
    differences of terms of order 1 to 1e3, whose rounding is below 1e-12, so no sign, and no decision of the loop, is
    left to the order of a sum."""
    import numpy as np

    po, pp = step_models.build_both(name)
    hc = hostcheck.HostCheck(pp.p)
    try:
        op = po.p
        n, me, mi = DIMS[name]
        scales = op.scaling()
        hc.set_scaling(scales)
        x, s, y, z, mu = step_models.indefinite_state(name, op.get_x(), n, me, mi, scales[0])
        info, _ = op.newton_step(x, s, y, z, mu, True, hc.perm())
        delta, gamma, nfact, _ = op.reg()
        assert info == 0 and (delta, gamma) == (10.0 if name.startswith("hub") else 1.0, 1e-10)
        hc.sweep(x, y, z, True)
        hc.assemble(s, z)
        hc.rhs(s, y, z, mu)
        rungs, d = [(0.0, 0.0)], 1e-4
        while d < delta:
            rungs.append((d, 1e-10))
            d *= 10.0
        assert d == delta and len(rungs) + 1 == nfact
        smallest = []
        for dd, gg in rungs + [(delta, gamma)]:
            D, stats = hc.factor(dd, gg)
            pos, neg, zero, bad = (int(v) for v in stats[:4])
            smallest.append(float(np.min(np.abs(D))))
            assert bad == 0 and zero == 0 and pos + neg == n + me
            assert (neg > me) == (dd < delta), (dd, pos, neg)
        print(name, "smallest |pivot| per rung", ["%.1e" % v for v in smallest])
        assert min(smallest) >= 1e-8
    finally:
        hc.close()


@pytest.mark.parametrize("case", ["step0", "interior"])
@pytest.mark.parametrize("name", STEP_MODELS + ["hub40_3_3"])
def test_plans_of_general_models_match_oracle(fresh, hostcheck, under_mf, name, case):
    po, pp = step_models.build_both(name)
    assert po.p.dims == pp.p.dims == DIMS[name]
    hc = hostcheck.HostCheck(pp.p)
    try:
        assert not hc.dense
        parity.check_newton_step(hc, po.p, case)
    finally:
        hc.close()
