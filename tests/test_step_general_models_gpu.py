"""GPU tier: the fused Newton step (ldlt_mf_step_kernel: the KKT entries evaluated from term lists in LDS, the fronts,
the solve, the back-substitution of p_s and p_z from rows that reach into ancestor tasks) on the general models of
tests/support/step_models.py — not only on the OCP chains of the benchmark, whose entry sums have a dozen terms and whose
inequality rows are plain bounds — and on both sides of the packers' limits (csrc/device_images.cpp):

  chain130 / chain300 / chain900   a hub variable in 24 rows of each kind, inequality rows of two and three columns
  hub40_3_3                        one task
  hub530_255_127                   the hub's row of the right-hand side: 1 + 255 + 127 terms, the source word of a
                                   multifrontal task image full (device_layout.h: mf_term_code_fits)
  hub530_256_127, hub530_255_128   one term more of either kind: the image is declined, the pair-list kernels serve
  hub2300_1100_1000                an entry of >= 2048 terms: no inline terms, the stand-alone assembly kernels serve

The path a system took is read (time_fused_step, info), never assumed, and printed (-s) with the errors found.  Two
further limits are not reached here: a first term index of 16384 and more in a task's block of terms, and a task image
longer than the 96 KB the staging loop requests (kMfImageGroups) — no model of this family gets there at a size a test
of a few seconds can afford.
tests/test_step_general_models_cpu.py asserts the limits themselves and the same steps on the host checker."""
import numpy as np
import pytest

from tests.support import cases, parity, step_models
from tests.test_chained_steps_gpu import _run as run_steps

pytestmark = pytest.mark.gpu

WITHIN = ["chain130", "chain300", "chain900", "hub40_3_3", "hub530_255_127"]
PAST = ["hub530_256_127", "hub530_255_128", "hub2300_1100_1000"]
EPS = 2.0 ** -52


def _path(system):
    """what the system's step is (time_fused_step runs it once on the state set)"""
    t = system.time_fused_step(1)
    return {"one_launch": bool(t["one_launch"]), "multifrontal": bool(t["multifrontal"]), "tasks": system.info["ldlt_tasks"],
            "fronts": system.info["ldlt_fronts"], "mfma_fronts": system.info["ldlt_mfma_fronts"]}


def _set(system, op, state):
    x, s, y, z, mu = state
    system.set_scaling(op.scaling())
    system.set_state(x, s, y, z, np.array([mu]))


# ---- a. the fused step against the oracle ----

@pytest.mark.parametrize("case", ["step0", "interior"])
@pytest.mark.parametrize("name", WITHIN + PAST)
def test_fused_step_of_general_models_against_oracle(fresh, slpx, name, case):
    """check_timed_step after newton_step(True) from a reset regularization.  The models within the limits take the
    multifrontal step in one launch; past a limit the step is not multifrontal (DeviceNlp::step_is_one_launch: only the
    fronts fuse the solve) and is the oracle's all the same.  The interior states are those of cases.SEED, the seed of
    every other parity test: check_timed_step wants the (delta, gamma) of the oracle's own loop."""
    po, pp = step_models.build_both(name)
    system = slpx.System(pp.p, batch=1, device=0)
    try:
        op = po.p
        n, me, mi = system.info["n"], system.info["m_e"], system.info["m_i"]
        state = cases.newton_state(case, op.get_x(), n, me, mi, op.scaling()[0])
        _set(system, op, state)
        path = _path(system)
        print(f"{name} {case}: path {path}")
        if not cases.OUTER_SWITCHES:
            assert system.info["ldlt_dense"] == 0
            if name in WITHIN:
                assert path["one_launch"] and path["multifrontal"], path
            else:
                assert not path["multifrontal"], path
        system.reset_regularization()
        assert np.all(system.newton_step(True) == 0)
        errs = parity.check_timed_step(system, op, state, verbose=True, label=f"{name} {case}")
        assert errs["resid"] <= 1e-10
    finally:
        system.close()


@pytest.mark.parametrize("name", sorted(step_models.INDEFINITE))
def test_fused_step_climbs_the_regularization_ladder_like_the_oracle(fresh, slpx, name):
    """The states of the cases above need no regularization on these models: one factorization each.  At
    step_models.indefinite_state the oracle's loop makes six (the chains) or seven (the hubs) — the product's later
    attempts run on the system the first one evaluated — and the (delta, gamma) it ends at must be the oracle's; on no
    rung is a pivot's sign left to rounding (tests/test_step_general_models_cpu.py)."""
    po, pp = step_models.build_both(name)
    system = slpx.System(pp.p, batch=1, device=0)
    try:
        op = po.p
        n, me, mi = system.info["n"], system.info["m_e"], system.info["m_i"]
        state = step_models.indefinite_state(name, op.get_x(), n, me, mi, op.scaling()[0])
        _set(system, op, state)
        print(f"{name} indefinite: path {_path(system)}")
        system.reset_regularization()
        assert np.all(system.newton_step(True) == 0)
        errs = parity.check_timed_step(system, op, state, verbose=True, label=f"{name} indefinite")
        assert errs["delta"] == (10.0 if name.startswith("hub") else 1.0) and errs["gamma"] == 1e-10
        assert errs["resid"] <= 1e-10
    finally:
        system.close()


# ---- b. the system evaluated in the fronts equals the assembled one, to the bit ----

def _hub_sums(system, state_mu):
    """The hub's row of the right-hand side and the entry (hub, hub) of the matrix as their terms (interior_point.hpp:
    426-448) in longdouble, from what the device holds: -g_h + sum A_e[r, h] y_r + sum A_i[r, h] (-sigma_r c_i_r +
    mu / s_r + z_r) and H_f[h, h] + H_c[h, h] + sum A_i[r, h] sigma_r A_i[r, h], sigma = z / s.
    Returns ((value, number of terms, sum of |terms|) of the row, the same of the entry, position of the entry in lhs)."""
    L = np.longdouble
    I = system.info
    n, me, mi = I["n"], I["m_e"], I["m_i"]
    h = n - 1
    V, s, y, z = (np.asarray(system.get(k)[0], dtype=L) for k in ("V", "s", "y", "z"))
    mu = L(state_mu)
    ci = V[1 + me:1 + me + mi]

    def column(which, off):
        cp, ri = system.pattern(which)
        sl = slice(int(cp[h]), int(cp[h + 1]))
        return ri[sl], V[I[off] + sl.start:I[off] + sl.stop]

    _, g = column(0, "off_g")
    re, ae = column(1, "off_Ae")
    rr, ai = column(2, "off_Ai")
    sigma = z[rr] / s[rr]
    rhs_terms = np.concatenate([-g, ae * y[re], ai * (-sigma * ci[rr] + mu / s[rr] + z[rr])])
    rf, hf = column(3, "off_Hf")
    rc, hc = column(4, "off_Hc")
    lhs_terms = np.concatenate([hf[rf == h], hc[rc == h], ai * sigma * ai])
    lcp, lri = system.pattern(5)
    at = int(lcp[h]) + int(np.flatnonzero(lri[lcp[h]:lcp[h + 1]] == h)[0])
    summary = lambda t: (float(t.sum()), len(t), float(np.abs(t).sum()))
    return summary(rhs_terms), summary(lhs_terms), at


@pytest.mark.parametrize("mf", ["1", "0"])
@pytest.mark.parametrize("name", ["chain300", "hub530_255_127", "hub530_256_127"])
def test_system_evaluated_in_the_step_equals_the_assembled_one_on_general_models(fresh, slpx, monkeypatch, name, mf):
    """tests/test_parity_holes_gpu.py::test_system_evaluated_inside_the_factorization_equals_the_assembled_one on entries
    of 50 (chain300) and 383 terms (hub530_255_127), and on the declined image (hub530_256_127: not multifrontal even
    under SLPX_LDLT_MF=1, the pair-list kernel sums its terms): kkt_terms_sum_grouped and kkt_terms_sum promise the
    bits of the stand-alone assembly kernels (kkt_kernels.h).  And the hub's row of the right-hand side and the entry
    (hub, hub) against their terms summed in longdouble: the kernel's sum has cnt - 1 additions and the negation of
    g, each term a handful of roundings of its own — (cnt + 2) 2^-52 sum |terms| bounds them for cnt >= 25."""
    po, pp = step_models.build_both(name)
    op = po.p
    n, me, mi = pp.p.dims
    state = cases.newton_state("interior", op.get_x(), n, me, mi, op.scaling()[0])
    got = {}
    monkeypatch.setenv("SLPX_LDLT_MF", mf)
    for mode, env in (("inline", {"SLPX_FUSE_KKT_STORE": "1"}), ("assembled", {"SLPX_FUSE_KKT": "0"})):
        for k in ("SLPX_FUSE_KKT_STORE", "SLPX_FUSE_KKT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        system = slpx.System(pp.p, batch=1, device=0)
        try:
            _set(system, op, state)
            assert system.newton_step(True)[0] == 0
            got[mode] = {k: system.get(k)[0].copy() for k in ("lhs", "rhs", "p", "p_s", "p_z", "D")}
            if mode == "inline":
                got["sums"] = _hub_sums(system, state[4])
            got[mode]["mf"] = system.time_fused_step(1)["multifrontal"]
        finally:
            system.close()
    is_mf = bool(got["inline"]["mf"])
    print(f"{name} SLPX_LDLT_MF={mf}: inline system evaluated by the {'multifrontal' if is_mf else 'pair-list'} kernel")
    expect_mf = mf == "1" and name != "hub530_256_127"
    assert (is_mf == expect_mf or bool(cases.OUTER_SWITCHES)) and not got["assembled"]["mf"] and not (is_mf and not expect_mf)
    for k in ("lhs", "rhs"):
        assert np.array_equal(got["inline"][k], got["assembled"][k]), k
    (row, row_cnt, row_abs), (ent, ent_cnt, ent_abs), at = got["sums"]
    # (these ARE the long sums: the gradient term, the hub's equality rows, its inequality rows — chain300's hub has a
    # bound of its own; H_f, H_c and the inequality rows' products)
    assert (row_cnt, ent_cnt) == {"chain300": (1 + 24 + 25, 2 + 25), "hub530_255_127": (1 + 255 + 127, 2 + 127),
                                  "hub530_256_127": (1 + 256 + 127, 2 + 127)}[name]
    err_row, err_ent = abs(got["inline"]["rhs"][n - 1] - row), abs(got["inline"]["lhs"][at] - ent)
    print(f"  hub row of rhs: {row_cnt} terms, error {err_row:.2e} (bound {(row_cnt + 2) * EPS * row_abs:.2e}); "
          f"(hub, hub) of lhs: {ent_cnt} terms, error {err_ent:.2e} (bound {(ent_cnt + 2) * EPS * ent_abs:.2e})")
    assert err_row <= (row_cnt + 2) * EPS * row_abs
    assert err_ent <= (ent_cnt + 2) * EPS * ent_abs
    if not is_mf:
        for k in ("D", "p"):
            assert np.array_equal(got["inline"][k], got["assembled"][k]), k
        for k in ("p_s", "p_z"):
            assert cases.max_rel(got["inline"][k], got["assembled"][k]) <= 1e-14, k
    else:
        Di, Da = got["inline"]["D"], got["assembled"]["D"]
        assert np.array_equal(np.sign(Di), np.sign(Da))
        assert np.median(np.abs(Di - Da) / np.abs(Da)) <= 1e-13
        for k in ("p", "p_s", "p_z"):
            assert cases.max_rel(got["inline"][k], got["assembled"][k]) <= 1e-6, k


# ---- c. a new right-hand side through the fronts ----

@pytest.mark.parametrize("name", ["chain300", "hub530_255_127"])
def test_a_new_right_hand_side_through_the_fronts_of_general_models(fresh, slpx, monkeypatch, name):
    po, pp = step_models.build_both(name)
    system = slpx.System(pp.p, batch=1, device=0)
    monkeypatch.setenv("SLPX_MF_SOLVE", "0")
    other = slpx.System(pp.p, batch=1, device=0)
    monkeypatch.delenv("SLPX_MF_SOLVE")
    try:
        assert cases.OUTER_SWITCHES or system.info["ldlt_multifrontal"] == 1
        parity.check_new_right_hand_sides(system, other, po.p)
    finally:
        system.close()
        other.close()


# ---- d. chained steps ----

@pytest.mark.parametrize("name", ["chain300", "hub530_255_127"])
def test_chained_steps_of_general_models_give_the_bits_of_the_unchained_ones(fresh, slpx, monkeypatch, name):
    """tests/test_chained_steps_gpu.py on three states: p, p_s, p_z and V of chained and unchained steps, to the bit.
    Whether these plans chain at all is system_choice.cpp's (tasks + sum workgroups + 64 <= CUs, and the one-time probe
    that kernels of two streams run side by side): where they do not, the comparison holds trivially.  What is printed
    is read off the device: a chained sweep told to wait for a kernel that does not exist (debug_chain(1)) loses its
    hand-over, once — an unchained system has none to lose.  (On an MI355X that chains cart-pole's steps neither of
    these plans chained when this was written: DeviceNlp::sweep_full_for_step also wants the sweep to be one generated
    kernel, no large or global tape tasks beside its bodies.)"""
    po, pp = step_models.build_both(name)
    op = po.p
    n, me, mi = pp.p.dims
    scales = op.scaling()
    states = [cases.newton_state("interior", op.get_x(), n, me, mi, scales[0], seed=cases.SEED + k) for k in range(3)]
    plain = run_steps(slpx, pp.p, states, scales, False, monkeypatch)
    other = run_steps(slpx, pp.p, states, scales, True, monkeypatch)
    for a, b in zip(plain, other):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert not np.array_equal(plain[0][0], plain[2][0])
    monkeypatch.delenv("SLPX_CHAIN_TAPE", raising=False)
    system = slpx.System(pp.p, batch=1, device=0)
    try:
        _set(system, op, states[0])
        assert np.all(system.newton_steps(5) == 0)
        assert system.debug_chain(0) == 0
        system.debug_chain(1)
        assert np.all(system.newton_steps(3) == 0)
        failures = system.debug_chain(0)
        assert failures in (0, 1)
        system.reset_regularization()
        assert np.all(system.newton_step(True) == 0)
        for u, v in zip(plain[1], [system.get(w)[0] for w in ("p", "p_s", "p_z", "V")]):
            assert np.array_equal(u, v)
        print(f"{name}: {system.info['ldlt_tasks']} tasks, {system.info['tape_global_tasks']} global tape tasks, "
              f"steps {'chained' if failures else 'NOT chained'}")
    finally:
        system.close()


# ---- e. batches ----

@pytest.mark.parametrize("B,items", [(70, (0, 63, 64, 69)), (3, (0, 2))])
def test_batch_timed_step_items_of_a_general_model_against_oracle(fresh, slpx, B, items):
    """chain130 at B = 70 (the interleaved kernels: one chunk of 64 and a ragged one of 6) and B = 3 (the pair lists):
    every checked item against its own oracle step."""
    po, pp = step_models.build_both("chain130")
    op = po.p
    n, me, mi = pp.p.dims
    scales = op.scaling()
    st = [cases.newton_state("interior", op.get_x(), n, me, mi, scales[0], seed=cases.SEED + b) for b in range(B)]
    system = slpx.System(pp.p, batch=B, device=0)
    try:
        system.set_scaling(scales)
        system.set_state(*(np.stack([s[k] for s in st]) for k in range(4)), np.array([s[4] for s in st]))
        system.reset_regularization()
        assert np.all(system.newton_step(True) == 0)
        snap = parity.snapshot_step(system)
        for b in items:
            parity.check_timed_step(system, op, st[b], b=b, verbose=True, label=f"{B} x chain130 item {b}", snap=snap)
    finally:
        system.close()
