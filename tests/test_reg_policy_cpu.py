"""The regularization policy every factorization driver runs (csrc/ldlt_policy.hpp), without a GPU: a scripted
inertia response goes in, the attempts judged, the launches and the end state come out (tests/support/hostcheck.cpp:
hc_reg_policy runs the loops NewtonSystem::compute, compute_twin and compute_hooked run, over scripted launchers).

The expected sequences come from `reference` below, written from the reference's lines
(util/sparse_regularized_ldlt.hpp:64-152), not from the code under test.  Throughout: n = 5 decision variables and
m_e = 3 equality rows, so the ideal inertia is (5, 3, 0).
"""
import itertools

import pytest

from tests.support.hostcheck import reg_policy

N, ME = 5, 3
INF = float("inf")
EPS = 2.220446049250313e-16
SUCCESS, NUMERICAL_ISSUE = 0, 1

# counters of an attempt: n_pos, n_neg, n_zero, n_bad, min |D|
IDEAL = (5, 3, 0, 0, 1.0)
SMALL = (5, 3, 0, 0, 9.9e-5)   # the ideal inertia, a pivot below 1e-4
NEG = (4, 4, 0, 0, 1.0)        # too many negative pivots
POS = (6, 2, 0, 0, 1.0)        # too many positive pivots
ZERO = (4, 3, 1, 0, 1.0)       # a zero pivot
BAD = (5, 3, 0, 1, 1.0)        # the decomposition failed


def row(counters, delta_below=INF, gamma_below=INF, only_gamma_zero=False):
    return (delta_below, gamma_below, float(only_gamma_zero)) + tuple(counters)


def respond(response, delta, gamma):
    """the counters a response gives the attempt (delta, gamma): its first row that matches"""
    for d_below, g_below, only_zero, *counters in response:
        if delta < d_below and gamma < g_below and (not only_zero or gamma == 0.0):
            return counters
    raise AssertionError("no row answers")


def reference(response, memory=(0.0, 0.0), gamma_min=1e-10, skip_first=False, eliminated_min_pivot=None):
    """sparse_regularized_ldlt.hpp:64-152 -> (attempts, info, memory).  skip_first: the product does not launch an
    unregularized attempt that is known to fail; eliminated_min_pivot: restoration's rows outside the matrix, whose
    pivots belong to D (:83)."""
    prev_delta, prev_gamma = memory
    tried = []
    if not skip_first:
        tried.append((0.0, 0.0))                                            # :74
        pos, neg, zero, bad, min_abs = respond(response, 0.0, 0.0)
        if bad == 0:                                                        # :77
            d_ok = min_abs >= 1e-4 and (eliminated_min_pivot is None or eliminated_min_pivot >= 1e-4)
            if (pos, neg, zero) == (N, ME, 0) and d_ok:                     # :82-83
                return tried, SUCCESS, (0.0, 0.0)                           # :84-86
    delta = 1e-4 if prev_delta == 0.0 else max(prev_delta / 2.0, EPS)       # :95-98
    gamma = gamma_min                                                       # :102
    while True:
        tried.append((delta, gamma))                                        # :105
        pos, neg, zero, bad, _ = respond(response, delta, gamma)
        if bad == 0:                                                        # :108
            if (pos, neg, zero) == (N, ME, 0):                              # :111
                return tried, SUCCESS, (delta, gamma)
            elif zero > 0:                                                  # :116
                if gamma == 0.0:
                    gamma = 1e-10                                           # :120
                else:
                    delta *= 10.0                                           # :124-125
                    gamma *= 10.0
            elif neg > ME:                                                  # :127
                delta *= 10.0
            elif pos > N:                                                   # :131
                gamma = 1e-10 if gamma == 0.0 else gamma * 10.0
        else:                                                               # :136-141
            delta *= 10.0
            gamma = 1e-10 if gamma == 0.0 else gamma * 10.0
        if delta > 1e20 or gamma > 1e20:                                    # :145-150
            return tried, NUMERICAL_ISSUE, (delta, gamma)


def second_stands(mode, first, response):
    """a launch (first | second, mode): is the second the attempt the reference makes after the first?  Mode 2: the
    first is the unregularized attempt, any failure leads to the first guess (:77-102); mode 1: the second is
    delta x 10, the answer to too many negative pivots alone (:127-130); mode 3: gamma x 10, :131-135."""
    pos, neg, zero, bad, min_abs = respond(response, *first)
    ideal = bad == 0 and (pos, neg, zero) == (N, ME, 0)
    if mode == 2:
        return not (ideal and min_abs >= 1e-4)
    inertia_only = bad == 0 and zero == 0 and not ideal
    return inertia_only and (neg > ME if mode == 1 else neg <= ME and pos > N)


def run(driver, response, memory=(0.0, 0.0), **kw):
    return reg_policy(N, ME, [(memory, response)], driver=driver, **kw)


def check(res, expected, b=0):
    attempts, info, memory = expected
    assert res["attempts"][b] == attempts
    assert res["info"][b] == info
    assert res["memory"][b] == memory


def check_all_drivers(response, memory=(0.0, 0.0), gamma_min=1e-10, skip_first=False):
    """the three drivers against the reference; returns its (attempts, info, memory)"""
    expected = reference(response, memory, gamma_min, skip_first)
    for driver in ("sequential", "twin") + (() if skip_first else ("hooked",)):
        res = run(driver, response, memory, gamma_min=gamma_min, skip_first=skip_first)
        check(res, expected)
        assert res["factorizations"] == len(expected[0]), driver
    return expected


def test_a_unregularized_attempt_accepted():
    attempts, info, memory = check_all_drivers([row(IDEAL)], memory=(1e-2, 1e-8))
    assert (attempts, info, memory) == ([(0.0, 0.0)], SUCCESS, (0.0, 0.0))
    res = run("twin", [row(IDEAL)])
    assert res["launches"] == [(0.0, 0.0, 1e-4, 1e-10, 2, True)]
    assert (res["twin_launches"], res["twin_taken"], res["seconds"]) == (1, 0, [])


def test_b_unregularized_attempt_rejected_only_by_a_small_pivot():
    response = [row(SMALL, delta_below=1e-300), row(IDEAL)]
    attempts, info, memory = check_all_drivers(response)
    assert (attempts, info, memory) == ([(0.0, 0.0), (1e-4, 1e-10)], SUCCESS, (1e-4, 1e-10))
    # 1e-4 itself passes (:83 is >=)
    at_threshold = [row((5, 3, 0, 0, 1e-4))]
    assert check_all_drivers(at_threshold)[0] == [(0.0, 0.0)]
    res = run("twin", response)
    assert (res["twin_taken"], res["seconds"]) == (1, [(1e-4, 1e-10)])


def test_b_unregularized_attempt_rejected_only_by_the_eliminated_pivot():
    for pivot, n_attempts in ((9.9e-5, 2), (1e-4, 1), (None, 1)):
        expected = reference([row(IDEAL)], eliminated_min_pivot=pivot)
        assert len(expected[0]) == n_attempts
        res = run("hooked", [row(IDEAL)], eliminated_min_pivot=pivot)
        check(res, expected)
        assert res["twin_taken"] == n_attempts - 1
    # the eliminated pivot belongs to the unregularized attempt alone
    response = [row(NEG, delta_below=1e-3), row(IDEAL)]
    expected = reference(response, eliminated_min_pivot=1e-9)
    assert expected[0] == [(0.0, 0.0), (1e-4, 1e-10), (1e-3, 1e-10)]
    check(run("hooked", response, eliminated_min_pivot=1e-9), expected)


def test_c_delta_ladder():
    response = [row(NEG, delta_below=1.0), row(IDEAL)]
    attempts, _, memory = check_all_drivers(response)
    assert [d for d, _ in attempts] == [0.0, 1e-4, 1e-4 * 10.0, 1e-4 * 10.0 * 10.0, 1e-4 * 10.0 * 10.0 * 10.0, 1e-4 * 10.0 * 10.0 * 10.0 * 10.0]
    assert memory == (attempts[-1][0], 1e-10) and memory[0] >= 1.0
    # from a memory: half of it, then x 10
    attempts, _, _ = check_all_drivers(response, memory=(0.5, 0.0))
    assert [d for d, _ in attempts] == [0.0, 0.25, 2.5]
    # ... but never below the machine epsilon
    attempts, _, memory = check_all_drivers([row(NEG, delta_below=1e-300), row(IDEAL)], memory=(1e-16, 0.0))
    assert attempts == [(0.0, 0.0), (EPS, 1e-10)] and memory == (EPS, 1e-10)
    attempts, _, _ = check_all_drivers([row(NEG, delta_below=1e-300), row(IDEAL)], memory=(4.0 * EPS, 0.0))
    assert attempts[1] == (2.0 * EPS, 1e-10)


def test_d_zero_pivots():
    # gamma = 0: gamma becomes 1e-10 and delta stays; then both x 10
    response = [row(ZERO, gamma_below=1e-8), row(IDEAL)]
    attempts, info, memory = check_all_drivers(response, gamma_min=0.0)
    assert attempts == [(0.0, 0.0), (1e-4, 0.0), (1e-4, 1e-10), (1e-4 * 10.0, 1e-10 * 10.0), (1e-4 * 10.0 * 10.0, 1e-10 * 10.0 * 10.0)]
    assert (info, memory) == (SUCCESS, attempts[-1])
    only_at_zero = [row(ZERO, only_gamma_zero=True), row(IDEAL)]
    assert check_all_drivers(only_at_zero, gamma_min=0.0)[0] == [(0.0, 0.0), (1e-4, 0.0), (1e-4, 1e-10)]
    # gamma_min > 0: both x 10 from the start
    assert check_all_drivers(response)[0][:3] == [(0.0, 0.0), (1e-4, 1e-10), (1e-4 * 10.0, 1e-10 * 10.0)]


@pytest.mark.parametrize("gamma_min", [0.0, 1e-10])
def test_e_too_many_positive_pivots(gamma_min):
    response = [row(POS, gamma_below=1e-7), row(IDEAL)]
    attempts, info, memory = check_all_drivers(response, gamma_min=gamma_min)
    ladder = [1e-10, 1e-10 * 10.0, 1e-10 * 10.0 * 10.0, 1e-10 * 10.0 * 10.0 * 10.0]
    assert ladder[-1] >= 1e-7 > ladder[-2]
    assert attempts == [(0.0, 0.0)] + ([(1e-4, 0.0)] if gamma_min == 0.0 else []) + [(1e-4, g) for g in ladder]
    assert (info, memory) == (SUCCESS, (1e-4, ladder[-1]))


def test_f_failed_decomposition():
    # n_bad != 0 with an otherwise ideal inertia is a failure, at the unregularized attempt and in the loop
    response = [row(BAD, delta_below=1e-2), row(IDEAL)]
    for gamma_min, gammas in ((0.0, [0.0, 1e-10, 1e-10 * 10.0]), (1e-10, [1e-10, 1e-10 * 10.0, 1e-10 * 10.0 * 10.0])):
        attempts, info, memory = check_all_drivers(response, gamma_min=gamma_min)
        assert attempts == [(0.0, 0.0)] + list(zip([1e-4, 1e-4 * 10.0, 1e-4 * 10.0 * 10.0], gammas))
        assert info == SUCCESS and memory == attempts[-1]


@pytest.mark.parametrize("counters", [NEG, POS, ZERO, BAD])
@pytest.mark.parametrize("gamma_min", [0.0, 1e-10])
def test_g_give_up(counters, gamma_min):
    attempts, info, memory = check_all_drivers([row(counters)], gamma_min=gamma_min)
    assert info == NUMERICAL_ISSUE
    # the memory holds the values that overshot: no attempt was made with them
    assert max(memory) > 1e20 and memory != attempts[-1]
    assert all(d <= 1e20 and g <= 1e20 for d, g in attempts)
    assert len(attempts) >= 25


def test_h_skip_first():
    response = [row(NEG, delta_below=1e-3), row(IDEAL)]
    attempts, info, memory = check_all_drivers(response, skip_first=True)
    assert attempts == [(1e-4, 1e-10), (1e-4 * 10.0, 1e-10)]
    res = run("twin", response, skip_first=True)
    assert res["launches"] == [(1e-4, 1e-10, 1e-4 * 10.0, 1e-10, 1, True)]
    assert (res["twin_taken"], res["factorizations"]) == (1, 2)
    # an ideal unregularized inertia changes nothing: the attempt is not made
    assert check_all_drivers([row(IDEAL)], skip_first=True)[0] == [(1e-4, 1e-10)]


@pytest.mark.parametrize("skip_first", [False, True])
def test_i_second_compute_opens_with_the_answer_the_first_drew(skip_first):
    response = [row(POS, gamma_below=1e-8), row(IDEAL)]
    first = run("twin", response, skip_first=skip_first)
    check(first, reference(response, skip_first=skip_first))
    assert first["memory"][0] == (1e-4, 1e-10 * 10.0 * 10.0)
    assert first["twin_expect"] == 3
    # the loop's first launch held delta x 10 (nobody had drawn the gamma answer yet), the later ones too
    assert [l[4] for l in first["launches"]] == [1 if skip_first else 2, 1, 1]
    assert first["twin_taken"] == 0 and first["seconds"] == ([] if skip_first else [(1e-4, 1e-10)])
    second = run("twin", response, memory=first["memory"][0], skip_first=skip_first, twin_expect=first["twin_expect"])
    check(second, reference(response, first["memory"][0], skip_first=skip_first))
    g = [1e-10, 1e-10 * 10.0, 1e-10 * 10.0 * 10.0]
    if skip_first:
        assert second["launches"] == [(5e-5, g[0], 5e-5, g[1], 3, True), (5e-5, g[2], 5e-5 * 10.0, g[2], 1, True)]
        assert second["seconds"] == [(5e-5, g[1])] and second["twin_taken"] == 0
    else:
        assert second["launches"] == [(0.0, 0.0, 5e-5, g[0], 2, True), (5e-5, g[1], 5e-5, g[2], 3, True)]
        assert second["seconds"] == [(5e-5, g[0]), (5e-5, g[2])] and second["twin_taken"] == 1
    assert second["twin_expect"] == 3
    # a compute whose loop's first launch is accepted, or draws too many negative pivots, goes back to delta x 10
    assert run("twin", [row(SMALL, delta_below=1e-300), row(IDEAL)], twin_expect=3, decline=1)["twin_expect"] == 1
    assert run("twin", [row(NEG, delta_below=1e-3), row(IDEAL)], twin_expect=3, skip_first=True)["twin_expect"] == 1
    # ... zero pivots or a failed decomposition leave it, and so does a compute that never reaches the loop
    assert run("twin", [row(BAD, delta_below=1e-3), row(IDEAL)], twin_expect=3, skip_first=True)["twin_expect"] == 3
    assert run("twin", [row(IDEAL)], twin_expect=3)["twin_expect"] == 3
    # the hooked driver neither reads nor writes it: delta x 10 beside every attempt of the loop
    hooked = run("hooked", response, twin_expect=3)
    assert hooked["twin_expect"] == 3 and [l[4] for l in hooked["launches"]] == [2, 1, 1]


def test_j_masked_batch():
    responses = [[row(NEG, delta_below=1e-2), row(IDEAL)], [row(BAD)], [row(POS, gamma_below=1e-9), row(IDEAL)]]
    memories = [(0.0, 0.0), (7.0, 8.0), (1e-3, 1e-9)]
    res = reg_policy(N, ME, list(zip(memories, responses)), mask=[1, 0, 1])
    check(res, reference(responses[0], memories[0]), 0)
    check(res, reference(responses[2], memories[2]), 2)
    assert res["attempts"][1] == [] and res["info"][1] == SUCCESS and res["memory"][1] == (7.0, 8.0)
    # one launch per round of the still-active problems: as many as the longest loop
    assert res["factorizations"] == max(len(res["attempts"][0]), len(res["attempts"][2])) == 4
    # unmasked, the middle problem gives up on its own while the others end as before
    res = reg_policy(N, ME, list(zip(memories, responses)))
    for b in range(3):
        check(res, reference(responses[b], memories[b]), b)
    assert res["info"] == [SUCCESS, NUMERICAL_ISSUE, SUCCESS]


def grid():
    """every response of the property test: a failure below delta*, another below gamma*, the ideal inertia beyond —
    with and without an unregularized attempt that only its small pivot rejects"""
    for d_star, g_star in itertools.product((0.0, 1e-4, 1e-2, 1.0), (0.0, 1e-10, 1e-8)):
        for kind_d, kind_g in itertools.product((NEG, ZERO, BAD), (POS, ZERO, BAD)):
            tail = [row(kind_d, delta_below=d_star), row(kind_g, gamma_below=g_star), row(IDEAL)]
            yield tail
            yield [row(SMALL, delta_below=1e-300)] + tail
            yield [row(ZERO, only_gamma_zero=True)] + tail


def check_launches(res, response):
    """every launch holds the attempt and the reference's answer to the failure its mode names; a second attempt is
    judged exactly where it stands for the attempt the reference makes next"""
    judged = []
    for d0, g0, d1, g1, mode, two in res["launches"]:
        if mode == 2:
            assert (d0, g0) == (0.0, 0.0)
        elif mode == 1:
            assert (d1, g1) == (d0 * 10.0, g0)
        else:
            assert mode == 3 and (d1, g1) == (d0, 1e-10 if g0 == 0.0 else g0 * 10.0)
        if two and second_stands(mode, (d0, g0), response):
            judged.append((d1, g1))
    assert res["seconds"] == judged
    assert res["twin_launches"] == sum(l[5] for l in res["launches"])
    taken = res["info"][0] == SUCCESS and res["last_was_second"]
    assert res["twin_taken"] == int(taken)


@pytest.mark.parametrize("gamma_min", [0.0, 1e-10])
@pytest.mark.parametrize("prev_delta", [0.0, 1e-3, 1e-16])
def test_twin_drivers_follow_the_sequential_policy(gamma_min, prev_delta):
    memory = (prev_delta, 1e-9)
    for response in grid():
        for skip_first in (False, True):
            expected = reference(response, memory, gamma_min, skip_first)
            assert expected[1] == SUCCESS
            seq = run("sequential", response, memory, gamma_min=gamma_min, skip_first=skip_first)
            check(seq, expected)
            for decline in range(16):
                drivers = [("twin", 1), ("twin", 3)] + ([] if skip_first else [("hooked", 1)])
                for driver, expect in drivers:
                    res = run(driver, response, memory, gamma_min=gamma_min, skip_first=skip_first, decline=decline, twin_expect=expect)
                    for key in ("attempts", "info", "memory", "factorizations"):
                        assert res[key] == seq[key], (key, driver, expect, decline, response)
                    check_launches(res, response)
                    if driver == "hooked":
                        assert all(l[4] in (1, 2) for l in res["launches"])
