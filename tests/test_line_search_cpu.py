"""The line searches of the solver drivers (csrc/ipm_line_search.hpp: the filter line search every driver but Newton
runs, and Newton's own — below), without a GPU: a scripted list of
answers goes in, the sequence of requests and the end state come out (tests/support/hostcheck.cpp: hc_line_search).

The expected sequences are written from the reference's lines (interior_point.hpp:512-716, filter.hpp:109-172), not
from the code under test.  Throughout: mu = 0 (an entry's cost is f), D_phi = 0 (the switching condition is off, so
a trial point passes the filter's rules iff  f <= f_cur - alpha^1.5 1e-8 viol_cur  or
viol <= (1 - alpha^1.5 1e-5) viol_cur), the current iterate is (f, violation) = (10, 1) unless said otherwise, and
the filter was made for an initial violation of 1: max_constraint_violation = 1e4.
"""
import itertools
import math

import pytest

from tests.support.hostcheck import line_search, newton_search

AZ = 0.9                                         # alpha_z of the Newton direction
START = (1.0, AZ, 0.0, 0.0, 10.0, 0.0, 1.0)      # alpha_max, alpha_z, D_phi, mu, f, sum ln s, violation
GOOD = (9.0, 0.5, 0.0, 1.0)                      # f, violation, sum ln s, finite: lower cost, half the violation
NAN = (float("nan"), 0.0, 0.0, 0.0)              # not finite
WORSE = (11.0, 2.0, 0.0, 1.0)                    # higher cost, twice the violation: rejected, violation not reduced
MAXV = 1e4


def req(kind, alpha, alpha_z, on_correction=False):
    """a trial point wanted at (alpha, alpha_z), along the correction's direction or the Newton direction"""
    return (kind, alpha, alpha_z, on_correction)


def solve(first, alpha_soc):
    """a correction solve wanted: the first of its rounds or not, accumulating with alpha_soc (:611-612)"""
    return ("soc_solve", first, alpha_soc)


def check(rows, expected):
    assert len(rows) == len(expected), rows
    for got, want in zip(rows, expected):
        if got[0] == "soc_solve":
            got = (got[0], got[4], got[5])
        elif got[0] != "done":
            got = got[:4]
        assert got == want, (got, want, rows)


def test_first_trial_accepted():
    rows = line_search([(START, [GOOD])])
    check(rows, [req("eval", 1.0, AZ), ("done", "newton", False, 1.0, AZ, 0, MAXV, False)])


def test_nonfinite_trial_values_halve_the_step_down_to_restoration():
    """:532-542.  2^-23 = 1.19e-7 is still a step, 2^-24 = 5.96e-8 is below alpha_min = 1e-7: 24 trial points, 24
    halvings, restoration.  A non-finite trial point is not a rejected full step: the counter stays."""
    rows = line_search([(START, [NAN] * 24)])
    check(rows, [req("eval", 0.5 ** k, AZ) for k in range(24)] + [("done", "none", True, 0.5 ** 24, AZ, 0, MAXV, False)])


def soc_rounds(violations, a_soc, az_soc):
    """answers and expected requests of correction rounds whose trial points come back with these violations"""
    answers, expected = [], []
    accumulate_with = 1.0  # :566: alpha_soc starts as the rejected full step
    for k, v in enumerate(violations):
        expected += [solve(k == 0, accumulate_with), req("soc_eval", a_soc, az_soc, True)]
        answers += [(a_soc, az_soc), (11.0, v, 0.0, 1.0)]
        accumulate_with = a_soc  # :623
    return answers, expected


def test_five_rejected_corrections_then_halving_resumes_on_the_newton_direction():
    """:561-664.  The full step is rejected with the violation doubled; five rounds, each rejected (cost up, violation
    above the current one) with the violation falling by more than 1 %: 1.9 <= 0.99 * 2, 1.8 <= 0.99 * 1.9, ...  After
    the fifth the full step counts as rejected (:669) and the search goes on at alpha_max / 2 along the Newton
    direction, with the Newton direction's alpha_z."""
    answers, expected = soc_rounds([1.9, 1.8, 1.7, 1.6, 1.5], 0.8, 0.7)
    rows = line_search([(START, [WORSE] + answers + [GOOD])])
    check(rows, [req("eval", 1.0, AZ)] + expected + [req("eval", 0.5, AZ), ("done", "newton", False, 0.5, AZ, 1, MAXV, False)])


def test_corrections_stop_when_the_violation_falls_by_less_than_one_percent():
    """:653.  1.99 > 0.99 * 2: no second round."""
    answers, expected = soc_rounds([1.99], 0.8, 0.7)
    rows = line_search([(START, [WORSE] + answers + [GOOD])])
    check(rows, [req("eval", 1.0, AZ)] + expected + [req("eval", 0.5, AZ), ("done", "newton", False, 0.5, AZ, 1, MAXV, False)])
    # 1.97 <= 0.99 * 2 is followed by a second round, 1.96 > 0.99 * 1.97 by no third
    answers, expected = soc_rounds([1.97, 1.96], 0.8, 0.7)
    rows = line_search([(START, [WORSE] + answers + [GOOD])])
    check(rows, [req("eval", 1.0, AZ)] + expected + [req("eval", 0.5, AZ), ("done", "newton", False, 0.5, AZ, 1, MAXV, False)])


def test_an_accepted_correction_ends_with_its_step_sizes():
    """:637-642.  The second round's trial point is accepted: alpha = alpha_soc, alpha_z = alpha_z_soc.  That is not
    the full step alpha_max, so a counter of 2 rejected full steps stays (:773 resets it for alpha == alpha_max)."""
    rows = line_search([(START, [WORSE, (0.8, 0.7), (11.0, 1.9, 0.0, 1.0), (0.6, 0.5), GOOD])], counter=2)
    check(rows, [req("eval", 1.0, AZ),
                 solve(True, 1.0), req("soc_eval", 0.8, 0.7, True),
                 solve(False, 0.8), req("soc_eval", 0.6, 0.5, True),
                 ("done", "correction", False, 0.6, 0.5, 2, MAXV, False)])


def test_fourth_full_step_rejected_by_the_table_resets_the_filter():
    """:669-684.  The first search's accepted step puts (10 - 1e-8, 1 - 1e-5) into the table (filter.hpp:140-172).
    Then four searches from (20, 1.5) whose full step (12, 1.2) passes the rules (violation down by a fifth) but is
    dominated by that entry: rejected due to the table, no corrections (the violation went down), halved, accepted at
    alpha_max / 2 — which is no full step, so the counter runs 1, 2, 3.  The fourth rejection makes it 4, and
    max_constraint_violation = 1e4 > 1.5 / 10: the filter is reset, its max_constraint_violation is a tenth, and the
    SAME step is evaluated again — and accepted by the empty table, a full step: the counter is 0 again."""
    later = (1.0, AZ, 0.0, 0.0, 20.0, 0.0, 1.5)
    dominated, ok = (12.0, 1.2, 0.0, 1.0), (9.0, 0.5, 0.0, 1.0)
    rows = line_search([(START, [GOOD])] + [(later, [dominated, ok])] * 3 + [(later, [dominated, dominated])])
    expected = [req("eval", 1.0, AZ), ("done", "newton", False, 1.0, AZ, 0, MAXV, False)]
    for k in (1, 2, 3):
        expected += [req("eval", 1.0, AZ), req("eval", 0.5, AZ), ("done", "newton", False, 0.5, AZ, k, MAXV, True)]
    expected += [req("eval", 1.0, AZ), req("eval", 1.0, AZ), ("done", "newton", False, 1.0, AZ, 0, MAXV * 0.1, False)]
    check(rows, expected)


def test_steps_below_the_floor_fall_back_on_the_kkt_error_at_the_full_step():
    """:686-716.  Every trial point is rejected (cost up, violation not down by the factor 1 - alpha^1.5 1e-5): the
    full step without corrections (its violation 0.999995 did go down: above 1 - 1e-5, below 1), the shorter ones with
    the violation unchanged.  24 trial points, then the one-norm KKT error at (alpha_max, alpha_z) against the
    current one.  Accepted iff next <= 0.999 * current; alpha stays the halved one either way."""
    stall = [(11.0, 0.999995, 0.0, 1.0)] + [(11.0, 1.0, 0.0, 1.0)] * 23
    evals = [req("eval", 0.5 ** k, AZ) for k in range(24)] + [req("kkt", 1.0, AZ)]
    rows = line_search([(START, stall + [(1.0, 0.999)])])
    check(rows, evals + [("done", "fallback", False, 0.5 ** 24, AZ, 1, MAXV, False)])
    rows = line_search([(START, stall + [(1.0, 0.9991)])])
    check(rows, evals + [("done", "none", True, 0.5 ** 24, AZ, 1, MAXV, False)])


def test_sqp_corrections_keep_the_full_step():
    """sqp.hpp:397-468 through the same machine.  The SQP driver moves y with the primal step: it reads alpha alone
    (the machine takes no decision from alpha_z), starts at alpha_max = 1 and answers every correction solve with the
    full step, since sqp.hpp never recomputes alpha_soc.  So every round accumulates with 1 and is evaluated at 1;
    after five the halving resumes at 1 / 2."""
    start = (1.0, 1.0, 0.0, 0.0, 10.0, 0.0, 1.0)
    answers, expected = [], []
    for k, v in enumerate([1.9, 1.8, 1.7, 1.6, 1.5]):
        answers += [(1.0, 1.0), (11.0, v, 0.0, 1.0)]
        expected += [solve(k == 0, 1.0), req("soc_eval", 1.0, 1.0, True)]
    rows = line_search([(start, [WORSE] + answers + [GOOD])])
    check(rows, [req("eval", 1.0, 1.0)] + expected + [req("eval", 0.5, 1.0), ("done", "newton", False, 0.5, 1.0, 1, MAXV, False)])


# ---- Newton's own search (csrc/ipm_line_search.hpp: NewtonSearch; hostcheck.cpp: hc_newton_search) ----
#
# The machine against a restatement of the reference's lines (newton.hpp: the loop "until a step is accepted" of
# newton(), and filter.hpp:109-172 for entries without a constraint violation), fed the same scripted answers.

REDUCTION, FLOOR, DECREASE = 0.5, 1e-20, 0.999   # α_reduction_factor, α_min, the fallback's factor, as the reference has them
# trial points it takes to pass the floor: the first k with REDUCTION^k < FLOOR
TO_THE_FLOOR = next(k for k in itertools.count(1) if REDUCTION ** k < FLOOR)
DESCENT = -1.0                                   # D_phi of a descent direction
NONFINITE = (float("nan"), False)


class ReferenceFilter:
    """filter.hpp:109-172 where every entry's constraint violation is 0 (an unconstrained problem): the violation
    tests pass (0 <= max, 0 <= min_constraint_violation, 0 <= (1 - phi gamma) 0), the table holds costs."""

    def __init__(self):
        self.table = []

    def try_add(self, f_cur, f_trial, D_phi, alpha):
        if not math.isfinite(f_trial):
            return False
        switching = D_phi < 0 and alpha * (-D_phi) ** 2.3 > 0.0 ** 1.1
        armijo = f_trial <= f_cur + 1e-8 * alpha * D_phi
        if switching and not armijo:
            return False                          # (otherwise: sufficient decrease holds by the violation's test)
        if any(cost <= f_trial for cost in self.table):
            return False                          # dominated by an entry of the table
        if not switching or not armijo:
            self.table = [cost for cost in self.table if not f_cur <= cost] + [f_cur]
        return True


def reference_newton_search(filt, f, D_phi, answers):
    """The reference's loop; `answers` as hc_newton_search takes them.  Returns the rows expected of the machine."""
    alpha_max = 1.0
    alpha = alpha_max
    rows = []
    while True:
        rows.append(("eval", alpha))
        trial_f, finite = next(answers)
        if not finite:
            alpha *= REDUCTION
            if alpha < FLOOR:
                return rows + [("done", True)], f
            continue
        if filt.try_add(f, trial_f, D_phi, alpha):
            return rows + [("done", False, alpha, trial_f, alpha)], trial_f
        alpha *= REDUCTION
        if alpha < FLOOR:
            rows.append(("kkt", alpha_max))
            current, at_full_step, f_at_full_step = next(answers)
            if at_full_step <= DECREASE * current:
                return rows + [("done", False, alpha_max, f_at_full_step, alpha)], f_at_full_step
            return rows + [("done", True)], f


def newton_rows(f0, searches):
    """the machine's rows, checked against the reference's restatement; a failed search's end is ("done", True)"""
    got = [r[:2] if r[0] == "done" and r[1] else r for r in newton_search(f0, searches)]
    filt, f, expected = ReferenceFilter(), f0, []
    for D_phi, answers in searches:
        rows, f = reference_newton_search(filt, f, D_phi, iter(answers))
        expected += rows
    assert got == expected, (got, expected)
    return got


def test_floor_of_the_newton_search_follows_from_its_constants():
    assert REDUCTION ** (TO_THE_FLOOR - 1) >= FLOOR > REDUCTION ** TO_THE_FLOOR


def test_newton_first_trial_accepted():
    rows = newton_rows(10.0, [(DESCENT, [(9.0, True)])])
    assert rows == [("eval", 1.0), ("done", False, 1.0, 9.0, 1.0)]


@pytest.mark.parametrize("k", [1, 3, TO_THE_FLOOR - 1])
def test_newton_rejections_then_acceptance(k):
    """k trial points with the cost up, then one with the cost down: accepted at REDUCTION^k.  The accepted cost is what
    the next search compares with: 9.5 is no decrease from 9 (it would have been one from 10)."""
    rows = newton_rows(10.0, [(DESCENT, [(11.0, True)] * k + [(9.0, True)]), (DESCENT, [(9.5, True), (8.0, True)])])
    assert rows[: k + 2] == [("eval", REDUCTION ** j) for j in range(k + 1)] + [("done", False, REDUCTION ** k, 9.0, REDUCTION ** k)]
    assert rows[k + 2:] == [("eval", 1.0), ("eval", REDUCTION), ("done", False, REDUCTION, 8.0, REDUCTION)]


def test_newton_nonfinite_costs_past_the_floor_fail_without_a_fallback():
    rows = newton_rows(10.0, [(DESCENT, [NONFINITE] * TO_THE_FLOOR)])
    assert rows == [("eval", REDUCTION ** j) for j in range(TO_THE_FLOOR)] + [("done", True)]
    # the last trial point decides: non-finite after finite rejections fails, finite after non-finite ones falls back
    rows = newton_rows(10.0, [(DESCENT, [(11.0, True)] * (TO_THE_FLOOR - 1) + [NONFINITE])])
    assert rows[-2:] == [("eval", REDUCTION ** (TO_THE_FLOOR - 1)), ("done", True)]
    rows = newton_rows(10.0, [(DESCENT, [NONFINITE] * (TO_THE_FLOOR - 1) + [(11.0, True), (1.0, 0.5, 7.0)])])
    assert rows[-2:] == [("kkt", 1.0), ("done", False, 1.0, 7.0, REDUCTION ** TO_THE_FLOOR)]


def test_newton_fallback_at_the_full_step_succeeds():
    """Every trial point rejected down to the floor; ||g||_1 at the full step is DECREASE times the current one: the
    full step is committed and the cost kept is the full sweep's.  alpha stays the halved one."""
    stall = [(11.0, True)] * TO_THE_FLOOR
    rows = newton_rows(10.0, [(DESCENT, stall + [(1.0, DECREASE, 7.0)]), (DESCENT, [(7.5, True), (6.0, True)])])
    evals = [("eval", REDUCTION ** j) for j in range(TO_THE_FLOOR)]
    assert rows[: TO_THE_FLOOR + 2] == evals + [("kkt", 1.0), ("done", False, 1.0, 7.0, REDUCTION ** TO_THE_FLOOR)]
    assert rows[TO_THE_FLOOR + 2:] == [("eval", 1.0), ("eval", REDUCTION), ("done", False, REDUCTION, 6.0, REDUCTION)]


def test_newton_fallback_at_the_full_step_fails():
    stall = [(11.0, True)] * TO_THE_FLOOR
    rows = newton_rows(10.0, [(DESCENT, stall + [(1.0, 0.9991, 7.0)])])
    assert rows == [("eval", REDUCTION ** j) for j in range(TO_THE_FLOOR)] + [("kkt", 1.0), ("done", True)]
    rows = newton_rows(10.0, [(DESCENT, stall + [(1.0, float("nan"), 7.0)])])
    assert rows[-1] == ("done", True)


def test_newton_ascent_direction_goes_through_the_table():
    """D_phi >= 0: no switching condition, so an accepted step adds the current cost to the table (filter.hpp:165-169)
    and a later trial point at or above it is rejected as dominated."""
    newton_rows(10.0, [(0.5, [(9.0, True)]), (0.5, [(10.0, True), (8.0, True)])])
