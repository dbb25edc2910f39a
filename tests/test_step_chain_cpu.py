"""The ledger of the chained-step protocol (csrc/chain_ledger.hpp) on the CPU, through the stand-alone program
tests/support/chaincheck_main.cpp, plain and built with -fsanitize=address,undefined.

The expected lines are written out here from the rule ("chained steps"), not computed by the class:

  * a sweep chains only directly behind a step: whatever else was handed the main stream since ("touch") sends the
    sweep there too, without a step number.  A new ledger counts as touched (the state is uploaded first), so the very
    first sweep goes to the main stream and the first CHAINED sweep is the second one;
  * chained sweep k waits for every workgroup of the chained step kernels so far — or, behind a step kernel that was
    not chained, for an event and no word (wait_step 0);
  * step k waits for every workgroup of the chained sweeps so far, its own included;
  * before a step number reaches 2^30 - 1 or a total 2^29: one sweep behind a drain ("restart"), counts from zero.

Every script uses 3 workgroups per sweep and 5 per step kernel.
"""
import pytest

from tests.support import chaincheck

W, S = 3, 5
T = 1 << 29
FIRST = ["sweep 3", "step 5"]  # the first step of a ledger: the main stream
FIRST_OUT = ["sweep: main order_pending 0", "step: chained 0 wait_step 0 this_step 0"]


def chained_sweep(wait_step, this_step, order_by_event=0):
    return f"sweep: chained wait_step {wait_step} this_step {this_step} order_by_event {order_by_event}"


def step(chained, wait_step, this_step):
    return f"step: chained {chained} wait_step {wait_step} this_step {this_step}"


def state(event, step_number, sweep_total, step_total, last_step_chained, pending, touched, failures=0):
    return (f"{event}: step_number {step_number} sweep_total {sweep_total} step_total {step_total} "
            f"last_step_chained {last_step_chained} pending {pending} touched {touched} failures {failures}")


@pytest.fixture(params=[False, True], ids=["plain", "sanitized"])
def run(request):
    return lambda events: chaincheck.run(events, sanitized=request.param)


def test_ten_chained_steps_in_a_row(run):
    out = run(FIRST + ["sweep 3", "step 5"] * 10)
    expect = list(FIRST_OUT)
    # the first chained sweep follows a step kernel that signals no word: an event, wait_step 0
    expect += [chained_sweep(0, 1, order_by_event=1), step(1, 3, 1)]
    for k in range(2, 11):
        expect += [chained_sweep(5 * (k - 1), k), step(1, 3 * k, k)]
    assert out == expect
    assert out[-2:] == ["sweep: chained wait_step 45 this_step 10 order_by_event 0", "step: chained 1 wait_step 30 this_step 10"]


def test_touch_between_steps(run):
    out = run(FIRST + ["sweep 3", "step 5"] * 2 + ["touch", "sweep 3", "step 5", "sweep 3", "step 5", "sweep 3", "step 5"])
    assert out[6:] == [
        "touch: order_by_event 0",
        "sweep: main order_pending 0",  # the main stream, no step number
        step(0, 0, 2),                  # not chained; the number of the last chained step is handed over as it is
        chained_sweep(0, 3, order_by_event=1),  # behind an unchained step kernel: an event
        step(1, 9, 3),                  # three chained sweeps so far
        chained_sweep(15, 4),           # three chained step kernels so far
        step(1, 12, 4),
    ]


def test_touch_while_a_sweep_is_pending(run):
    out = run(FIRST + ["sweep 3", "touch", "step 5", "sweep 3", "step 5"])
    assert out[2:] == [
        chained_sweep(0, 1, order_by_event=1),
        "touch: order_by_event 1",  # the main stream waits for the sweep in flight
        step(0, 0, 1),
        "sweep: main order_pending 0",
        step(0, 0, 1),
    ]


def test_sweep_after_sweep(run):
    out = run(FIRST + ["sweep 3", "sweep 3", "step 5", "sweep 3", "step 5"])
    assert out[2:] == [
        chained_sweep(0, 1, order_by_event=1),
        "sweep: main order_pending 1",  # the sweep nobody consumed first, by an event; then the main stream
        step(0, 0, 1),
        chained_sweep(0, 2, order_by_event=1),  # last_step_chained is false
        step(1, 6, 2),                  # both chained sweeps ran and count
    ]


def test_twin_clears_pending_and_chaining(run):
    out = run(FIRST + ["sweep 3", "twin", "sweep 3", "step 5", "twin", "sweep 3"])
    assert out[2:] == [
        chained_sweep(0, 1, order_by_event=1),
        state("twin", 1, 3, 0, 0, 0, 0),
        chained_sweep(0, 2, order_by_event=1),
        step(1, 6, 2),
        state("twin", 2, 6, 5, 0, 0, 0),
        chained_sweep(0, 3, order_by_event=1),  # behind a twin launch: an event again
    ]


def test_totals_restart_before_their_bound(run):
    # (20 workgroups of headroom at 5 per step kernel: the step kernels' total reaches 2^29 with the FOURTH chained step,
    # 20 / 5 = 4, so the restart is the fifth chained sweep's)
    out = run(["start 20"] + FIRST + ["sweep 3", "step 5"] * 7)
    assert out == [
        state("start", 0, T - 20, T - 20, 0, 0, 1),
        "sweep: main order_pending 0", step(0, 0, 0),
        chained_sweep(0, 1, order_by_event=1), step(1, T - 17, 1),
        chained_sweep(T - 15, 2), step(1, T - 14, 2),
        chained_sweep(T - 10, 3), step(1, T - 11, 3),
        chained_sweep(T - 5, 4), step(1, T - 8, 4),  # the step kernels' total is 2^29 now
        "sweep: restart order_pending 0", step(0, 0, 0),
        chained_sweep(0, 1, order_by_event=1), step(1, 3, 1),  # counts from zero, the same rules
        chained_sweep(5, 2), step(1, 6, 2),
    ]
    assert sum(line.startswith("sweep: restart") for line in out) == 1


def test_step_numbers_restart_before_their_bound(run):
    last = (1 << 30) - 1
    out = run([f"start {1 << 28} {last - 1}"] + FIRST + ["sweep 3", "step 5"] * 3)
    assert out == [
        state("start", last - 1, 1 << 28, 1 << 28, 0, 0, 1),
        "sweep: main order_pending 0", step(0, 0, last - 1),
        chained_sweep(0, last, order_by_event=1), step(1, (1 << 28) + 3, last),
        "sweep: restart order_pending 0", step(0, 0, 0),
        chained_sweep(0, 1, order_by_event=1), step(1, 3, 1),
    ]
    assert sum(line.startswith("sweep: restart") for line in out) == 1


def test_break_adds_to_a_nonzero_wait_once(run):
    out = run(FIRST + ["break", "sweep 3", "step 5", "sweep 3", "step 5", "sweep 3", "step 5"])
    assert out[2:] == [
        state("break", 0, 0, 0, 0, 0, 0),
        chained_sweep(0, 1, order_by_event=1),  # a zero wait_step is left alone (and the break stays armed)
        step(1, 3, 1),
        chained_sweep(5 + (1 << 20), 2),
        step(1, 6, 2),
        chained_sweep(10, 3),
        step(1, 9, 3),
    ]


def test_fail(run):
    out = run(FIRST + ["sweep 3", "step 5"] * 2 + ["sweep 3", "fail", "sweep 3", "step 5", "sweep 3", "fail"])
    assert out[6:] == [
        chained_sweep(10, 3),
        state("fail", 3, 0, 0, 0, 0, 1, failures=1),  # the step number is kept
        "sweep: main order_pending 0",
        step(0, 0, 3),
        chained_sweep(0, 4, order_by_event=1),
        state("fail", 4, 0, 0, 0, 0, 1, failures=2),
    ]


@pytest.mark.parametrize("speculation", [["sweep 3", "step 5"], ["sweep 3", "twin"], ["twin"]], ids=["sweep-step", "sweep-twin", "twin"])
def test_restore_undoes_a_speculative_launch(run, speculation):
    """A speculative launch is made by the resident interior-point driver behind its own kernels on the main stream
    (touched): its sweep goes there and moves neither the step number nor the totals — those count what the device
    was handed and are not part of the book."""
    head = FIRST + ["sweep 3", "step 5"] * 2 + ["touch"]
    tail = ["sweep 3", "step 5"] * 3
    plain = run(head + tail)
    with_speculation = run(head + ["save"] + speculation + ["restore"] + tail)
    assert with_speculation[len(head)] == state("save", 2, 6, 10, 1, 0, 1)
    assert with_speculation[len(head) + 1 + len(speculation)] == state("restore", 2, 6, 10, 1, 0, 1)
    assert with_speculation[-len(tail):] == plain[-len(tail):]
    assert plain[-len(tail):] == [
        "sweep: main order_pending 0", step(0, 0, 2),
        chained_sweep(0, 3, order_by_event=1), step(1, 9, 3),
        chained_sweep(15, 4), step(1, 12, 4),
    ]


def test_restore_leaves_what_the_device_was_handed(run):
    """The book is last_step_chained, pending and touched only.  A speculative sweep that DID chain (no touch in front
    of save) has been handed its step number and its workgroups are counted in the words: restore() puts neither the
    step number nor the totals back, as before the ledger existed."""
    head = FIRST + ["sweep 3", "step 5"] * 2
    out = run(head + ["save", "sweep 3", "step 5", "restore", "sweep 3", "step 5"])
    assert out[len(head):] == [
        state("save", 2, 6, 10, 1, 0, 0),
        chained_sweep(10, 3), step(1, 9, 3),
        state("restore", 3, 9, 15, 1, 0, 0),  # numbers and totals stay where the launches left them
        chained_sweep(15, 4), step(1, 12, 4),
    ]
    out = run(head + ["save", "sweep 3", "restore", "sweep 3", "step 5"])
    assert out[len(head):] == [
        state("save", 2, 6, 10, 1, 0, 0),
        chained_sweep(10, 3),
        state("restore", 3, 9, 10, 1, 0, 0),  # pending is put back; the sweep that ran still counts
        chained_sweep(10, 4), step(1, 12, 4),
    ]
