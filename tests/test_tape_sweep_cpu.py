"""CPU tier of the tape-sweep tests: the mpmath reference (tests/support/mpref.py), the models (tests/support/
tape_models.py) and the conditions the GPU tier relies on, proven without a GPU.  The host interpreter of the compiled
program (HostCheck.sweep: the op_forward of tape_ops.h in hostcheck.cpp's own sequential loop) and the oracle — two
independent double implementations — are each compared with the 50-digit reference on every model.  What the host does
not share with the device is out of this tier's sight and is the GPU tier's to catch: the kernels of tape_kernels.h,
the branch-free path for + - neg * of tape_interp.h, the generated bodies.

rho(e) = |V(e) - T(e)| / (2^-53 M(e)); M(e) >= |T(e)| is the entry without cancellation (mpref.py).  Worst rho per model
and block, host interpreter / oracle, over the ACCURACY_BATCH = 2 states of tape_models.measure (measured on x86-64
with glibc's libm):

  model    class (large, global, shared, bodies)   f          c_e        c_i        g          A_e        A_i        H
  small    (0, 0, 0, 0)                            0.23/0.23  0.65/0.65  0.90/0.90  1.71/1.71  3.68/3.68  1.22/1.22  0.90/0.96
  large    (1, 0, 0, 0)                            0.57/0.57  0.94/0.94  0.68/0.68  1.89/1.89  1.32/1.32  0.90/0.90  0.60/0.60
  global   (0, 1, 0, 0)                            0.05/0.05  0.44/0.44  0.01/0.01  0.19/0.19  0.22/0.20  0.10/0.06  0.01/0.01
  family   (0, 0, 11, 1)                           0.21/0.21  1.69/1.69  1.93/1.93  0.00/0.00  1.79/1.79  3.05/3.05  2.38/2.38
  mixed    (1, 1, 11, 1)                           0.32/0.46  1.37/1.37  1.93/1.93  0.80/0.94  2.27/2.27  3.05/3.75  2.83/2.31
  ride     (1, 0, 11, 1)                           0.66/0.66  1.37/1.37  1.93/1.93  0.78/0.78  2.24/2.24  3.05/3.05  1.74/1.86

("ride" is mixed_model without its global component: the one layout in which the generated launch has 256-thread
workgroups and the large task rides in it.  g of "family" is exact: its cost is a sum of squares of variables.)

ops_model, worst error in ulps (the spacing of doubles at M(e)) per op, at the regular points / at the extreme points
(large trigonometric arguments, saturating arguments, cbrt of general arguments, atan2 by quadrant and on the axes,
(-1.5)^3), of the host interpreter and of the oracle.  ABS, SIGN, MAX, MIN, ISNONNEG, ISPOS: 0 throughout.

             host interpreter                                oracle
  op         value      dl         dr         d2             value      dl         dr         d2
  ADD        0.50       0.00       0.00       -              0.50       0.00       0.00       -
  SUB        0.50       0.00       0.00       -              0.50       0.00       0.00       -
  NEG        0.50       0.00       -          -              0.50       0.00       -          -
  MUL        0.50       0.00       0.00       0.50           0.50       0.00       0.00       0.50
  DIV        0.49       0.50       1.51       2.51           0.49       0.50       1.03       2.51
  POW        0.49/0.44  1.15/0.58  1.57/0.74  1.73/0.61      0.49/0.44  1.15/0.58  1.57/0.74  1.47/0.61
  SQRT       0.50       1.23       -          2.61           0.50       1.23       -          3.04
  CBRT       0.56/1.59  1.63/2.44  -          4.37/4.98      0.56/1.59  1.63/2.44  -          4.40/4.94
  EXP        0.78/0.14  0.48/0.14  -          1.46/0.83      0.78/0.14  0.48/0.14  -          0.89/0.36
  LOG        0.99       0.49       -          1.51           0.99       0.49       -          1.39
  LOG10      1.26       1.54       -          2.64           1.26       1.54       -          3.13
  SIN        0.91/0.30  0.49/0.49  -          1.50/0.76      0.91/0.30  0.49/0.49  -          1.25/0.76
  COS        0.59/0.49  0.49/0.30  -          1.37/0.19      0.59/0.49  0.49/0.30  -          1.13/0.19
  TAN        0.78/0.58  2.81/0.58  -          4.19/0.77      0.78/0.58  2.81/0.58  -          3.14/1.46
  ASIN       0.74       1.07       -          4.89           0.74       1.07       -          3.89
  ACOS       0.57       0.92       -          2.84           0.57       0.92       -          1.81
  ATAN       0.70       1.73       -          2.51           0.70       1.73       -          2.51
  ATAN2      0.49/0.44  1.45/0.69  1.43/0.80  2.76/1.49      0.49/0.44  1.45/0.69  1.43/0.80  2.10/1.25
  SINH       0.97       0.78       -          1.31           0.97       0.78       -          1.30
  COSH       0.87       0.96       -          1.17           0.87       0.96       -          1.50
  TANH       1.54/0.04  2.40/0.11  -          4.08/1.21      1.54/0.04  2.40/0.11  -          6.08/0.21
  ERF        0.71/0.00  4.76/0.23  -          4.20/0.48      0.71/0.00  4.76/0.23  -          4.20/0.48
  HYPOT      0.52       1.15       1.15       3.32           0.52       1.15       1.15       4.32

(dl of erf: the rounding of -l^2 goes through exp, l^2 times half an ulp.)
"""
import math

import pytest

from tests.support import mpref, tape_models as tm

# Two double implementations against the reference.  Every entry is a sum of products of the ops' partials; the
# products' rounding errors are a few units of 2^-53 each, relative to the term — M(e) is the sum of the terms'
# magnitudes — and the error of an op's ARGUMENT reaches the entry through the op's condition number, which the models
# keep moderate (arguments inside the domains with margin).  64 units leave room for that at the depth of these chains;
# a dropped partial, a wrong edge or a wrong sign convention is an error of the size of a term: rho of 1e8 and more.
RHO_CPU = 64.0
ULP_REGULAR = 8.0  # the host interpreter and the oracle at the regular points of ops_model
T_RANGE = (1e-4, 1e3)


@pytest.fixture(scope="module", params=list(tm.CASES))
def case(request, slpx, orc, hostcheck):
    return request.param, tm.measure(request.param)


@pytest.fixture(scope="module")
def ops(slpx, orc, hostcheck):
    return tm.measure("ops")


def test_model_is_in_its_task_class(case):
    name, r = case
    assert r["class"] == tm.CASES[name][1], (name, r["class"])
    assert r["scaling_is_one"], "the oracle scales this model: the comparison assumes factors of 1"


def test_chain_entries_are_finite_and_of_moderate_size(case):
    name, r = case
    n, me, mi = r["dims"]
    for who in ("host", "oracle"):
        for res in r[who]:
            for block in ("g", "A_e", "A_i", "H"):
                assert not res[block]["nonfinite"], (name, who, block, res[block]["nonfinite"][:4])
                assert T_RANGE[0] <= res[block]["tmin"] and res[block]["tmax"] <= T_RANGE[1], (name, who, block, res[block])
            # no entry left out: every value, every column of g, every stored entry of the matrices was compared
            assert (res["f"]["count"], res["c_e"]["count"], res["c_i"]["count"], res["g"]["count"]) == (1, me, mi, n)
    for b, ev in enumerate(r["evs"]):
        for block in ("A_e", "A_i", "H"):
            assert r["host"][b][block]["count"] >= len(ev.T[block]) > 0, (name, block)


def test_host_interpreter_and_oracle_against_the_reference(case):
    name, r = case
    print(name, "class", r["class"])
    for block in mpref.BLOCKS:
        print("  %-4s rho_host %6.2f  rho_oracle %6.2f" % (block, r["rho_host"][block], r["rho_oracle"][block]))
    for block in mpref.BLOCKS:
        assert r["rho_host"][block] <= RHO_CPU, (name, block, r["rho_host"][block])
        assert r["rho_oracle"][block] <= RHO_CPU, (name, block, r["rho_oracle"][block])


def test_ops_model_is_one_small_interpreted_task(ops):
    assert ops["class"] == (0, 0, 0, 0) and ops["scaling_is_one"]
    assert len(ops["evs"]) == tm.OPS_BATCH


def test_ops_model_covers_every_op_and_flag(ops):
    rows = ops["rows"]
    for op in tm.OPS:
        kinds = {k for b in range(tm.OPS_BATCH) for o, k in rows.kind[b].items() if o == op}
        assert "regular" in kinds
        quantities = {q for (o, q, k) in ops["host"] if o == op}
        want = {"value", "dl"} | ({"dr"} if op in tm.BINARY else set())
        if op not in ("ADD", "SUB", "NEG", "SIGN", "ISNONNEG", "ISPOS"):
            want |= {"d2"}
        assert want <= quantities, (op, quantities)
    # rows with a constant child: phi(u, c) has no entry in v's column and phi(c, v) none in u's
    ev = ops["evs"][0]
    for r, (op, lv, rv) in enumerate(rows.rows_eq):
        cols = {c for (rr, c) in ev.T["A_e"] if rr == r}
        assert cols == {v for v in (lv, rv) if v is not None} or op in ("SIGN", "ISNONNEG", "ISPOS"), (r, op, cols)


def test_ops_at_regular_and_extreme_points(ops):
    for who in ("host", "oracle"):
        for op in tm.OPS:
            line = []
            for q in ("value", "dl", "dr", "d2"):
                for kind in ("regular", "extreme"):
                    if (op, q, kind) in ops[who]:
                        line.append("%s %s %.2f" % (q, kind, ops[who][(op, q, kind)]))
            print("%-6s %-8s %s" % (who, op, "  ".join(line)))
    for who in ("host", "oracle"):
        for (op, q, kind), ulps in ops[who].items():
            if kind == "regular":
                assert ulps <= ULP_REGULAR, (who, op, q, ulps)
            else:
                assert math.isfinite(ulps), (who, op, q)


def test_ops_at_edge_points(ops):
    """Where the reference has no finite number (or the point is an edge point) the host interpreter and the oracle
    show the same NaN / inf pattern, and the piecewise ops give the reference's value and partials exactly, by the
    conventions of tape_ops.h (abs'(0) = 0, sign' = 0, the left argument of max / min on a tie)."""
    compared = exact = 0
    for b in range(tm.OPS_BATCH):
        ph, po = ops["host_pattern"][b], ops["oracle_pattern"][b]
        for key, (vh, op, t) in ph.items():
            if key in po:
                assert tm.same_pattern(vh, po[key][0]), (b, key, op, vh, po[key][0])
                compared += 1
            if op in tm.PIECEWISE:
                assert t is not None and vh == t, (b, key, op, vh, t)
                if key in po:
                    assert po[key][0] == t, (b, key, op, po[key][0], t)
                exact += 1
    nonfinite = sum(1 for b in range(tm.OPS_BATCH) for v, _, _ in ops["host_pattern"][b].values() if not math.isfinite(v))
    print("edge entries compared", compared, "exact", exact, "not finite", nonfinite)
    assert compared > 100 and exact > 50 and nonfinite > 5
