"""GPU tier of the tape-sweep tests: System.sweep — tape_sweep_lds_kernel<64> and <256>, tape_sweep_global_kernel, the
generated bodies and the interpreted tasks that ride in their launch — against the mpmath reference
(tests/support/mpref.py) on the models of tests/support/tape_models.py, each proven to be in its task class on the CPU
(tests/test_tape_sweep_cpu.py, whose docstring holds the measured rho_host, rho_oracle and per-op ulps; they are
recomputed here by the same code, tape_models.measure, so the bounds follow the machine's libm).

  a. accuracy: per block rho_gpu <= 8 max(rho_host, rho_oracle, 2) on the chain and mixed models — the device's math
     functions are good to about 2 ulp where glibc is below 1, and -ffp-contract=on rounds in another order; a dropped
     partial, a stale LDS value or a wrong edge is rho of 1e8 and more.  ops_model: per op and quantity, in ulps,
     4 + 2 x the host interpreter's worst error at the same points; edge points by NaN / inf pattern and, for the
     piecewise ops, exactly.  By default and with SLPX_TAPE_JIT=0.
  b. the values-only sweep rewrites f, c_e, c_i with the full sweep's bits and leaves the derivatives alone
  c. an instance of a batch is the batch-1 run of its state, bit for bit, wherever it sits in the batch
  d. per-instance parameter pools in the large and the global class (test_parameters_gpu.py reaches the small one)
  e. generated bodies against the interpreter, bit for bit, with ops outside the basic set in the bodies
"""
import numpy as np
import pytest

from tests.support import model, mpref, parity, tape_models as tm

pytestmark = pytest.mark.gpu

MODES = [pytest.param({}, id="default"), pytest.param({"SLPX_TAPE_JIT": "0"}, id="interpreted")]


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _gpu_model(slpx, make):
    slpx.lib().slpx_graph_reset()
    return make(model.Model(model.ProductBackend("gpu")))


def _system(slpx, t, batch):
    return slpx.System(t.p.p, batch=batch)


def _sweep(sy, x, s, y, z, full=True):
    sy.set_state(x=x, s=s, y=y, z=z)
    sy.sweep(full=full)
    return sy.get("V").copy()


def _assert_class(sy, name):
    large, glob, shared, _ = tm.CASES[name][1]
    assert (sy.info["tape_global_tasks"], sy.info["tape_shared_tasks"]) == (glob, shared), (name, sy.info)


# ---- a. accuracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", MODES)
@pytest.mark.parametrize("name", list(tm.CASES))
def test_chain_and_mixed_models_against_the_reference(fresh, slpx, hostcheck, monkeypatch, name, env):
    r = tm.measure(name)
    assert r["class"] == tm.CASES[name][1]
    _setenv(monkeypatch, env)
    t = _gpu_model(slpx, tm.CASES[name][0])
    x, s, y, z = r["state"]
    sy = _system(slpx, t, len(x))
    _assert_class(sy, name)
    V = _sweep(sy, x, s, y, z)
    res = [mpref.compare(r["evs"][b], parity.unpack_sweep(sy, V[b])) for b in range(len(x))]
    rho = mpref.worst(res)
    print(name, dict(env), "rho_gpu", {b: round(v, 2) for b, v in rho.items()})
    for b in range(len(x)):
        for block in mpref.BLOCKS:
            assert res[b][block]["count"] == r["host"][b][block]["count"] and not res[b][block]["nonfinite"], (name, block)
    for block in mpref.BLOCKS:
        bound = 8.0 * max(r["rho_host"][block], r["rho_oracle"][block], 2.0)
        assert rho[block] <= bound, (name, block, rho[block], bound)
    sy.close()
    t.close()


@pytest.mark.parametrize("env", MODES)
def test_every_op_against_the_reference(fresh, slpx, hostcheck, monkeypatch, env):
    r = tm.measure("ops")
    _setenv(monkeypatch, env)
    t = _gpu_model(slpx, tm.ops_model)
    x, s, y, z = r["state"]
    sy = _system(slpx, t, tm.OPS_BATCH)
    V = _sweep(sy, x, s, y, z)
    worst, compared = {}, 0
    for b in range(tm.OPS_BATCH):
        measured, pattern = tm.ops_compare(t, b, r["evs"][b], parity.unpack_sweep(sy, V[b]))
        for k, v in measured.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # edge points: the host interpreter's NaN / inf pattern; the piecewise ops exactly
        host = r["host_pattern"][b]
        assert set(pattern) == set(host), (b, sorted(set(pattern) ^ set(host))[:4])
        for key, (v, op, _) in pattern.items():
            assert tm.same_pattern(v, host[key][0]), (b, key, op, v, host[key][0])
            if op in tm.PIECEWISE:
                assert v == host[key][0], (b, key, op, v, host[key][0])
            compared += 1
    assert set(worst) == set(r["host"]) and compared > 100
    for op in tm.OPS:
        print("%-8s" % op, "  ".join("%s %s %.2f (host %.2f)" % (q, k[:3], worst[(op, q, k)], r["host"][(op, q, k)])
                                     for q in ("value", "dl", "dr", "d2") for k in ("regular", "extreme") if (op, q, k) in worst))
    for key, ulps in worst.items():
        assert ulps <= 4.0 + 2.0 * r["host"][key], (key, ulps, r["host"][key])
    sy.close()
    t.close()


# ---- b. the values-only sweep --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["large", "global", "mixed", "ride"])
def test_values_only_sweep(fresh, slpx, name):
    t = _gpu_model(slpx, tm.CASES[name][0])
    xa, s, y, z = tm.state(t, 2, seed=11)
    xb = tm.state(t, 2, seed=12)[0]
    sy = _system(slpx, t, 2)
    _assert_class(sy, name)
    head = 1 + sy.info["m_e"] + sy.info["m_i"]
    Va = _sweep(sy, xa, s, y, z)
    Vv = _sweep(sy, xb, s, y, z, full=False)
    Vb = _sweep(sy, xb, s, y, z)
    assert np.array_equal(Vv[:, :head], Vb[:, :head])
    assert np.array_equal(Vv[:, head:], Va[:, head:]), "the values-only sweep touched the derivatives"
    assert not np.array_equal(Va[:, :head], Vb[:, :head]) and not np.array_equal(Va[:, head:], Vb[:, head:])
    assert np.all(np.isfinite(Vb))
    sy.close()
    t.close()


# ---- c. batch independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["large", "global", "mixed", "ride"])
def test_an_instance_is_its_batch_of_one(fresh, slpx, name):
    """blockIdx.y, v_stride and the global kernel's scratch_stride: B = 3 different (x, y, z)."""
    t = _gpu_model(slpx, tm.CASES[name][0])
    B = 3
    x, s, y, z = tm.state(t, B, seed=21)
    one = _system(slpx, t, 1)
    alone = [_sweep(one, x[b], s[b], y[b], z[b])[0] for b in range(B)]
    one.close()
    assert not np.array_equal(alone[0], alone[1]) and not np.array_equal(alone[1], alone[2])
    sy = _system(slpx, t, B)
    _assert_class(sy, name)
    V = _sweep(sy, x, s, y, z)
    for b in range(B):
        assert np.array_equal(V[b], alone[b]), (name, b, np.flatnonzero(V[b] != alone[b])[:8])
    perm = [2, 0, 1]
    Vp = _sweep(sy, x[perm], s[perm], y[perm], z[perm])
    for b in range(B):
        assert np.array_equal(Vp[b], alone[perm[b]]), (name, "permuted", b)
    sy.close()
    t.close()


# ---- d. per-instance parameter pools -------------------------------------------------------------------------------
PARAMETER_ROWS = np.array([tm.CHAIN_CONSTANTS, (0.55, 0.45, 0.2, 0.35), (0.7, 0.3, 0.3, 0.25)])


@pytest.mark.parametrize("name", ["large", "global"])
def test_parameter_pool_per_instance(fresh, slpx, hostcheck, name):
    """test_parameters_gpu.py::test_sweep_with_a_pool_per_instance at the two classes it does not reach: every instance
    has the bits of the model compiled with its row folded in."""
    n, L, stages = tm.CHAIN_SIZES[name]
    B = len(PARAMETER_ROWS)
    build = lambda row: _gpu_model(slpx, lambda m: tm.chain_model(m, n, L, stages, parameters=row))
    folded = []
    state = None
    for b in range(B):
        tf = build(PARAMETER_ROWS[b])
        state = tm.state(tf, B, seed=31) if state is None else state
        x, s, y, z = state
        sf = _system(slpx, tf, 1)
        folded.append(_sweep(sf, x[b], s[b], y[b], z[b])[0])
        sf.close()
        tf.close()
    assert not np.array_equal(folded[0], folded[1]) and not np.array_equal(folded[1], folded[2])
    t = build(PARAMETER_ROWS[0])
    hc = hostcheck.HostCheck(t.p.p)
    assert tm.task_class(hc) == tm.CASES[name][1], (name, tm.task_class(hc))  # with parameters too
    hc.close()
    x, s, y, z = state
    sy = _system(slpx, t, B)
    sy.set_parameters(PARAMETER_ROWS, per_instance=True)
    V = _sweep(sy, x, s, y, z)
    for b in range(B):
        assert np.array_equal(V[b], folded[b]), (name, b, np.flatnonzero(V[b] != folded[b])[:8])
    # the values-only program reads its own per-instance pool
    head = 1 + sy.info["m_e"] + sy.info["m_i"]
    _sweep(sy, x[::-1].copy(), s, y, z)
    Vv = _sweep(sy, x, s, y, z, full=False)
    for b in range(B):
        assert np.array_equal(Vv[b][:head], folded[b][:head]), (name, b)
    sy.close()
    t.close()


# ---- e. generated against interpreted ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["family", "mixed", "ride"])
def test_generated_bodies_match_the_interpreter_bit_for_bit(fresh, slpx, monkeypatch, name):
    """test_gpu_parity.py::test_generated_tape_kernel_matches_the_interpreter_bit_for_bit beyond cart-pole: the bodies of
    these families hold pow, atan2, exp, hypot, log, tanh, erf and cbrt (op_forward<true>)."""
    got = {}
    for jit in ("1", "0"):
        monkeypatch.setenv("SLPX_TAPE_JIT", jit)
        t = _gpu_model(slpx, tm.CASES[name][0])
        x, s, y, z = tm.state(t, 2, seed=41)
        sy = _system(slpx, t, 2)
        _assert_class(sy, name)
        got[jit] = _sweep(sy, x, s, y, z)
        sy.close()
        t.close()
    assert np.all(np.isfinite(got["1"])) and np.any(got["1"] != 0.0)
    assert np.array_equal(got["1"], got["0"]), np.flatnonzero(got["1"] != got["0"])[:8]
