"""The configuration of a system on the CPU: the switches as the environment gives them (csrc/switches.hpp), the
options and the route to a plan, and the launch modes of DeviceNlp (csrc/system_choice.hpp) from capacities handed in.
tests/support/choicecheck.cpp hands the structs over; everything is checked here, against values written out from a
reading of the rules as they stood in newton.cpp and kernels.hip before they moved."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.support import choicecheck as cc

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for name in list(os.environ):
        if name.startswith("SLPX_") and name not in ("SLPX_LIB", "SLPX_CACHE_DIR", "SLPX_JIT_CACHE", "SLPX_PREBUILT_DIR"):
            monkeypatch.delenv(name)


# ---- switches ----

DEFAULTS = {"fuse_launches": 1, "fuse_kkt": 1, "fuse_backsub": 1, "ldlt_mf": 1, "ldlt_il": 1, "chain_tape": 1, "ipm_resident": 1,
            "ipm_lookahead": 1, "ipm_pipeline": 1, "twin": 1, "ipm_ride": 1, "mf_solve": 1, "fuse_kkt_store": 0, "il_min_batch": 64,
            "dense": None, "task_entries": None, "single_launch": None, "mf_threads": None, "relax_zeros": None, "sn_min_width": None,
            "mfma_min_entries": None}
ENV_OF = {"fuse_launches": "SLPX_FUSE_LAUNCHES", "fuse_kkt": "SLPX_FUSE_KKT", "fuse_backsub": "SLPX_FUSE_BACKSUB", "ldlt_mf": "SLPX_LDLT_MF",
          "ldlt_il": "SLPX_LDLT_IL", "chain_tape": "SLPX_CHAIN_TAPE", "ipm_resident": "SLPX_IPM_RESIDENT",
          "ipm_lookahead": "SLPX_IPM_LOOKAHEAD", "ipm_pipeline": "SLPX_IPM_PIPELINE", "twin": "SLPX_TWIN", "ipm_ride": "SLPX_IPM_RIDE",
          "mf_solve": "SLPX_MF_SOLVE", "fuse_kkt_store": "SLPX_FUSE_KKT_STORE", "il_min_batch": "SLPX_IL_MIN_BATCH", "dense": "SLPX_DENSE",
          "task_entries": "SLPX_TASK_ENTRIES", "single_launch": "SLPX_SINGLE_LAUNCH", "mf_threads": "SLPX_MF_THREADS",
          "relax_zeros": "SLPX_RELAX_ZEROS", "sn_min_width": "SLPX_SN_MIN_WIDTH", "mfma_min_entries": "SLPX_MFMA_MIN_ENTRIES"}
FLAGS = ["fuse_launches", "fuse_kkt", "fuse_backsub", "ldlt_mf", "ldlt_il", "chain_tape", "ipm_resident", "ipm_lookahead", "ipm_pipeline",
         "twin", "ipm_ride", "mf_solve", "fuse_kkt_store", "single_launch"]
NUMBERS = ["il_min_batch", "task_entries", "mf_threads", "relax_zeros", "sn_min_width", "mfma_min_entries"]


def test_unset_switches_are_the_defaults():
    assert set(ENV_OF) == set(cc.SWITCHES) == set(DEFAULTS)
    assert cc.switches() == DEFAULTS


@pytest.mark.parametrize("member", FLAGS)
def test_a_flag_is_off_only_from_a_leading_zero(member, monkeypatch):
    # `env[0] != '0'`: "0", "0x", "00" are off; "1", "", "no", "2" are on
    for text, value in (("0", 0), ("1", 1), ("00", 0), ("0x", 0), ("", 1), ("no", 1), ("2", 1)):
        monkeypatch.setenv(ENV_OF[member], text)
        assert cc.switches() == dict(DEFAULTS, **{member: value}), text


@pytest.mark.parametrize("member", NUMBERS)
def test_a_number_is_atoi(member, monkeypatch):
    for text, value in (("0", 0), ("1", 1), ("768", 768), ("16", 16), ("12abc", 12), ("abc", 0), ("", 0)):
        monkeypatch.setenv(ENV_OF[member], text)
        assert cc.switches() == dict(DEFAULTS, **{member: value}), text


def test_dense_has_three_states(monkeypatch):
    # unset: the reference's density rule; "0...": always sparse; "1...": dense without pivoting; anything else was
    # compared with '0' and with '1' and matched neither: as unset
    for text, value in (("0", 0), ("1", 1), ("01", 0), ("10", 1), ("2", None), ("", None), ("yes", None)):
        monkeypatch.setenv("SLPX_DENSE", text)
        assert cc.switches() == dict(DEFAULTS, dense=value), text


def test_task_entries_unset_and_single_launch_both_ways(monkeypatch):
    assert cc.switches()["task_entries"] is None and cc.switches()["single_launch"] is None
    monkeypatch.setenv("SLPX_TASK_ENTRIES", "2048")  # (the default value, set: still "set")
    assert cc.switches()["task_entries"] == 2048
    monkeypatch.setenv("SLPX_SINGLE_LAUNCH", "1")
    assert cc.switches()["single_launch"] == 1
    monkeypatch.setenv("SLPX_SINGLE_LAUNCH", "0")
    assert cc.switches()["single_launch"] == 0


def test_interleaved_threshold(monkeypatch):
    assert [cc.interleaved_for(b) for b in (1, 63, 64, 512)] == [False, False, True, True]
    monkeypatch.setenv("SLPX_IL_MIN_BATCH", "16")
    assert [cc.interleaved_for(b) for b in (15, 16, 64)] == [False, True, True]
    monkeypatch.setenv("SLPX_LDLT_IL", "0")
    assert [cc.interleaved_for(b) for b in (16, 64, 512)] == [False, False, False]


# ---- plan options ----

BATCHES = (1, 2, 15, 16, 63, 64, 191, 192, 512)
PLAIN = {"task_entries": 2048, "supernodal": 1, "multifrontal": 0, "min_supernode_width": 4, "relax_zeros": 0, "balance_supernode_cuts": 0,
         "chain_from_deepest_child": 0, "chain_from_deepest_min_round": 1, "single_problem_task_rules": 0, "mfma_min_entries": 400}
FRONTS = {"multifrontal": 1, "min_supernode_width": 2, "relax_zeros": 8, "balance_supernode_cuts": 1, "chain_from_deepest_child": 1,
          "chain_from_deepest_min_round": 0}
# the task size of a compiled model in a batch < 16: 256 round(2048 sqrt(dim / 9000) / 256) within [1024, 2048] below 9000
# rows (dim 1000: 683 -> 768 -> 1024), the default 2048 from 9000 on
SMALL_BATCH_ENTRIES = {1000: 1024, 9000: 2048}


def expected_options(batch, dim, row):
    """The options of a compiled model, written out per switch row."""
    e = dict(PLAIN)
    il_min = 16 if row == "SLPX_IL_MIN_BATCH=16" else 64
    il = row != "SLPX_LDLT_IL=0" and batch >= il_min
    if batch < 16:
        e["task_entries"] = SMALL_BATCH_ENTRIES[dim]
    elif not il:
        e["task_entries"] = 1024
    else:
        e["task_entries"] = 512 if batch < 192 else 384
    if il:
        e["supernodal"] = 0
    if batch == 1:
        e["single_problem_task_rules"] = 1
        if row != "SLPX_LDLT_MF=0":
            e.update(FRONTS)
    if row == "SLPX_TASK_ENTRIES=768":
        e["task_entries"] = 768
        e["single_problem_task_rules"] = 0
    if row == "SLPX_RELAX_ZEROS=0":
        e["relax_zeros"] = 0
    return e


OPTION_ROWS = ("", "SLPX_LDLT_MF=0", "SLPX_LDLT_IL=0", "SLPX_IL_MIN_BATCH=16", "SLPX_TASK_ENTRIES=768", "SLPX_RELAX_ZEROS=0")


def test_expected_options_spelled_out():
    """What expected_options says at the corners, as literals."""
    assert expected_options(1, 1000, "") == dict(PLAIN, task_entries=1024, single_problem_task_rules=1, **FRONTS)
    assert expected_options(1, 9000, "SLPX_LDLT_MF=0") == dict(PLAIN, task_entries=2048, single_problem_task_rules=1)
    assert expected_options(15, 1000, "") == dict(PLAIN, task_entries=1024)
    assert expected_options(16, 9000, "") == dict(PLAIN, task_entries=1024)
    assert expected_options(63, 1000, "SLPX_IL_MIN_BATCH=16") == dict(PLAIN, task_entries=512, supernodal=0)
    assert expected_options(64, 1000, "") == expected_options(191, 9000, "") == dict(PLAIN, task_entries=512, supernodal=0)
    assert expected_options(192, 1000, "") == expected_options(512, 9000, "") == dict(PLAIN, task_entries=384, supernodal=0)
    assert expected_options(512, 1000, "SLPX_LDLT_IL=0") == dict(PLAIN, task_entries=1024)
    assert expected_options(1, 1000, "SLPX_TASK_ENTRIES=768") == dict(PLAIN, task_entries=768, **FRONTS)
    assert expected_options(512, 1000, "SLPX_TASK_ENTRIES=768") == dict(PLAIN, task_entries=768, supernodal=0)
    assert expected_options(1, 1000, "SLPX_RELAX_ZEROS=0") == dict(PLAIN, task_entries=1024, single_problem_task_rules=1, **dict(FRONTS, relax_zeros=0))


@pytest.mark.parametrize("row", OPTION_ROWS)
def test_options_of_a_compiled_model(row, monkeypatch):
    if row:
        monkeypatch.setenv(*row.split("="))
    for batch in BATCHES:
        for dim in (1000, 9000):
            assert cc.options(batch, dim)[0] == expected_options(batch, dim, row), (batch, dim)


@pytest.mark.parametrize("row", OPTION_ROWS)
def test_options_of_a_bare_linear_system_are_the_three_batch_rules(row, monkeypatch):
    if row:
        monkeypatch.setenv(*row.split("="))
    il_min = 16 if row == "SLPX_IL_MIN_BATCH=16" else 64
    for batch in BATCHES:
        il = row != "SLPX_LDLT_IL=0" and batch >= il_min
        entries = 2048 if batch < 16 else 1024 if not il else 512 if batch < 192 else 384
        for dim in (1000, 9000):
            assert cc.options(batch, dim, compiled_model=False)[0] == dict(PLAIN, task_entries=entries, supernodal=0 if il else 1), (batch, dim)


def test_a_task_size_of_the_callers_is_kept_below_16_problems():
    assert cc.options(1, 1000, base_task_entries=512)[0]["task_entries"] == 512
    assert cc.options(16, 1000, base_task_entries=512)[0]["task_entries"] == 512
    assert cc.options(64, 1000, base_task_entries=1536)[0]["task_entries"] == 512  # (>= 1024: the interleaved kernels' size)


def test_pair_list_options_drop_the_fronts_tuning():
    chosen, pair = cc.options(1, 1000)
    assert chosen["multifrontal"] == 1
    assert pair == dict(PLAIN, task_entries=1024)


# ---- the plan ----

def test_dense_factor_bound():
    assert cc.dense_bound_error(1024, 2048) is None  # 32 GB
    assert cc.dense_bound_error(2048, 2048) is None  # 64 GB: the bound itself
    msg = cc.dense_bound_error(4096, 2048)
    assert msg is not None and "4096 systems of order 2048" in msg and "128 GB" in msg and "SLPX_DENSE=0" in msg
    assert cc.dense_bound_error(1, 8192) is None and cc.dense_bound_error(0, 8192) is None


@pytest.fixture(scope="module")
def dense_model():
    from tests.support import dense_models, hostcheck, model

    p = dense_models.build(model.Model(model.ProductBackend("hostcheck")), 4, 0)
    hc = hostcheck.HostCheck(p.p)
    yield hc
    hc.close()


def test_plan_route_on_a_small_dense_model(dense_model, monkeypatch):
    hc = dense_model
    assert cc.plan(hc) == {"dense": True, "dense_pivoted": True, "mf": False, "mf_asked": True}
    assert cc.plan(hc, batch=64)["dense_pivoted"] is True
    monkeypatch.setenv("SLPX_DENSE", "1")
    assert cc.plan(hc) == {"dense": True, "dense_pivoted": False, "mf": False, "mf_asked": True}
    assert cc.plan(hc, perm=np.arange(4))["dense"] is True  # (SLPX_DENSE=1 does not ask about a permutation)
    monkeypatch.setenv("SLPX_DENSE", "0")
    assert cc.plan(hc)["dense"] is False
    monkeypatch.delenv("SLPX_DENSE")
    sparse = cc.plan(hc, perm=np.arange(4))
    assert sparse["dense"] is False and sparse["dense_pivoted"] is False


# ---- launch modes ----

# cart-pole N=1000's shape on a device of 256 CUs: 137 tasks, two separable sums
SPARSE = dict(batch=1, tasks=137, factor_lds_bytes=60000, mf=1, one_reader=1, n_sums=2, cus=256, kkt_ok=1, backsub_ok=1, mf_lds=70000,
              ask_twin=1, ask_ride=1)
FITS_1024 = dict(step_1024=256, step_512=512, solve_1024=256, solve_512=512, twin_1024=256, twin_512=512, riding=512)
FITS_512 = dict(step_1024=0, step_512=512, solve_1024=0, solve_512=512, twin_1024=0, twin_512=512, riding=512)
# one problem on the multifrontal step, chained, two attempts a launch (of 512 threads: 2 x 137 + 2 > 256) with the error
# launch riding (2 x 137 + 64 + 2 = 340 <= 512)
STEP = dict(dense=0, dense_pivoted=0, il=0, single_launch=1, fuse_launches=1, fuse_kkt=1, fuse_backsub=1, fuse_kkt_store=0, fuse_solve=1,
            slot_handoff=1, xg_by_data=1, mf=1, mf_solve=1, mf_mfma=0, mf_threads=1024, twin_threads=512, chain_mode=1, chain_on=1, twin=1,
            ride=1)
# ... and the same system on the pair lists: nothing of the step kernel, twin asked and refused, ride never asked
PAIRS = dict(STEP, fuse_solve=0, mf=0, mf_solve=0, twin_threads=1024, chain_on=0, twin=-1, ride=-1)
NOTHING = dict(dense=0, dense_pivoted=0, il=0, single_launch=0, fuse_launches=0, fuse_kkt=0, fuse_backsub=0, fuse_kkt_store=0, fuse_solve=0,
               slot_handoff=0, xg_by_data=0, mf=0, mf_solve=0, mf_mfma=0, mf_threads=1024, twin_threads=1024, chain_mode=0, chain_on=0,
               twin=-1, ride=-1)
BATCH_FACTS = dict(SPARSE, mf=0)  # (a batch's plan has no fronts)
DENSE = dict(batch=1, dense=1, dense_pivoted=1, tasks=1, factor_lds_bytes=0, one_reader=1, n_sums=0, cus=256, ask_twin=1, ask_ride=1)

MODE_CASES = [
    # (name, environment, inputs, expected)
    ("everything fits at 1024 threads", {}, dict(SPARSE, tasks=80, **FITS_1024), dict(STEP, twin_threads=1024)),
    ("N=1000: the step at 1024, two attempts at 512", {}, dict(SPARSE, **FITS_1024), STEP),
    ("fits only at 512", {}, dict(SPARSE, **FITS_512), dict(STEP, mf_threads=512)),
    ("static LDS in front of the dynamic block", {}, dict(SPARSE, static_lds=64, **FITS_1024), dict(PAIRS, mf_threads=512)),
    ("images over 160 KB", {}, dict(SPARSE, **dict(FITS_1024, mf_lds=163841)), PAIRS),
    ("nothing fits", {}, dict(SPARSE), dict(PAIRS, mf_threads=512)),
    ("the packer declined", {}, dict(SPARSE, mf_declined=1, **FITS_1024), PAIRS),
    ("a failed KKT pack clears fuse_kkt only", {}, dict(SPARSE, **dict(FITS_1024, kkt_ok=0)), dict(PAIRS, fuse_kkt=0)),
    ("a failed back-substitution pack", {}, dict(SPARSE, **dict(FITS_1024, backsub_ok=0)), dict(PAIRS, fuse_backsub=0)),
    ("twin without ride", {}, dict(SPARSE, **dict(FITS_1024, riding=339)), dict(STEP, ride=0)),
    ("two attempts do not fit", {}, dict(SPARSE, **dict(FITS_1024, twin_512=275)), dict(STEP, twin=-1, ride=-1)),
    ("twin and ride not asked yet", {}, dict(SPARSE, **dict(FITS_1024, ask_twin=0, ask_ride=0)), dict(STEP, twin=0, twin_threads=1024, ride=-1)),
    ("fronts on the matrix cores: no twin", {}, dict(SPARSE, mf_n_mfma=3, **FITS_1024), dict(STEP, mf_mfma=1, twin=-1, twin_threads=1024, ride=-1)),
    ("the solve does not fit", {}, dict(SPARSE, **dict(FITS_1024, solve_1024=136)), dict(STEP, mf_solve=0)),
    ("too many workgroups to chain", {}, dict(SPARSE, **dict(FITS_1024, cus=202)), dict(STEP, chain_mode=0, chain_on=0)),
    ("several readers of an update slot", {}, dict(SPARSE, **dict(FITS_1024, one_reader=0)), dict(STEP, slot_handoff=0)),
    ("a task with less than 64 doubles of LDS", {}, dict(SPARSE, **dict(FITS_1024, factor_lds_bytes=511)),
     dict(PAIRS, fuse_launches=0, fuse_kkt=0, fuse_backsub=0)),
    ("SLPX_FUSE_LAUNCHES=0", {"SLPX_FUSE_LAUNCHES": "0"}, dict(SPARSE, **FITS_1024), dict(PAIRS, fuse_launches=0, fuse_kkt=0, fuse_backsub=0)),
    ("SLPX_FUSE_KKT=0", {"SLPX_FUSE_KKT": "0"}, dict(SPARSE, **FITS_1024), dict(PAIRS, fuse_kkt=0)),
    ("SLPX_FUSE_BACKSUB=0", {"SLPX_FUSE_BACKSUB": "0"}, dict(SPARSE, **FITS_1024), dict(PAIRS, fuse_backsub=0)),
    ("SLPX_FUSE_KKT_STORE=1", {"SLPX_FUSE_KKT_STORE": "1"}, dict(SPARSE, **FITS_1024), dict(STEP, fuse_kkt_store=1)),
    ("SLPX_LDLT_MF=0 (the plan then has no fronts)", {"SLPX_LDLT_MF": "0"}, dict(SPARSE, mf=0, **FITS_1024), dict(PAIRS, chain_mode=0)),
    ("SLPX_LDLT_MF=0 on a plan with fronts", {"SLPX_LDLT_MF": "0"}, dict(SPARSE, **FITS_1024), PAIRS),
    ("SLPX_CHAIN_TAPE=0", {"SLPX_CHAIN_TAPE": "0"}, dict(SPARSE, **FITS_1024), dict(STEP, chain_mode=0, chain_on=0)),
    ("SLPX_IPM_RIDE=0", {"SLPX_IPM_RIDE": "0"}, dict(SPARSE, **FITS_1024), dict(STEP, ride=0)),
    ("SLPX_TWIN=0", {"SLPX_TWIN": "0"}, dict(SPARSE, **FITS_1024), dict(STEP, twin=-1, twin_threads=1024, ride=-1)),
    ("SLPX_MF_SOLVE=0", {"SLPX_MF_SOLVE": "0"}, dict(SPARSE, **FITS_1024), dict(STEP, mf_solve=0)),
    ("SLPX_MF_THREADS=512", {"SLPX_MF_THREADS": "512"}, dict(SPARSE, **FITS_1024), dict(STEP, mf_threads=512)),
    ("SLPX_MF_THREADS=1024", {"SLPX_MF_THREADS": "1024"}, dict(SPARSE, **FITS_1024), STEP),
    ("SLPX_SINGLE_LAUNCH=0", {"SLPX_SINGLE_LAUNCH": "0"}, dict(SPARSE, **FITS_1024), dict(NOTHING, chain_mode=1)),
    ("SLPX_SINGLE_LAUNCH=1", {"SLPX_SINGLE_LAUNCH": "1"}, dict(SPARSE, **FITS_1024), STEP),
    ("the interior-point switches touch no mode", {"SLPX_IPM_RESIDENT": "0", "SLPX_IPM_LOOKAHEAD": "0", "SLPX_IPM_PIPELINE": "0"},
     dict(SPARSE, **FITS_1024), STEP),
    # batches: no launch fusion, so nothing of the step kernel
    ("batch 8, 800 workgroups", {}, dict(BATCH_FACTS, batch=8, tasks=100, **FITS_1024), dict(NOTHING, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("batch 8, 1096 workgroups", {}, dict(BATCH_FACTS, batch=8, **FITS_1024), NOTHING),
    ("batch 8, a plan with fronts", {}, dict(SPARSE, batch=8, tasks=100, **FITS_1024), dict(NOTHING, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("batch 8, SLPX_SINGLE_LAUNCH=1", {"SLPX_SINGLE_LAUNCH": "1"}, dict(BATCH_FACTS, batch=8, **FITS_1024),
     dict(NOTHING, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("batch 64: interleaved", {}, dict(BATCH_FACTS, batch=64, tasks=242, **FITS_1024), dict(NOTHING, il=1)),
    ("batch 64, SLPX_LDLT_IL=0", {"SLPX_LDLT_IL": "0"}, dict(BATCH_FACTS, batch=64, tasks=242, **FITS_1024), NOTHING),
    ("batch 8, SLPX_IL_MIN_BATCH=8", {"SLPX_IL_MIN_BATCH": "8"}, dict(BATCH_FACTS, batch=8, tasks=100, **FITS_1024), dict(NOTHING, il=1)),
    ("batch 64, SLPX_SINGLE_LAUNCH=0", {"SLPX_SINGLE_LAUNCH": "0"}, dict(BATCH_FACTS, batch=64, tasks=242, **FITS_1024), dict(NOTHING, il=1)),
    ("batch 64, SLPX_SINGLE_LAUNCH=1", {"SLPX_SINGLE_LAUNCH": "1"}, dict(BATCH_FACTS, batch=64, tasks=242, **FITS_1024),
     dict(NOTHING, il=1, single_launch=1, slot_handoff=1, xg_by_data=1)),
    # the dense branch: one task, no LDS plan, never interleaved
    ("dense, one problem", {}, DENSE, dict(NOTHING, dense=1, dense_pivoted=1, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("dense without pivoting", {}, dict(DENSE, dense_pivoted=0), dict(NOTHING, dense=1, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("dense, batch 8", {}, dict(DENSE, batch=8), dict(NOTHING, dense=1, dense_pivoted=1, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("dense, batch 64", {}, dict(DENSE, batch=64), dict(NOTHING, dense=1, dense_pivoted=1, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("dense, batch 64, SLPX_LDLT_IL=0", {"SLPX_LDLT_IL": "0"}, dict(DENSE, batch=64),
     dict(NOTHING, dense=1, dense_pivoted=1, single_launch=1, slot_handoff=1, xg_by_data=1)),
    ("dense, SLPX_SINGLE_LAUNCH=0", {"SLPX_SINGLE_LAUNCH": "0"}, DENSE, dict(NOTHING, dense=1, dense_pivoted=1)),
    ("dense, SLPX_FUSE_LAUNCHES=0", {"SLPX_FUSE_LAUNCHES": "0"}, DENSE,
     dict(NOTHING, dense=1, dense_pivoted=1, single_launch=1, slot_handoff=1, xg_by_data=1)),
]


def check_invariants(name, env, inputs, m):
    if m["mf"]:
        assert m["fuse_launches"] and m["fuse_kkt"] and m["fuse_backsub"] and m["single_launch"] and inputs["batch"] == 1, name
    if m["il"]:
        assert not m["dense"], name
        assert not m["single_launch"] or env.get("SLPX_SINGLE_LAUNCH") == "1", name  # (the switch overrules in both directions)
    if m["chain_on"]:
        assert m["mf"], name
    if m["twin"] > 0:
        assert m["mf"] and not m["mf_mfma"], name
    if m["ride"] > 0:
        assert m["twin"] > 0, name
    assert m["fuse_solve"] == m["mf"], name
    assert not m["dense_pivoted"] or m["dense"], name


@pytest.mark.parametrize("name,env,inputs,expected", MODE_CASES, ids=[c[0] for c in MODE_CASES])
def test_launch_modes(name, env, inputs, expected, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = cc.modes(**inputs)
    assert got == expected
    check_invariants(name, env, inputs, got)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "address,undefined"])
def test_launch_modes_by_the_stand_alone_program(sanitized, monkeypatch):
    """The same table through the program with its own main, plain and built with -fsanitize=address,undefined: every
    row as expected and nothing reported."""
    by_env = {}
    for name, env, inputs, expected in MODE_CASES:
        by_env.setdefault(tuple(sorted(env.items())), []).append((name, inputs, expected))
    for env, cases in by_env.items():
        with monkeypatch.context() as mp:
            for k, v in env:
                mp.setenv(k, v)
            got = cc.modes_by_program([inputs for _, inputs, _ in cases], sanitized=sanitized)
        for (name, _, expected), g in zip(cases, got):
            assert g == expected, name


# ---- the product's own options for batches, as plans ----

def _plan_row(env, *args):
    base = {k: v for k, v in os.environ.items() if not k.startswith("SLPX_HOSTCHECK_")}
    base["PYTHONPATH"] = str(ROOT)
    res = subprocess.run([sys.executable, "-m", "tests.support.plan_hash_cli", "cart_pole", "500", "--info", *args], cwd=ROOT,
                         env=dict(base, **env), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("batch,entries", [(64, 512), (512, 384)])
def test_a_batchs_plan_is_the_column_plan_the_hash_matrix_imitates(batch, entries):
    """profiles/plan_hash_matrix.py: cart_pole500/product/batch_<B> against cart_pole500/columns/task_entries_<K>."""
    product = _plan_row({}, "--product-batch", str(batch))
    imitation = _plan_row({"SLPX_HOSTCHECK_COLUMN_PLAN": str(entries)})
    assert product == imitation
    assert not product["mf"] and not product["dense"]
