"""The plans of the symbolic LDLT over the option sets the product and the tests reach, as hashes: what a change to
csrc/ldlt_*.cpp that must leave every plan the same to the byte is checked with, on the CPU.

    python profiles/plan_hash_matrix.py run > OUT.jsonl         # on each of the two commits
    python profiles/plan_hash_matrix.py compare A.jsonl B.jsonl   # -> the text of plan_hash_matrix.txt

One JSON line per case: its name, the six hashes of hostcheck.cpp: hc_plan_hash ([structure, full tape, values tape, KKT
plan, LDLT plan, multifrontal plan]), tasks, rounds, whether the fronts were built (`mf`), how many of them go to the
matrix cores (`mfma`), whether the plan is the dense one.  Every case runs in a process of its own
(tests.support.plan_hash_cli): the setup pool is made once per process, and the options are environment variables.
`compare` wants every row equal; one differing hash means the change is wrong, not that the matrix needs editing."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MF = {"SLPX_LDLT_MF": "1"}
RULES = {"SLPX_LDLT_MF": "1", "SLPX_HOSTCHECK_SINGLE_PROBLEM_RULES": "1"}


def cases():
    """(name, model, N, environment, further arguments of plan_hash_cli)"""
    out = []
    baseline = [("cart_pole", N) for N in (4, 37, 60, 300, 700, 1000, 5000)] + [("flywheel", 50)]
    for kind, N in baseline:
        out.append((f"{kind}{N}", kind, N, {}, []))
        out.append((f"{kind}{N}/mf", kind, N, MF, []))
    # one problem, every round in one launch (newton.cpp): N = 5000 is partitioned a second time with tasks twice the size
    for N in (1000, 5000):
        out.append((f"cart_pole{N}/mf/single_problem_rules", "cart_pole", N, RULES, ["--first-pass"]))
    # fronts on the matrix cores
    out.append(("gfold100/mf", "gfold", 100, MF, []))
    out.append(("gfold100/mf/mfma_min_128", "gfold", 100, dict(MF, SLPX_MFMA_MIN_ENTRIES="128"), []))
    # the batched plans: column levels, small tasks
    for N in (500, 1000):
        for entries in (1024, 512, 384):
            out.append((f"cart_pole{N}/columns/task_entries_{entries}", "cart_pole", N, {"SLPX_HOSTCHECK_COLUMN_PLAN": str(entries)}, []))
    # ... and what the product's own rules give a batch (choose_ldlt_options): 64 is the 512-entry column plan above, 512
    # the 384-entry one (tests/test_system_choice_cpu.py asserts both)
    for batch in (1, 16, 64, 512):
        out.append((f"cart_pole500/product/batch_{batch}", "cart_pole", 500, {}, ["--product-batch", str(batch)]))
    out.append(("cart_pole24/task_entries_64", "cart_pole", 24, {}, ["--task-entries", "64", "--small-lds", str(24 * 1024)]))
    for kind, N in (("cart_pole", 37), ("flywheel", 50)):
        for var, values in (("SLPX_SN_MIN_WIDTH", (2, 3)), ("SLPX_SN_DEEPEST", (0, 1, 2)), ("SLPX_RELAX_ZEROS", (0, 4, 32)),
                            ("SLPX_SUPERNODAL", (0,))):
            for v in values:
                out.append((f"{kind}{N}/{var}={v}", kind, N, {var: str(v)}, []))
                if var != "SLPX_SUPERNODAL":
                    out.append((f"{kind}{N}/mf/{var}={v}", kind, N, dict(MF, **{var: str(v)}), []))
    # fronts asked for and not built: supernodes wider than a front may be
    out.append(("cart_pole1000/mf/sn_max_width_16", "cart_pole", 1000, dict(MF, SLPX_HOSTCHECK_SN_MAX_WIDTH="16"), []))
    # the default build's own permutation fed back in as user_perm
    out.append(("cart_pole300/mf/user_perm", "cart_pole", 300, MF, ["--user-perm"]))
    out.append(("flywheel50/user_perm", "flywheel", 50, {}, ["--user-perm"]))
    # the dense branch: by the reference's density rule (pivoted), and because no column of L fits a task
    out.append(("shooting40/dense_pivoted", "shooting", 40, {}, []))
    out.append(("shooting300/dense", "shooting", 300, {"SLPX_DENSE": "0"}, []))
    out.append(("shooting40/sparse", "shooting", 40, dict(MF, SLPX_DENSE="0"), []))
    # the first attempt of build_ldlt_plan throws "a single column exceeds the LDS task budget" (a column of four
    # entries below the diagonal already costs 4 + 2 + 17 / 4 = 10 > 8 entry-equivalents), the retry with the sharper hub rule and
    # the default task size succeeds
    out.append(("cart_pole24/task_entries_8/retry", "cart_pole", 24, MF, ["--task-entries", "8"]))
    out.append(("gfold100/mf/task_entries_256/retry", "gfold", 100, MF, ["--task-entries", "256"]))
    # small irregular models (SLPX_DENSE=0: the sparse plan also where the reference's rule takes the dense branch)
    for name in ("eq:rosenbrock", "eq:newton_chain", "eq:circle", "eq:pendulum", "fr:tiny", "fr:ineq_only", "fr:eq_only", "fr:chain300"):
        out.append((f"{name}/mf/sparse", name, 0, dict(MF, SLPX_DENSE="0"), []))
    # plans do not depend on the number of setup threads
    for kind, N in (("cart_pole", 700), ("cart_pole", 5000)):
        for threads in (1, 3, 8):
            out.append((f"{kind}{N}/mf/threads_{threads}", kind, N, dict(MF, SLPX_SETUP_THREADS=str(threads)), []))
    return out


KNOBS = ("SLPX_LDLT_MF", "SLPX_HOSTCHECK_PRODUCT_BATCH", "SLPX_HOSTCHECK_SINGLE_PROBLEM_RULES", "SLPX_HOSTCHECK_COLUMN_PLAN", "SLPX_HOSTCHECK_SN_MAX_WIDTH",
         "SLPX_MFMA_MIN_ENTRIES", "SLPX_SN_MIN_WIDTH", "SLPX_SN_MAX_WIDTH", "SLPX_SN_BALANCE", "SLPX_SN_DEEPEST", "SLPX_RELAX_ZEROS",
         "SLPX_SUPERNODAL", "SLPX_DENSE", "SLPX_SETUP_THREADS", "SLPX_TASK_ENTRIES", "SLPX_LDLT_VERBOSE", "SLPX_SETUP_TIMING")


def run(only=None):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    base["PYTHONPATH"] = str(ROOT)
    for name, kind, N, env, args in cases():
        if only and only not in name:
            continue
        res = subprocess.run([sys.executable, "-m", "tests.support.plan_hash_cli", kind, str(N), "--info", *args], cwd=ROOT,
                             env=dict(base, **env), capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            row = {"error": (res.stderr.strip().splitlines() or ["?"])[-1]}
        else:
            row = json.loads(res.stdout.strip().splitlines()[-1])
            row["hash"] = [f"{h:016x}" for h in row["hash"]]
        print(json.dumps({"case": name, **row}), flush=True)


def compare(path_a, path_b):
    a, b = (Path(p).read_text().strip().splitlines() for p in (path_a, path_b))
    print("parent:")
    print("\n".join(a))
    print("\nbranch:")
    print("\n".join(b))
    rows_a, rows_b = ({r["case"]: r for r in map(json.loads, lines)} for lines in (a, b))
    different = sorted(k for k in rows_a if rows_a[k] != rows_b.get(k))
    added = sorted(k for k in rows_b if k not in rows_a)
    failed = sorted(k for k, r in rows_a.items() if "error" in r)
    print()
    for k in different:
        print(f"DIFFERENT: {k}")
    for k in failed:
        print(f"NOT BUILT AT THE PARENT: {k}")
    for k in added:
        print(f"NEW IN THE BRANCH: {k}")
    print(f"{len(rows_a)} rows compared")
    print("identical" if not different else f"{len(different)} DIFFERENT")
    return 1 if different else 0


if __name__ == "__main__":
    if len(sys.argv) in (2, 3) and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) == 3 else None)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
