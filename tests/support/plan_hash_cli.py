"""Prints the hashes of the compiled plans (hostcheck.HostCheck.plan_hash) of one model as JSON: run in a process
of its own so that SLPX_SETUP_THREADS / SLPX_LDLT_MF take effect (the setup pool is made once per process).
    python -m tests.support.plan_hash_cli cart_pole 300
Models: cart_pole, flywheel, gfold, shooting (single shooting: the dense branch), eq:<name> (tests/support/eq_models.py:
rosenbrock, newton_chain, circle, pendulum; N ignored) and fr:<name> (tests/support/fr_models.py: tiny, ineq_only,
eq_only, chain<n>; N ignored).  Options, for profiles/plan_hash_matrix.py:
    --task-entries K   LdltOptions::task_entries
    --small-lds B      the tape compiler's small-task LDS, bytes
    --user-perm        build once, then again with the first build's own permutation as `user_perm`: hashes of the second
    --info             a JSON object {"hash", "tasks", "rounds", "mf", "mfma", "dense"} instead of the list of hashes
    --product-batch B  the options the product gives this model in a batch of B (csrc/system_choice.cpp:
                       choose_ldlt_options and the plan route of NewtonSystem) instead of hostcheck's own knobs
    --first-pass       with --info: also "tasks_first_pass", the tasks of the same build without
                       SLPX_HOSTCHECK_SINGLE_PROBLEM_RULES (another count: the partition was redone with bigger tasks)"""
import argparse
import json
import os

import sleipnir_amd as sa
from tests.support import hostcheck, models


def problem(kind: str, N: int):
    if kind == "cart_pole":
        return models.cart_pole(N, 5.0 / N)
    if kind == "flywheel":
        return models.flywheel(N, 0.005)
    from tests.support import model

    m = model.Model(model.ProductBackend("hostcheck"))
    if kind == "gfold":
        from tests.support import gfold

        return gfold.build(m, N).p
    if kind == "shooting":
        from tests.support import shooting

        return shooting.build(m, N).p
    family, _, name = kind.partition(":")
    if family == "eq":
        from tests.support import eq_models

        return getattr(eq_models, name)(m).p
    if family == "fr":
        from tests.support import fr_models

        return fr_models.make(m, name)[0].p
    raise SystemExit(f"unknown model {kind!r}")


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("kind")
    ap.add_argument("N", type=int)
    ap.add_argument("--task-entries", type=int, default=0)
    ap.add_argument("--small-lds", type=int, default=0)
    ap.add_argument("--user-perm", action="store_true")
    ap.add_argument("--info", action="store_true")
    ap.add_argument("--first-pass", action="store_true")
    ap.add_argument("--product-batch", type=int, default=0)
    a = ap.parse_args(argv)
    if a.product_batch > 0:
        os.environ["SLPX_HOSTCHECK_PRODUCT_BATCH"] = str(a.product_batch)
    sa.lib().slpx_graph_reset()
    pp = problem(a.kind, a.N)
    kw = {"task_entries": a.task_entries, "small_lds_bytes": a.small_lds}
    hc = hostcheck.HostCheck(pp, **kw)
    if a.user_perm:
        hc = hostcheck.HostCheck(pp, perm=hc.perm(), **kw)
    if not a.info:
        print(json.dumps(hc.plan_hash()))
        return
    mf = hc.mf_plan()
    row = {"hash": hc.plan_hash(), "tasks": hc.info["ldlt_tasks"], "rounds": hc.info["ldlt_rounds"],
           "mf": bool(mf["built"]), "mfma": mf["mfma_fronts"], "dense": hc.is_dense()}
    if a.first_pass:
        os.environ.pop("SLPX_HOSTCHECK_SINGLE_PROBLEM_RULES", None)
        row["tasks_first_pass"] = hostcheck.HostCheck(pp, **kw).info["ldlt_tasks"]
    print(json.dumps(row))


if __name__ == "__main__":
    main()
