#!/usr/bin/env python3
"""Prints what tests/test_gpu_krylov_truth.py holds: per step of femshell_krylov_launch, mesh and storage the largest share of
its bound the intact code uses (dot_bound, axpy_bound, the block-Jacobi readers' bound, the product's: tests/helpers/krylov_truth.py)
and the number of bitwise cases, the same for the two-stage reduction at every length, and the chains that are the solve.
Nothing in the tests depends on a number printed here: every tolerance there is a derived bound or bitwise equality.
profiles/krylov_steps_vs_exact.txt is the output of this script on an MI355X.

    python tools/krylov_truth_report.py [output file]        needs a GPU"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import krylov_cases as kc  # noqa: E402
from tests.helpers import krylov_truth as kt  # noqa: E402
from tests.helpers.product import ensure_built, pkg  # noqa: E402

SETTINGS = [("1", "1"), ("1", "0"), ("0", "1")]  # (FEMSHELL_SYMMETRIC, FEMSHELL_SPMV_LOCAL)


def with_env(env, f):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return f()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def by_step(out):
    """{step: (largest share, bitwise cases, cases)} of a check's {label: share}: a label begins with its step"""
    rows = {}
    for label, share in out.items():
        step = label.split(" ")[0] if not label.startswith("gated") else "gated"
        worst, bitwise, count = rows.get(step, (0.0, 0, 0))
        rows[step] = (max(worst, share), bitwise + (share == 0.0), count + 1)
    return rows


def reduction(say):
    say("# the two-stage reduction (femshell_cg_reduce): groups, largest |red - exact| / (gamma_len sum |partials|) over random and")
    say("# cancelling words, whether the bits are reduce_model's, integer and one-hot launches that came back exact")
    ctx = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    for n in kt.REDUCE_LENGTHS:
        rng = np.random.default_rng(n)
        exact = 0
        for nsums in (1, 2, 3):
            for len3 in sorted({1, max(n // 2, 1), n}) if nsums == 3 else (0,):
                arrays = [kt.integer_partials(n), kt.integer_partials(n) + float(n), 3.0 * kt.integer_partials(len3)][:nsums]
                red, ticket = ctx.cg_reduce(np.concatenate(arrays), n, nsums, len3)
                for a in range(nsums):
                    kt.assert_reduction_exact(red[a], arrays[a])
                exact += 1
        for i in kt.chunk_edges(n):
            assert ctx.cg_reduce(kt.one_hot(n, i), n)[0][0] == 1.0
            exact += 1
        worst, model = 0.0, True
        for p in (kt.random_partials(rng, n), kt.cancelling(rng, n)):
            red = ctx.cg_reduce(p, n)[0][0]
            worst = max(worst, kt.assert_reduction_within(red, p))
            model = model and kt.bits(red) == kt.bits(kt.reduce_model(p))
        say("n %6d  groups %2d  share %.4f  model bits %s  exact launches %d" % (n, kt.reduce_groups(n), worst, model, exact))
    ctx.close()


def steps(say):
    say("")
    say("# the steps: mesh, FEMSHELL_SYMMETRIC, FEMSHELL_SPMV_LOCAL, step: largest share of its bound, bitwise cases / cases")
    for name in kc.MESHES:
        for symmetric, local in SETTINGS:
            def run():
                fs = kc.context(pkg, name)
                out = kc.check_vector_steps(fs)
                if symmetric == "1":
                    out.update(kc.check_gathered_updates(fs))
                out.update(kc.check_product(fs, symmetric == "1"))
                out.update(kc.check_gating(fs, symmetric == "1"))
                fs.close()
                return out
            rows = by_step(with_env({"FEMSHELL_SYMMETRIC": symmetric, "FEMSHELL_SPMV_LOCAL": local}, run))
            for step in sorted(rows):
                say("%-8s sym %s local %s  %-18s share %.4f  bitwise %3d / %3d" % ((name, symmetric, local, step) + rows[step]))
    for name in ("curved", "panel49", "strip", "mixed"):
        for symmetric in ("1", "0"):
            def run():
                fs = kc.context(pkg, name, pc="amg", refine_passes=0)
                out = kc.check_flexible_update_start(fs, symmetric == "1")
                out.update(kc.check_pc_apply(fs))
                fs.close()
                return out
            rows = by_step(with_env({"FEMSHELL_SYMMETRIC": symmetric}, run))
            for step in sorted(rows):
                say("%-8s sym %s local 1  %-18s share %.4f  bitwise %3d / %3d" % ((name, symmetric, step) + rows[step]))


def chains(say):
    say("")
    say("# chained probes against solve(rtol = 0, max_it = k), k = 1, 2, 9, 17: x and history bit for bit (an AssertionError otherwise)")
    for name in ("curved", "panel49"):
        for symmetric in ("1", "0"):
            sym = symmetric == "1"

            def jacobi():
                fs = kc.context(pkg, name)
                n = len(with_env({"FEMSHELL_CG_SINGLE_REDUCTION": "0"}, lambda: kc.assert_chain_is_the_solve(fs, lambda k: kc.chain_classic(fs, k, sym), "classic")))
                for fold in ("1", "0"):
                    n += len(with_env({"FEMSHELL_CG_SINGLE_REDUCTION": "1", "FEMSHELL_CG_FOLD": fold},
                                      lambda: kc.assert_chain_is_the_solve(fs, lambda k: kc.chain_single_reduction(fs, k, sym, fold == "1"), "single")))
                fs.close()
                return n

            def multigrid(fuse):
                fs = kc.context(pkg, name, pc="amg", refine_passes=0)
                fused = fuse == "3" and len(fs.amg_levels()) > 1
                n = len(kc.assert_chain_is_the_solve(fs, lambda k: kc.chain_flexible(fs, k, sym, fused), "flexible"))
                fs.close()
                return n

            n = with_env({"FEMSHELL_SYMMETRIC": symmetric}, jacobi)
            for fuse in ("0", "3"):
                n += with_env({"FEMSHELL_SYMMETRIC": symmetric, "FEMSHELL_AMG_FUSE": fuse}, lambda: multigrid(fuse))
            say("%-8s sym %s  %d chains are the solve (classic, single-reduction folded and not, flexible with FEMSHELL_AMG_FUSE 0 and 3)" % (name, symmetric, n))


def main():
    ensure_built()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    reduction(say)
    steps(say)
    chains(say)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
