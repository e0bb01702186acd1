#!/usr/bin/env python3
"""Prints what tests/test_gpu_jacobi_truth.py and tests/test_gpu_spectral_bound.py measure: the error of the device's 6 x 6
block-Jacobi inverse (csrc/kernels.hip k_block_jacobi) against the exact truth of tests/helpers/jacobi_truth.py over the error of
the plain-double restatement, per family and storage; the worst error / budget of the two readers of the packed inverse per
level and vector; and lambda_device / lambda_true with the distance to the restated power iteration per mesh and level.
profiles/block_jacobi_and_spectral_bound.txt is the output of this script on an MI355X.

    python tools/jacobi_truth_report.py [output file]        needs a GPU"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import jacobi_truth as jt  # noqa: E402
from tests.helpers.product import ensure_built, pkg  # noqa: E402

LD = jt.LD


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


def lambda_rows(name, safety=1.1, iterations=30):
    """[(level, nodes, lambda_device, lambda_device / lambda_true, distance to the restated iteration)] of a fresh context"""
    ctx = jt.spectral_context(pkg, name)
    ctx.block_jacobi_export(0)
    lv = ctx.amg_levels()
    rows = []
    for l in range(len(lv) - 1):
        r, c, v = jt.level_operator(ctx, l)
        eld = float(jt.restated_lambda(r, c, v, ctx.block_jacobi_export(l), iterations, LD))
        lam = lv[l]["lambda_max"]
        rows.append((l, lv[l]["n_nodes"], lam, lam / jt.true_lambda(r, c, v), abs(lam / safety - eld) / eld))
    ctx.close()
    return rows


def variants(say):
    """the knobs, the row partition and the float copy: what tests/test_gpu_spectral_bound.py and the float-copy test assert"""
    import tempfile
    from pathlib import Path

    from tests.helpers import meshes
    from tests.test_multirank_gpu import run_ranks, stacked_k_rows, stacked_level_rows

    say("# variants: lambda_device / lambda_true and the distance of lambda_device / safety from the restated iteration")
    runs = [("curved, every step on the device (FEMSHELL_AMG_DEVICE_MIN=100), patterns in HBM", "curved", {"FEMSHELL_AMG_DEVICE_MIN": "100"}, 1.1, 30),
            ("curved, every step on the device, FEMSHELL_AMG_SYMBOLIC=host", "curved", {"FEMSHELL_AMG_DEVICE_MIN": "100", "FEMSHELL_AMG_SYMBOLIC": "host"}, 1.1, 30),
            ("strip, default", "strip", {}, 1.1, 30),
            ("strip, FEMSHELL_AMG_LAMBDA_SAFETY=1.3", "strip", {"FEMSHELL_AMG_LAMBDA_SAFETY": "1.3"}, 1.3, 30),
            ("strip, FEMSHELL_AMG_POWER_ITS=60", "strip", {"FEMSHELL_AMG_POWER_ITS": "60"}, 1.1, 60)]
    for title, name, env, safety, its in runs:
        for l, n, lam, ratio, dist in with_env(env, lambda: lambda_rows(name, safety, its)):
            say("%-84s level %d %5d nodes | lambda %.15f | %8.4f %9.1e" % (title, l, n, lam, ratio, dist))
    with tempfile.TemporaryDirectory() as tmp:
        env = {"FEMSHELL_AMG_DIST_MIN": "100", "FEMSHELL_TEST_AMG_EXPORT": "1", "FEMSHELL_TEST_EXPORT": "1"}
        ranks = sorted(run_ranks(2, "panel", Path(tmp), pc="amg", extra_env=env), key=lambda q: int(q["begin"]))
    lam = np.asarray(ranks[0]["amg_lambda"])
    same = all(np.asarray(r["amg_lambda"]).tobytes() == lam.tobytes() for r in ranks)
    for level in range(int(ranks[0]["amg_partitioned_levels"])):
        rp, ci, va = stacked_k_rows(ranks) if level == 0 else stacked_level_rows(ranks, level, "A")
        n = len(rp) - 1
        true = jt.true_lambda(rp, ci, va) if 6 * n <= 3600 else jt.true_lambda_sparse(rp, ci, va)
        say("%-84s level %d %5d nodes | lambda %.15f | %8.4f" % ("two ranks, the panel of the multi-rank tests, FEMSHELL_AMG_DIST_MIN=100 (%s)"
                                                                 % ("both ranks report the same bits" if same else "THE RANKS DIFFER"), level, n, lam[level], lam[level] / true))
    m = meshes.structured(64, 64, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    ctx = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    ctx.set_mesh(m.xyz, m.tri)
    ctx.set_dirichlet(m.dirichlet_mask())
    ctx.set_loads(m.loads)
    ctx.set_preconditioner("amg")
    B64, B32 = ctx.block_jacobi_export(0), ctx.block_jacobi_export(0, single_precision=True)
    n = ctx.n_nodes
    r = np.random.default_rng(22).standard_normal(((n + 31) // 32 * 32, 6))
    z1 = ctx.block_jacobi_apply(0, 1, r).reshape(-1, 6)[:n].astype(LD)
    w32, b32 = jt.apply_truth(B32, r[:n])
    w64, b64 = jt.apply_truth(B64, r[:n])
    ctx.close()
    say("# float copy (64 x 64 panel, default multigrid context): export(single precision) %s float32(export(double)); the lane-per-node reader"
        % ("=" if np.array_equal(B32, B64.astype(np.float32).astype(np.float64)) else "DIFFERS FROM"))
    say("#   is at %.3f of the budget against the float matrix and at %.1e of it against the double one"
        % (float((np.abs(z1 - w32) / b32).max()), float((np.abs(z1 - w64) / b64).max())))


def main():
    ensure_built()
    for k in ("FEMSHELL_SYMMETRIC", "FEMSHELL_AMG_LAMBDA_SAFETY", "FEMSHELL_AMG_POWER_ITS", "FEMSHELL_AMG_SYMBOLIC"):
        os.environ.pop(k, None)
    out = []
    say = lambda s: (out.append(s), print(s, flush=True))
    fs = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    say("# block-Jacobi inverse against the exact rational truth: err = max|S (B - T) S| / max|S T S|, S = diag(sqrt(A_ii)); worst over")
    say("# the family; bound = max(4 x restated, 16 eps).  storage 0: every block, 1: diagonal + upper blocks, 2: the same read as K's")
    say("# diagonal slots (upper triangle only).  nodes per launch: " + ", ".join(map(str, jt.NODE_COUNTS)))
    say("%-10s %7s | %9s %9s %9s | %s" % ("family", "storage", "device", "restated", "bound", "device / restated"))
    for name in jt.SYNTHETIC:
        c = jt.case(name)
        for storage in (0, 1, 2):
            worst = 0.0
            for n in jt.NODE_COUNTS:
                sel = slice(0, n) if n == jt.PER_FAMILY else slice(jt.PER_FAMILY - n, jt.PER_FAMILY)
                B, status = fs.amg_device_block_jacobi(*jt.launch_matrix(c["A"][sel], n), symmetric_storage=storage)
                assert status == 0
                worst = max(worst, jt.worst(B, c["T"][sel], c["A"][sel]))
            say("%-10s %7d | %9.2e %9.2e %9.2e | %.2f" % (name, storage, worst, c["worst"], c["bound"], worst / c["worst"]))
    fs.close()
    say("# real blocks: K on the element families of tests/golden/element_truth.npz (isolated elements, Dirichlet masks dealt out), per")
    say("# family and FEMSHELL_SYMMETRIC, the contexts of the family's flags pooled")
    for symmetric in ("1", "0"):
        os.environ["FEMSHELL_SYMMETRIC"] = symmetric
        pooled = {}
        for label, flags, case in jt.real_cases():
            ctx = pkg.FemShell(*case.sections[0], flags=flags, device=0)
            case.apply(ctx)
            ctx.assemble()
            r, c, v, _ = ctx.export_bsr()
            B = ctx.block_jacobi_export(0)
            ctx.close()
            D = jt.as_read(jt.diagonal_blocks(r, c, v), upper=symmetric == "1")
            T = jt.truths(D)
            e, e_r = jt.worst(B, T, D), jt.worst(jt.restated(D)[0], T, D)
            cond = max(jt.scaled_condition(b) for b in D)
            p = pooled.setdefault(label.split("-")[0], [0.0, 0.0, 0.0])
            p[:] = [max(p[0], e), max(p[1], e_r), max(p[2], cond)]
        for fam, (e, e_r, cond) in pooled.items():
            say("%-4s symmetric %s: scaled condition %8.1e | %9.2e %9.2e %9.2e | %.2f" % (fam, symmetric, cond, e, e_r, jt.bound(e_r), e / e_r))
    os.environ.pop("FEMSHELL_SYMMETRIC", None)
    say("# multigrid contexts (coarsest_nodes = 60): per level the inverse against the truth of the exported diagonal blocks, the two readers")
    say("# (worst |z - B r| / (6 eps sum |B_ij| |r_j|) over the rows, random r), lambda_device / lambda_true, and the distance of")
    say("# lambda_device / 1.1 from the restated power iteration (in long double) beside that of the restatement in double")
    say("%-9s %5s %5s | %9s %9s | %6s %6s %5s | %8s %9s %9s" % ("mesh", "level", "nodes", "device", "restated", "path0", "path1", "bits", "lam/true", "distance", "dbl-ld"))
    rng = np.random.default_rng(21)
    for name in jt.SPECTRAL_MESHES:
        ctx = jt.spectral_context(pkg, name)
        B0 = ctx.block_jacobi_export(0)
        patches = ctx.amg_patch_info()
        lv = ctx.amg_levels()
        for l in range(len(lv)):
            r, c, v = jt.level_operator(ctx, l)
            D = jt.as_read(jt.diagonal_blocks(r, c, v), upper=l == 0)
            B = B0 if l == 0 else ctx.block_jacobi_export(l)
            T = jt.truths(D)
            e, e_r = jt.worst(B, T, D), jt.worst(jt.restated(D)[0], T, D)
            n = lv[l]["n_nodes"]
            n_pad = (n + 31) // 32 * 32
            rv = rng.standard_normal((n_pad, 6))
            want, budget = jt.apply_truth(B, rv[:n])
            z = [ctx.block_jacobi_apply(l, path, rv).reshape(-1, 6) for path in (0, 1)]
            over = [float((np.abs(zz[:n].astype(LD) - want) / budget).max()) for zz in z]
            line = "%-9s %5d %5d | %9.2e %9.2e | %6.3f %6.3f %5s |" % (name, l, n, e, e_r, over[0], over[1], "same" if np.array_equal(z[0], z[1]) else "differ")
            if l + 1 < len(lv):
                clustered = l == 0 and patches["clusters"] > 0
                true = jt.true_lambda(r, c, v, labels=ctx.amg_export(0)["patch_labels"] if clustered else None)
                line += " %8.4f" % (lv[l]["lambda_max"] / true)
                if clustered:
                    line += " (level 0 smooths with %d clusters of rigidly coupled nodes: D over the clusters)" % patches["clusters"]
                else:
                    e64, eld = float(jt.restated_lambda(r, c, v, B, 30)), float(jt.restated_lambda(r, c, v, B, 30, LD))
                    line += " %9.1e %9.1e" % (abs(lv[l]["lambda_max"] / 1.1 - eld) / eld, abs(e64 - eld) / eld)
            say(line)
        ctx.close()
    variants(say)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
