#!/usr/bin/env python3
"""Prints, for every case of tests/test_gpu_dense_inverse.py, the error of the device's dense inverse (csrc/amg_dense.hip)
against the long-double truth of tests/helpers/dense_truth.py beside the errors of the plain-double restatement of the method
and of LAPACK on the same matrix, the ratio to the tests' bound, the dropped directions, and whether the variants that only
redistribute work give the default's bits.  profiles/dense_inverse_vs_long_double.txt is the output of this script on an MI355X.

    python tools/dense_inverse_report.py [output file]        needs a GPU"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import dense_truth as dt  # noqa: E402
from tests.helpers.product import ensure_built, pkg  # noqa: E402

KNOBS = ("FEMSHELL_AMG_DENSE_LOOKAHEAD", "FEMSHELL_AMG_DENSE_XCD_MAP", "FEMSHELL_AMG_DENSE_PANEL_SPLIT")


def with_env(name, value, f):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return f()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def main():
    ensure_built()
    for k in KNOBS + ("FEMSHELL_AMG_DENSE_TILE",):
        os.environ.pop(k, None)
    out = []
    say = lambda s: (out.append(s), print(s, flush=True))
    fs = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    say("# device dense inverse against the long-double truth: err(X) = max|X - X*| / max|X*|; bound = 4 x max(restated, n 2^-53);")
    say("# family b: 4 x max(restated, block, cond(pivot block) 2^-53, n 2^-53).  restated: scalar sweeps in plain double; block: the")
    say("# device's block structure (explicit pivot-block inverses) in plain double; x4scalar: device / (4 x max(restated, n 2^-53))")
    say("# families: a random SPD, b graded and shell-like, c Galerkin operator of the host coarsening, d planted dead directions")
    say("%-22s %5s %5s %8s %8s | %9s %9s %9s %9s | %9s %6s %8s | %7s | %s" % ("case", "n", "n_pad", "cond", "condpiv", "device", "restated",
                                                                          "block", "lapack", "bound", "ratio", "x4scalar", "dropped", "variants"))
    worst = {}
    cases = [(f, w) for f, w in dt.ACCURACY_CASES] + [("d", c) for c in dt.PLANTED_CASES]
    for fam, which in cases:
        c = dt.case(fam, which)
        run = lambda **kw: fs.amg_device_dense_inverse(*c["bcsr"], **kw)
        X, st = run()
        e = dt.err(X, c["truth"])
        notes = []
        if fam != "d" and which in dt.VARIANT_SHAPES:
            for knob in KNOBS:
                Xv, _ = with_env(knob, "0", run)
                notes.append("%s=0 %s" % (knob.replace("FEMSHELL_AMG_DENSE_", ""), "same bits" if np.array_equal(Xv, X) else "DIFFERENT"))
            Xt, _ = with_env("FEMSHELL_AMG_DENSE_TILE", "128", run)
            notes.append("TILE=128 %.2e%s" % (dt.err(Xt, c["truth"]), " (same bits)" if np.array_equal(Xt, X) else ""))
            X32, _ = run(single_precision=True)
            notes.append("f32 %s" % ("= rounded FP64" if np.array_equal(X32, X.astype(np.float32).astype(np.float64)) else "DIFFERENT"))
        name = "%s-%s" % (fam, which if fam != "d" else "%d-%s" % (which[0], "_".join(map(str, which[1]))))
        ratio = e / c["bound"]
        worst[fam] = max(worst.get(fam, 0.0), ratio)
        say("%-22s %5d %5d %8.1e %8.1e | %9.2e %9.2e %9.2e %9.2e | %9.2e %6.3f %8.2f | %3d/%-3d | %s"
            % (name, c["n"], dt.n_pad(c["n"]), c["cond"], c["kappa_pivot"], e, c["e_restated"], c["e_block"], c["e_lapack"], c["bound"], ratio,
               e / dt.bound(c["e_restated"], c["n"]), st["dropped_directions"], len(c["dead"]), "; ".join(notes)))
    say("# worst device error / bound per family: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    fs.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
