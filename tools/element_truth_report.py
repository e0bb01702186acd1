#!/usr/bin/env python3
"""Prints, for every family of tests/golden/element_truth.npz, metric and device path, the device's worst error against
the quad-precision truth, the FP64 oracle's, their ratio and the bound of tests/test_gpu_element_truth.py (needs a GPU).
profiles/element_truth_vs_quad.txt is the output of this script."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import truth  # noqa: E402
from tests.helpers.product import ensure_built  # noqa: E402


def main():
    pkg = ensure_built()
    fx = dict(truth.load())
    print("device error / FP64 oracle error against quad precision, worst over each family of 8 elements; bound: device <= "
          "max(4 x oracle, 16 eps = %.2e)" % (16 * truth.EPS))
    print("%-4s %-12s %-34s %10s %10s %8s %10s  %s" % ("fam", "metric", "path", "device", "oracle", "ratio", "bound", ""))
    over = 0
    for fam in truth.FAMILIES:
        # (the "own" paths: the whole family in one mesh, a section per material, where the family has more than one)
        for path in truth.PATHS + (truth.OWN_PATHS if fam in truth.OWN_FAMILIES else []):
            for name in ("FEMSHELL_SYMMETRIC", "FEMSHELL_ASM_PIPE"):  # a path that sets neither runs under the defaults
                os.environ.pop(name, None)
            worst = truth.device_family_errors(pkg, os.environ.__setitem__, fx, fam, path)
            for m in truth.metrics_of(fam):
                o = float(fx["%s_err_%s" % (fam, m)].max())
                b = truth.bound(o)
                over += worst[m] > b
                print("%-4s %-12s %-34s %10.2e %10.2e %8.2f %10.2e  %s" % (fam, m, truth.path_id(path), worst[m], o, worst[m] / o, b,
                                                                         "OVER" if worst[m] > b else ""))
            if "spurious" in worst:
                over += worst["spurious"] > 0
                print("%-4s %-12s %-34s %10d %10d %8s %10d  %s" % (fam, "spurious", truth.path_id(path), worst["spurious"], 0, "-", 0,
                                                                 "OVER" if worst["spurious"] else ""))
        sys.stdout.flush()
    print("%d over their bound" % over)


if __name__ == "__main__":
    main()
