#!/usr/bin/env python3
"""Prints, for every family of tests/golden/derived_truth.npz, displacement state, metric and device path, the device's worst
error against the long-double truth, the FP64 reference's, their ratio and the bound of tests/test_gpu_derived_truth.py (needs a
GPU).  profiles/derived_truth_vs_long_double.txt is the output of this script."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import derived_truth as dt, truth  # noqa: E402
from tests.helpers.product import ensure_built  # noqa: E402


def rows(dx, fam, label, worst, metrics=None):
    """prints the lines of one (family, path); returns how many are over their bound"""
    from tests.test_gpu_derived_truth import FACTORS
    over = 0
    for m in (dt.metrics_of(fam) if metrics is None else metrics):
        per_state = np.ndim(worst[m]) > 0
        for s in (range(len(dt.STATES)) if per_state else [None]):
            w = float(worst[m][s]) if per_state else float(worst[m])
            o = dt.reference_worst(dx, fam, m, s)
            factor = FACTORS.get(fam, {}).get(m, 4.0)
            b = truth.bound(o, factor)
            over += not w <= b
            print("%-4s %-7s %-7s %-14s %10.2e %10.2e %8s %10.2e  %s" % (fam, dt.STATES[s] if per_state else "-", m, label, w, o,
                                                                         "%.2f" % (w / o) if o > 0 else "-", b, ("" if factor == 4.0 else "factor %g" % factor) if w <= b else "OVER"))
    if "spurious" in worst:
        n = int(np.max(worst["spurious"]))
        over += n > 0
        print("%-4s %-7s %-7s %-14s %10d %10d %8s %10d  %s" % (fam, "-", "spurious", label, n, 0, "-", 0, "OVER" if n else ""))
    return over


def main():
    pkg = ensure_built()
    fx, dx = dict(truth.load()), dict(dt.load())
    print("device error / FP64 reference error against long double, worst over each family of 8 elements (all copies); bound: device <= "
          "max(4 x reference, 16 eps = %.2e), 4 unless the line names another factor" % (16 * truth.EPS))
    print("%-4s %-7s %-7s %-14s %10s %10s %8s %10s" % ("fam", "state", "metric", "path", "device", "reference", "ratio", "bound"))
    over = 0
    for fam in truth.FAMILIES:
        for sectioned in dt.PATHS + (("own",) if fam in truth.OWN_FAMILIES else ()):
            over += rows(dx, fam, dt.path_id(sectioned), dt.device_family_worst(pkg, fx, dx, fam, sectioned))
        sys.stdout.flush()
    from tests.test_gpu_element_truth import MIXED, MIXED_OWN
    default = tuple(truth.DEFAULT_MATERIAL[:3]) + (3,)
    cases = [(MIXED, sec, default, [(f, e) for f in MIXED for e in range(truth.PER_FAMILY) if truth.material_of(fx, f, e) == default])
             for sec in dt.PATHS]
    cases.append((MIXED_OWN, "own", truth.OWN_CONTEXT + (3,),
                  [(f, e) for f in MIXED_OWN for e in range(truth.PER_FAMILY) if truth.material_of(fx, f, e)[3] == 3]))
    for families, sectioned, material, elements in cases:
        got = dt.device_results(pkg, material, [(f, e, False) for f, e in elements], sectioned, fx, dx)
        for fam in families:
            els = [e for f, e in elements if f == fam]
            worst = dt.family_worst(fx, dx, fam, [got[(fam, e, False)] for e in els], elements=els)
            over += rows(dx, fam, "mixed-" + dt.path_id(sectioned), worst, dt.MIXED_METRICS)
        sys.stdout.flush()
    print("%d over their bound" % over)


if __name__ == "__main__":
    main()
