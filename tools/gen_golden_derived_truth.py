#!/usr/bin/env python3
"""Writes tests/golden/derived_truth.npz: stress resultants, geometric stiffness coefficients, element-load shares and lumped
masses of the 13 families of 8 elements of tests/golden/element_truth.npz, in two displacement states, evaluated by the numpy
reference in long double (every intermediate; tests/helpers/derived_truth.py has the layout) and rounded once to double, with the
FP64 reference's own distance from them per metric.  The device is held to a small multiple of that distance
(tests/test_gpu_derived_truth.py); tests/test_derived_truth_cpu.py checks that this file is what the reference computes here.
Fixed seeds: running this again reproduces the file bit for bit.

The displacement states:
  random   u uniform in (-1, 1), all six dofs
  smooth   translations A (x - x_first), A a random 3 x 3 matrix of entries ~1e-4, formed in long double and rounded to double;
           rotations random, ~1e-4.  The first node is the origin, not the coordinate origin: at distance 1e8 (T5) the rounding of
           A x to double alone is a strain of 1e-8.
Every stored (element, state) has the FP64 reference within derived_truth.CONDITION of the truth in N, M, vm and g; a state that
does not would get another seed here (RESEED), the element stays.  None needed one.
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import derived_truth as dt, element_loads as el, truth  # noqa: E402

N = truth.PER_FAMILY
LD = dt.LD
RESEED = {}  # (family, element, state) -> seed of that entry's displacements, where the family's own draw is over CONDITION


def displacements(rng, xyz, state):
    nn = len(xyz)
    if state == 0:
        return rng.uniform(-1.0, 1.0, (nn, 6))
    A = rng.normal(size=(3, 3)) * 1e-4
    u = np.zeros((nn, 6))
    X = xyz.astype(LD)
    u[:, :3] = ((X - X[0]) @ A.T.astype(LD)).astype(np.float64)
    u[:, 3:] = rng.normal(size=(nn, 3)) * 1e-4
    return u


def save_npz(path, arrays):
    """np.savez with a fixed time stamp on every member: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    assert dt.long_double_is_extended(), "numpy's long double has fewer than 64 bits of mantissa here"
    fx = dict(truth.load())
    out = {}
    densities = {}  # one per distinct (nu, E, t), in the order of first appearance
    rho_rng = np.random.default_rng(20261999)
    for idx, fam in enumerate(truth.FAMILIES):
        rng = np.random.default_rng(20261000 + idx)
        nn = truth.nodes_of(fam)
        xyz = fx[fam + "_xyz"]
        u = np.zeros((2, N, nn, 6))
        for s in range(2):
            for e in range(N):
                r = np.random.default_rng(RESEED[fam, e, s]) if (fam, e, s) in RESEED else rng
                u[s, e] = displacements(r, xyz[e], s)
        out[fam + "_u"] = u
        if fam in truth.FRAME:
            Q = fx[fam + "_Q"].astype(LD)
            um = np.zeros_like(u)
            for s in range(2):
                for e in range(N):
                    ul = u[s, e].astype(LD)
                    um[s, e] = np.concatenate([ul[:, :3] @ Q[e].T, ul[:, 3:] @ Q[e].T], axis=1).astype(np.float64)
            out[fam + "_u_moved"] = um
        loads = el.random_loads(N, 0, seed=100 + idx)[0]
        rho = np.zeros(N)
        for e in range(N):
            m = truth.material_of(fx, fam, e)[:3]
            if m not in densities:
                densities[m] = float(rho_rng.uniform(0.5, 9.5)) * 1e-9
            rho[e] = densities[m]
        out[fam + "_load"], out[fam + "_rho"] = loads, rho

        tr = [[dt.reference(fx, out, fam, e, s, LD) for s in range(2)] for e in range(N)]
        out[fam + "_res"] = np.array([[tr[e][s]["res"] for e in range(N)] for s in range(2)])
        out[fam + "_g"] = np.array([[truth.upper(tr[e][s]["g"]) for e in range(N)] for s in range(2)])
        out[fam + "_share"] = np.array([tr[e][0]["share"] for e in range(N)])
        out[fam + "_mass"] = np.array([tr[e][0]["mass"] for e in range(N)])
        ref = [[dt.reference(fx, out, fam, e, s) for s in range(2)] for e in range(N)]
        if fam in dt.FLAT:
            out[fam + "_zero"] = np.array([[(tr[e][s]["res"][:12] == 0.0) & (ref[e][s]["res"][:12] == 0.0) for e in range(N)]
                                           for s in range(2)])
        moved = None
        if fam in truth.FRAME:
            moved = [[dt.reference(fx, out, fam, e, s, moved=True) for s in range(2)] for e in range(N)]
        err = [dt.element_errors(fx, out, fam, e, ref[e], None if moved is None else moved[e]) for e in range(N)]
        for m in dt.state_metrics(fam):
            out["%s_err_%s" % (fam, m)] = np.array([[err[e][m][s] for e in range(N)] for s in range(2)])
        for m in ("load", "mass"):
            out["%s_err_%s" % (fam, m)] = np.array([err[e][m] for e in range(N)])
        for s in range(2):
            print("%s %-6s " % (fam, dt.STATES[s]) + "  ".join("%s %.1e" % (m, out["%s_err_%s" % (fam, m)][s].max()) for m in dt.state_metrics(fam))
                  + ("  spurious %d, exact zeros %d" % (sum(err[e]["spurious"][s] for e in range(N)), out[fam + "_zero"][s].sum())
                     if fam in dt.FLAT else ""))
        print("%s        load %.1e  mass %.1e" % (fam, out[fam + "_err_load"].max(), out[fam + "_err_mass"].max()))
        for m in dt.CONDITIONED:
            bad = np.argwhere(out["%s_err_%s" % (fam, m)] > dt.CONDITION)
            assert len(bad) == 0, (fam, m, bad.tolist(), out["%s_err_%s" % (fam, m)])
    save_npz(dt.FIXTURE, out)
    print(dt.FIXTURE, os.path.getsize(dt.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
