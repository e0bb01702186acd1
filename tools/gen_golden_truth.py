#!/usr/bin/env python3
"""Writes tests/golden/element_truth.npz: element stiffness matrices of 13 families of 8 elements each, evaluated by the
quad-precision build of the oracle's element path (oracle/femshell_oracle_quad.c, __float128) and rounded once to double,
with the FP64 oracle's own distance from them per metric (tests/helpers/truth.py).  The device is held to a small multiple
of that distance (tests/test_gpu_element_truth.py); tests/test_element_truth_cpu.py checks that this file is what the
quad build computes here.  Fixed seeds: running this again reproduces the file bit for bit.

Per family F (T1..T7 triangles, Q1..Q6 quadrilaterals), e = 0..7:
  F_xyz (8, nodes, 3), F_mat (8, 4: nu, E, t, flags)       the inputs
  F_K (8, 171 | 300)                                        quad K, global axes, node-major, upper triangle
  F_trafo (8, 3, 3)                                         quad frame, rows = local axes
  F_err_<metric> (8,)                                       the FP64 oracle's error against quad
  F_normal (8,)           T2 T3 Q2 Q4: the global axis the flat element is normal to
  F_Q, F_c, F_xyz_moved   T1 Q1: a rotation, a shift and Q X + c as the double inputs of the moved element
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import oracle, oracle_quad, truth  # noqa: E402

N = truth.PER_FAMILY
NU, E, T, _ = truth.DEFAULT_MATERIAL
ALL_FLAGS = [3.0, 2.0, 1.0, 0.0] * 2


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def direction(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def default_mat(n=N):
    return np.tile([NU, E, T, 3.0], (n, 1))


def embed(p2, plane, offset):
    """2-D points into the coordinate plane xy / yz / zx (plane 0 / 1 / 2: normal z / x / y), the third coordinate the same
    number for every node: in-plane axes (a, b) in cyclic order, so that a positive 2-D orientation has the normal +axis"""
    a, b, n = [(0, 1, 2), (1, 2, 0), (2, 0, 1)][plane]
    X = np.zeros((len(p2), 3))
    X[:, a], X[:, b], X[:, n] = p2[:, 0], p2[:, 1], offset
    return X, n


def flat_triangle(rng, aligned=False, sign=1.0, orient=1.0):
    """unit-size triangle in 2-D; aligned: first edge exactly along +-x (the frame's entries are exactly 0 and +-1)"""
    p0 = rng.uniform(-1.0, 1.0, size=2)
    ln = rng.uniform(0.6, 1.5)
    if aligned:
        U = np.array([sign * ln, 0.0])
    else:
        a = rng.uniform(0.2, 1.3) + rng.integers(0, 4) * np.pi / 2
        U = ln * np.array([np.cos(a), np.sin(a)])
    perp = np.array([-U[1], U[0]]) * orient
    return np.stack([p0, p0 + U, p0 + rng.uniform(-0.3, 1.3) * U + rng.uniform(0.4, 1.2) * perp])


def flat_quad(rng, aligned=False, orient=1.0):
    """unit-size convex quadrilateral in 2-D; aligned: a rectangle with sides along the axes"""
    base = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float64)
    if aligned:
        base = base * rng.uniform(0.6, 1.5, size=2)
    else:
        base += rng.uniform(-0.25, 0.25, size=(4, 2))
        a = rng.uniform(0.2, 1.3)
        base = base @ np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
    base = base + rng.uniform(-1.0, 1.0, size=2)
    return base if orient > 0 else base[::-1].copy()


def place(rng, p2, shift_scale=1.0, shift=None):
    """2-D (or 3-D) points, randomly rotated and shifted"""
    X = np.c_[p2, np.zeros(len(p2))] if p2.shape[1] == 2 else p2
    c = rng.normal(size=3) * shift_scale if shift is None else shift
    return X @ rotation(rng).T + c


# ------------------------------------------------------------------ triangles

def family_T1(rng):  # generic: random in 3-D, size factor 0.1 .. 10
    xyz = np.stack([rng.normal(size=(3, 3)) * rng.uniform(0.1, 10.0) for _ in range(N)])
    mat = default_mat()
    mat[:, 3] = ALL_FLAGS
    return xyz, mat, {}


def family_T2(rng):  # coordinate planes xy, yz, zx, both orientations, half with the first edge along +- an axis
    xyz, normal = [], []
    for k in range(N):
        tri2 = flat_triangle(rng, aligned=(k // 2) % 2 == 0, sign=1.0 if k in (0, 5) else -1.0, orient=1.0 if k % 2 == 0 else -1.0)
        X, n = embed(tri2, k % 3, rng.uniform(-1.0, 1.0))
        xyz.append(X)
        normal.append(n)
    mat = default_mat()
    mat[:, 3] = ALL_FLAGS
    return np.stack(xyz), mat, {"normal": np.array(normal, dtype=np.int8)}


def family_T3(rng):  # thin and flat: in the xy plane, unit size, t/h = 1e-1, 1e-3, 1e-5
    xyz = np.stack([embed(flat_triangle(rng), 0, 0.0 if k % 2 else rng.uniform(-1.0, 1.0))[0] for k in range(N)])
    mat = default_mat()
    mat[:, 2] = [1e-1, 1e-3, 1e-5, 1e-1, 1e-3, 1e-5, 1e-3, 1e-5]
    return xyz, mat, {"normal": np.full(N, 2, dtype=np.int8)}


def family_T4(rng):  # slivers: caps of height 1e-1 .. 1e-4 over a unit base, needles of width 1e-2 and 1e-4
    xyz = []
    for h in (1e-1, 1e-2, 1e-3, 1e-4):
        xyz.append(np.array([[0, 0], [1, 0], [rng.uniform(0.3, 0.7), h]]))
    for w in (1e-2, 1e-4, 1e-2, 1e-4):
        xyz.append(np.array([[0, 0], [w, 0], [w * rng.uniform(0.2, 0.8), 1.0]]))
    xyz = np.stack([place(rng, p)[rng.permutation(3)] for p in xyz])
    return xyz, default_mat(), {}


def family_T5(rng):  # far from the origin: unit size at distance 1e2, 1e4, 1e6, 1e8
    xyz = np.stack([place(rng, flat_triangle(rng), shift=D * direction(rng)) for D in (1e2, 1e4, 1e6, 1e8) * 2])
    return xyz, default_mat(), {}


def family_T6(rng):  # Poisson's ratio 0, 0.499, 0.4999999
    xyz = np.stack([rng.normal(size=(3, 3)) * rng.uniform(0.5, 2.0) for _ in range(N)])
    mat = default_mat()
    mat[:, 0] = [0.0, 0.499, 0.4999999, 0.0, 0.499, 0.4999999, 0.499, 0.4999999]
    return xyz, mat, {}


def family_T7(rng):  # units: size 1e-4 with E 1e11, size 1e4 with E 1e-3
    xyz, mat = [], default_mat()
    for k in range(N):
        size, mat[k, 1] = (1e-4, 1e11) if k % 2 == 0 else (1e4, 1e-3)
        xyz.append(rng.normal(size=(3, 3)) * size)
    return np.stack(xyz), mat, {}


# ------------------------------------------------------------------ quadrilaterals

def family_Q1(rng):  # generic: planar, convex, random size, orientation and place (tests.test_gpu_parity.random_quads)
    xyz = []
    for _ in range(N):
        base = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float64) + rng.uniform(-0.25, 0.25, size=(4, 2))
        xyz.append(place(rng, base * rng.uniform(0.2, 5.0), shift_scale=3.0))
    mat = default_mat()
    mat[:, 3] = ALL_FLAGS
    return np.stack(xyz), mat, {}


def family_Q2(rng):  # coordinate planes, both orientations, half of them rectangles along the axes
    xyz, normal = [], []
    for k in range(N):
        X, n = embed(flat_quad(rng, aligned=(k // 2) % 2 == 0, orient=1.0 if k % 2 == 0 else -1.0), k % 3, rng.uniform(-1.0, 1.0))
        xyz.append(X)
        normal.append(n)
    return np.stack(xyz), default_mat(), {"normal": np.array(normal, dtype=np.int8)}


def family_Q3(rng):  # far from the origin: unit size at distance 1e2, 1e4, 1e6
    xyz = np.stack([place(rng, flat_quad(rng), shift=D * direction(rng)) for D in (1e2, 1e2, 1e4, 1e4, 1e4, 1e6, 1e6, 1e6)])
    return xyz, default_mat(), {}


def family_Q4(rng):  # thin and flat: in the xy plane, unit size
    xyz = np.stack([embed(flat_quad(rng), 0, 0.0 if k % 2 else rng.uniform(-1.0, 1.0))[0] for k in range(N)])
    mat = default_mat()
    mat[:, 2] = [1e-1, 1e-3, 1e-5, 1e-1, 1e-3, 1e-5, 1e-3, 1e-5]
    return xyz, mat, {"normal": np.full(N, 2, dtype=np.int8)}


def family_Q5(rng):  # distorted: rhombi with a corner angle near 20 degrees, trapezoids with parallel sides 5 : 1
    xyz = []
    for k in range(N):
        if k % 2 == 0:
            a = np.radians(20.0 + rng.uniform(-2.0, 2.0))
            p = np.array([[0, 0], [1, 0], [1 + np.cos(a), np.sin(a)], [np.cos(a), np.sin(a)]])
        else:
            o = rng.uniform(0.0, 4.0)
            p = np.array([[0, 0], [5, 0], [o + 1, 2.0], [o, 2.0]]) / 3.0
        xyz.append(place(rng, np.roll(p, k // 2, axis=0)))
    return np.stack(xyz), default_mat(), {}


def family_Q6(rng):  # warped: corners lifted by +-0.01 and +-0.1 of the side, alternately up and down
    xyz = []
    for k in range(N):
        p = np.c_[flat_quad(rng), (0.01 if k % 2 == 0 else 0.1) * np.array([1.0, -1.0, 1.0, -1.0])]
        xyz.append(place(rng, p))
    return np.stack(xyz), default_mat(), {}


def main():
    out = {}
    for idx, fam in enumerate(truth.FAMILIES):
        rng = np.random.default_rng(20260000 + idx)
        xyz, mat, extra = globals()["family_" + fam](rng)
        nodes = truth.nodes_of(fam)
        assert xyz.shape == (N, nodes, 3) and mat.shape == (N, 4)
        quad_el = oracle_quad.element_tri3 if nodes == 3 else oracle_quad.element_quad4
        fp64_el = oracle.element_tri3 if nodes == 3 else oracle.element_quad4
        mats = [oracle.material(*m[:3], int(m[3])) for m in mat]
        parts = [quad_el(xyz[e], mats[e])[1] for e in range(N)]
        out[fam + "_xyz"], out[fam + "_mat"] = xyz, mat
        out[fam + "_K"] = np.stack([truth.upper(p["K_global_nm"]) for p in parts])
        out[fam + "_trafo"] = np.stack([p["trafo"] for p in parts])
        for k, v in extra.items():
            out[fam + "_" + k] = v
        K64 = [fp64_el(xyz[e], mats[e], want_parts=True)[1]["K_global_nm"] for e in range(N)]
        moved = None
        if fam in truth.FRAME:
            Q = np.stack([rotation(rng) for _ in range(N)])
            c = rng.normal(size=(N, 3)) * 2.0
            out[fam + "_Q"], out[fam + "_c"] = Q, c
            out[fam + "_xyz_moved"] = np.stack([xyz[e] @ Q[e].T + c[e] for e in range(N)])
            moved = [fp64_el(out[fam + "_xyz_moved"][e], mats[e], want_parts=True)[1]["K_global_nm"] for e in range(N)]
        err = truth.family_errors(out, fam, K64, moved)
        for m in truth.metrics_of(fam):
            out["%s_err_%s" % (fam, m)] = err[m]
        print("%s  " % fam + "  ".join("%s %.1e" % (m, err[m].max()) for m in truth.metrics_of(fam))
              + ("  spurious %d" % err["spurious"].sum() if "spurious" in err else ""))
        assert err["whole"].max() <= truth.FAMILY_CONDITION, (fam, err["whole"])
    np.savez(truth.FIXTURE, **out)
    print(truth.FIXTURE, os.path.getsize(truth.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
