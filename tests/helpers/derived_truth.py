"""The derived element quantities -- stress resultants (femshell_element_resultants), the geometric stiffness coefficients g_ab
(femshell_geometric_product), the nodal shares of element loads (femshell_element_load_vector) and the lumped nodal masses
(femshell_lumped_mass) -- against an extended-precision truth: the fixture tests/golden/derived_truth.npz (written by
tools/gen_golden_derived_truth.py) and the metrics that are applied alike to the FP64 reference (by the generator and
tests/test_derived_truth_cpu.py) and to the device (tests/test_gpu_derived_truth.py).

The truth is the numpy reference of these four quantities (tests/helpers/resultants.py, buckling.py, element_loads.py, dynamics.py;
DESIGN.md 8d, 8g) evaluated with dtype=np.longdouble from the double inputs, nothing rounded to double on the way (restated: the
triangle's frame and Specht's B~ restated in numpy, the frame's products carrying their rounding errors; a quadrilateral's
coordinates taken relative to its first node before they are projected on its frame), and rounded once to double at the end.  The FP64 reference is the same code with
dtype=np.float64: its distance from the truth is the reference's own error, and the device is held to truth.bound of it.

The elements and materials are those of tests/golden/element_truth.npz (tests/helpers/truth.py): the two fixtures describe the same
shapes.  Per family F and element e = 0..7 the fixture holds, for the two displacement states STATES (axis 0 where there are two):
  F_u (2, 8, nn, 6)            the displacements; F_u_moved on T1 and Q1: (Q u_t, Q u_r) for the moved copy F_xyz_moved
  F_load (8, 4), F_rho (8,)    the element-load row (p, qx, qy, qz) and the density (one per distinct material)
  F_res (2, 8, 14)             truth: N[0:6], M[6:12] in global axes, the two von Mises values
  F_g (2, 8, 6 | 10)           truth: upper triangle of g
  F_share (8, nn, 3), F_mass (8, nn, 6)     truth: what every node gets of the element's load and mass
  F_zero (2, 8, 12)            T2 T3 Q2 Q4: entries of N, M that are exactly zero in the truth and in the FP64 reference
  F_err_<metric> (2, 8) or (8,)             the FP64 reference's error against the truth
"""
import os

import numpy as np

from tests.helpers import buckling as bk, dynamics as dy, element_loads as el, resultants as rs, truth
from tests.helpers.meshes import GOLDEN

FIXTURE = os.path.join(GOLDEN, "derived_truth.npz")
LD = np.longdouble
STATES = ("random", "smooth")
FLAT = truth.CLASSWISE
# every stored (element, state): FP64 reference within this of the truth in N, M, vm and g (beyond it an entry tests nothing but
# conditioning)
CONDITION = 1e-9
CONDITIONED = ("N", "M", "vm", "g")
PATHS = (False, True)  # sections: none; one section equal to the context's material.  "own": truth.OWN_FAMILIES, see truth.PATHS
MIXED_METRICS = ("N", "M", "vm", "g", "load", "mass")


def long_double_is_extended():
    return np.finfo(LD).nmant >= 63


def state_metrics(fam):
    return ["N", "M", "vm", "plane", "g", "g_rows"] + (["frame"] if fam in truth.FRAME else [])


def metrics_of(fam):
    return state_metrics(fam) + ["load", "mass"]


def path_id(sectioned):
    return "own" if sectioned == "own" else ("sections" if sectioned else "plain")


def load():
    return np.load(FIXTURE)


# ------------------------------------------------------------------ the reference, in one type

def evaluate(xyz, u, material, flags, load_row, rho, dtype):
    """One element with nodes of its own through the numpy reference, every intermediate in `dtype`, the results rounded once to
    double: dict res (14,), g (nn, nn), share (nn, 3), mass (nn, 6)"""
    xyz = np.asarray(xyz, dtype=np.float64)
    nn = len(xyz)
    nu, E, t = material
    conn = np.arange(nn, dtype=np.int32)[None]
    tri, quad = (conn, None) if nn == 3 else (None, conn)
    # the FP64 evaluation is a plain one (its error is what the device may have four times over); the truth keeps its digits on
    # slivers by carrying the rounding errors of the frame's products along (rs.tri3_operators)
    restated = True if dtype is np.float64 else "twofold"
    res, _ = rs.element_resultants(xyz, u, nu, E, t, flags=flags, dtype=dtype, restated=restated)
    g = bk.element_coefficients(xyz, tri, quad, u, nu, E, t, flags=flags, dtype=dtype, restated=restated)[0][1]
    share = el.element_shares(xyz, conn, np.asarray(load_row, dtype=np.float64)[None], work=dtype)[0]
    mass = dy.lumped_mass(xyz, tri, quad, rho, t, dtype=dtype)
    return {"res": res, "g": np.asarray(g).astype(np.float64), "share": np.tile(np.asarray(share).astype(np.float64), (nn, 1)),
            "mass": np.asarray(mass).astype(np.float64)}


def reference(fx, dx, fam, e, state, dtype=np.float64, moved=False):
    """element e of the family in displacement state `state` (index into STATES) through evaluate(); moved: its moved copy"""
    nu, E, t, flags = truth.material_of(fx, fam, e)
    xyz = fx[fam + ("_xyz_moved" if moved else "_xyz")][e]
    u = dx[fam + ("_u_moved" if moved else "_u")][state][e]
    return evaluate(xyz, u, (nu, E, t), flags, dx[fam + "_load"][e], float(dx[fam + "_rho"][e]), dtype)


def truth_of(dx, fam, e, state):
    nn = truth.nodes_of(fam)
    return {"res": dx[fam + "_res"][state][e], "g": truth.full(dx[fam + "_g"][state][e], nn), "share": dx[fam + "_share"][e],
            "mass": dx[fam + "_mass"][e]}


# ------------------------------------------------------------------ the metrics

def tensor(v6):
    A = np.zeros((3, 3))
    for v, (p, q) in zip(v6, rs.VOIGT):
        A[p, q] = A[q, p] = v
    return A


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


def state_errors(result, tr, ez, zero=None):
    """Errors of one element's resultants and g (result: dict res, g) against the truth tr in one displacement state: dict over
    state_metrics (without "frame"), and "spurious" where `zero` (12,) marks the entries of N, M that must be exactly zero.
    ez: the element's normal, from tests/golden/element_truth.npz (binary128, rounded once)."""
    res, g = np.asarray(result["res"], dtype=np.float64), np.asarray(result["g"], dtype=np.float64)
    N, M = tensor(res[:6]), tensor(res[6:12])
    out = {"N": _rel(res[:6], tr["res"][:6]), "M": _rel(res[6:12], tr["res"][6:12]),
           "vm": float(np.max(np.abs(res[12:] - tr["res"][12:]) / np.abs(tr["res"][12:]))),
           "plane": float(max(np.linalg.norm(N @ ez) / np.linalg.norm(N), np.linalg.norm(M @ ez) / np.linalg.norm(M))),
           "g": _rel(g, tr["g"]),
           "g_rows": float(np.linalg.norm(g.sum(axis=1)) / np.linalg.norm(g))}
    if zero is not None:
        out["spurious"] = int(np.count_nonzero(res[:12][np.asarray(zero, dtype=bool)]))
    return out


def frame_defect(res_moved, res, Q):
    """the larger of || A(moved) - Q A Q^T || / || A || for A = N, M: what moving the element rigidly (and its displacements with
    it) does to its resultants beyond rotating them.  Needs no formula of the reference's."""
    worst = 0.0
    for k in (0, 6):
        A, Am = tensor(res[k:k + 6]), tensor(res_moved[k:k + 6])
        worst = max(worst, float(np.linalg.norm(Am - Q @ A @ Q.T) / np.linalg.norm(A)))
    return worst


def once_errors(result, tr):
    """load: 2-norm relative error of the element's nodal shares; mass: the same, the translational and the rotational masses
    each on their own scale (they differ by t^2 / 12), the larger of the two"""
    share, mass = np.asarray(result["share"], dtype=np.float64), np.asarray(result["mass"], dtype=np.float64)
    return {"load": _rel(share, tr["share"]),
            "mass": max(_rel(mass[:, :3], tr["mass"][:, :3]), _rel(mass[:, 3:], tr["mass"][:, 3:]))}


def element_errors(fx, dx, fam, e, results, moved=None):
    """metric -> per-state list (state metrics, "spurious") or number (load, mass) for element e of the family; results: per state
    the dict of evaluate() (share and mass are read from state 0), moved: the same for the moved copy (T1, Q1; None: no "frame")"""
    ez = fx[fam + "_trafo"][e][2]
    out = {m: [] for m in state_metrics(fam) + (["spurious"] if fam in FLAT else []) if m != "frame" or moved is not None}
    for s in range(len(STATES)):
        err = state_errors(results[s], truth_of(dx, fam, e, s), ez, dx[fam + "_zero"][s][e] if fam in FLAT else None)
        if moved is not None:
            err["frame"] = frame_defect(moved[s]["res"], results[s]["res"], fx[fam + "_Q"][e])
        for m in out:
            out[m].append(err[m])
    out.update(once_errors(results[0], truth_of(dx, fam, e, 0)))
    return out


def family_worst(fx, dx, fam, results, moved=None, elements=None):
    """metric -> (2,) worst per state over the elements (state metrics, "spurious") or number (load, mass); results[k][s] is the
    dict of element elements[k] in state s (or a list of such dicts: every copy of the element is held to the bound)"""
    elements = list(range(truth.PER_FAMILY)) if elements is None else list(elements)
    worst = {}
    for k, e in enumerate(elements):
        copies = results[k] if isinstance(results[k][0], (list, tuple)) else [results[k]]
        copies_moved = [None] * len(copies) if moved is None else (moved[k] if isinstance(moved[k][0], (list, tuple)) else [moved[k]])
        for r, rm in zip(copies, copies_moved):
            for m, v in element_errors(fx, dx, fam, e, r, rm).items():
                worst[m] = np.maximum(worst[m], v) if m in worst else np.array(v, dtype=np.float64)
    return worst


def reference_worst(dx, fam, m, state=None):
    v = dx["%s_err_%s" % (fam, m)]
    return float((v if state is None or v.ndim == 1 else v[state]).max())


def check(dx, fam, worst, factors=None, metrics=None):
    """[(metric, state, worst, reference's worst, bound)] of the metrics over their bound, per state; "spurious" must be 0"""
    bad = []
    for m in (metrics_of(fam) if metrics is None else metrics):
        per_state = np.ndim(worst[m]) > 0
        for s in (range(len(STATES)) if per_state else [None]):
            w = float(worst[m][s]) if per_state else float(worst[m])
            o = reference_worst(dx, fam, m, s)
            b = truth.bound(o, (factors or {}).get(m, 4.0))
            if not w <= b:
                bad.append((m, STATES[s] if per_state else "-", w, o, b))
    if "spurious" in worst and np.any(worst["spurious"]):
        bad.append(("spurious", "-", int(np.max(worst["spurious"])), 0, 0))
    return bad


def report(dx, fam, label, worst, metrics=None):
    lines = []
    for m in (metrics_of(fam) if metrics is None else metrics):
        per_state = np.ndim(worst[m]) > 0
        for s in (range(len(STATES)) if per_state else [None]):
            lines.append("%s %s %s %s: device %.2e (reference %.2e)" % (fam, label, STATES[s] if per_state else "-", m,
                                                                       float(worst[m][s]) if per_state else float(worst[m]),
                                                                       reference_worst(dx, fam, m, s)))
    return "\n".join(lines)


# ------------------------------------------------------------------ the device's values

def device_results(pkg, material, members, sectioned, fx, dx, reached=None):
    """`members`: (family, element, moved) triples, triangles and quadrilaterals in any mix, as one mesh in which every element has
    nodes of its own, repeated to at least truth.MIN_ELEMENTS elements, under a context of `material` = (nu, E, t, flags).
    sectioned: False; True: one section equal to the context's material; "own": every element a section of its own material and
    density.  Returns per member the list over its copies of the per-state list of dicts res, g, share, mass (as evaluate() gives
    them).  All read-outs are exact: a resultant row per element; g_ab = Y[column b, node a, d] of the geometric product with
    "translation d of local node b of every element = 1" (one product with 1.0 plus exact zeros), read from all three
    translations, which must agree bit for bit, with rotational rows that are exactly zero; a node's load share and mass from the
    one element that contains it.  reached: a list that gets (the mesh has quadrilaterals, sections are set)."""
    nu, E, t, flags = material
    tris = [m for m in members if m[0][0] == "T"]
    quads = [m for m in members if m[0][0] == "Q"]
    order = tris + quads
    nt, nq = len(tris), len(quads)
    reps = -(-truth.MIN_ELEMENTS // (nt + nq))

    def xyz_of(m):
        return fx[m[0] + ("_xyz_moved" if m[2] else "_xyz")][m[1]]

    def u_of(m, s):
        return dx[m[0] + ("_u_moved" if m[2] else "_u")][s][m[1]]

    xyz, tri, quad = truth.isolated_mesh([xyz_of(m) for m in tris] or None, [xyz_of(m) for m in quads] or None, reps)
    conn = list(tri) + list(quad)
    n = len(xyz)
    assert len(conn) >= truth.MIN_ELEMENTS
    if reached is not None:
        reached.append((nq > 0, bool(sectioned)))
    fs = pkg.FemShell(nu, E, t, flags=flags)
    fs.set_mesh(xyz, tri, quad)
    mats = [truth.material_of(fx, f, e)[:3] for f, e, _ in order]
    rhos = [float(dx[f + "_rho"][e]) for f, e, _ in order]
    if sectioned == "own":
        table, index = truth.section_table(mats)
        assert len(table) > 1 and all(table[:, k].tolist().count(material[k]) == 0 for k in range(3)), "the context's material is an element's"
        fs.set_sections(table, np.tile(index[:nt], reps), np.tile(index[nt:], reps))
        sec_rho = np.zeros(len(table))
        for i, r in zip(index, rhos):
            assert sec_rho[i] in (0.0, r), "one density per material"
            sec_rho[i] = r
        assert len(set(sec_rho)) == len(sec_rho) and 1.0 not in sec_rho
        fs.set_density(1.0, section_rho=sec_rho)
    else:
        assert all(m == (nu, E, t) for m in mats) and len(set(rhos)) == 1, "one material per context"
        if sectioned:
            fs.set_sections([[nu, E, t]], np.zeros(len(tri), np.int32), np.zeros(len(quad), np.int32))
            fs.set_density(1.0, section_rho=[rhos[0]])
        else:
            fs.set_density(rhos[0])
    # copy r of triangle k is triangle r * nt + k, and likewise for the quadrilaterals
    member_of = [k for _ in range(reps) for k in range(nt)] + [nt + k for _ in range(reps) for k in range(nq)]  # -> index into `order`

    loads = np.array([dx[order[k][0] + "_load"][order[k][1]] for k in member_of]).reshape(-1, 4)
    fs.set_element_loads(loads[:len(tri)] if nt else None, loads[len(tri):] if nq else None)
    S = fs.element_load_vector()
    mass = fs.lumped_mass()
    assert not S[:, 3:].any(), "element loads on a rotation"

    out = [[[None] * len(STATES) for _ in range(reps)] for _ in order]
    seen = [0] * len(order)
    copy_of = []
    for k in member_of:
        copy_of.append(seen[k])
        seen[k] += 1
    nn_max = 4 if nq else 3
    for s in range(len(STATES)):
        u = np.zeros((n, 6))
        for c, k in zip(conn, member_of):
            u[c] = u_of(order[k], s)
        res = fs.element_resultants(u)
        assert res.shape == (len(conn), 14)
        G = None
        for d in range(3):
            X = np.stack([truth.probe_vector(n, conn, b, d) for b in range(nn_max)])
            Y = fs.geometric_product(u, X).reshape(nn_max, n, 6)
            assert not Y[:, :, 3:].any(), "geometric stiffness on a rotation"
            other = [q for q in range(3) if q != d]
            assert not Y[:, :, other].any(), "geometric stiffness couples two directions"
            if G is None:
                G = Y[:, :, d].copy()
            else:
                np.testing.assert_array_equal(Y[:, :, d], G, err_msg="g read from translation %d differs from translation 0" % d)
        for i, (c, k) in enumerate(zip(conn, member_of)):
            nn = len(c)
            g = np.array([[G[b, c[a]] for b in range(nn)] for a in range(nn)])
            out[k][copy_of[i]][s] = {"res": res[i], "g": g, "share": S[c, :3], "mass": mass[c]}
    fs.close()
    return {m: out[k] for k, m in enumerate(order)}


def device_family_worst(pkg, fx, dx, fam, sectioned, reached=None):
    """metric -> the device's worst error over the family (all copies of every element) through one path, context by context;
    on T1 and Q1 the moved copies ride in the same mesh"""
    own = sectioned == "own"
    results, moved, elements = [], [], []
    for material, els in truth.groups_of(fx, fam, None, own).items():
        members = [(fam, e, False) for e in els] + ([(fam, e, True) for e in els] if fam in truth.FRAME else [])
        got = device_results(pkg, material, members, sectioned, fx, dx, reached)
        for e in els:
            elements.append(e)
            results.append(got[(fam, e, False)])
            if fam in truth.FRAME:
                moved.append(got[(fam, e, True)])
    return family_worst(fx, dx, fam, results, moved if fam in truth.FRAME else None, elements)
