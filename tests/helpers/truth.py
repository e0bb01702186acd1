"""Element stiffness against a quad-precision truth: the fixture tests/golden/element_truth.npz (written by
tools/gen_golden_truth.py from oracle/libfemshell_oracle_quad.so) and the metrics that are applied alike to the FP64
oracle (by the generator and tests/test_element_truth_cpu.py) and to the device (tests/test_gpu_element_truth.py).

All matrices here are node-major, (6 nodes) x (6 nodes), in global axes: entry (6 i + a, 6 j + b) couples dof a of node i
with dof b of node j, dofs (u, v, w, rx, ry, rz).  The fixture keeps upper triangles.
"""
import os

import numpy as np

from tests.helpers.meshes import GOLDEN

FIXTURE = os.path.join(GOLDEN, "element_truth.npz")
EPS = 2.0 ** -52
PER_FAMILY = 8
TRI_FAMILIES = ["T1", "T2", "T3", "T4", "T5", "T6", "T7"]
QUAD_FAMILIES = ["Q1", "Q2", "Q3", "Q4", "Q5", "Q6"]
FAMILIES = TRI_FAMILIES + QUAD_FAMILIES
CLASSWISE = ("T2", "T3", "Q2", "Q4")  # flat elements in a coordinate plane: the dof classes occupy disjoint entries of K
FRAME = ("T1", "Q1")                  # a second copy of every element, rotated and shifted
DEFAULT_MATERIAL = (0.3, 2.1e5, 0.37, 3.0)
# every stored element: FP64 oracle within this of quad, whole matrix (an element beyond it tests nothing but conditioning)
FAMILY_CONDITION = 1e-9


def nodes_of(fam):
    return 3 if fam[0] == "T" else 4


def metrics_of(fam):
    m = ["whole", "symmetry", "translation"]
    if fam in CLASSWISE:
        m += ["membrane", "bending", "drilling"]
    if fam in FRAME:
        m += ["frame"]
    return m


def bound(oracle_worst, factor=4.0):
    """The device's worst error over a family may be `factor` times the FP64 oracle's own worst distance from quad (two
    FP64 evaluations of one set of formulas in different orders, the device's with rsqrt and contraction: more than two
    bits lost against the reference's own error means a formulation that loses digits the reference keeps), and never
    needs to be below 16 eps = 3.6e-15, the recorded agreement of two FP64 assemblies (2e-15) as a power of two."""
    return max(factor * oracle_worst, 16.0 * EPS)


def upper(K):
    return K[np.triu_indices(K.shape[0])]


def full(u, n):
    K = np.zeros((n, n))
    K[np.triu_indices(n)] = u
    return K + np.triu(K, 1).T


def to_node_major(Ke, nodes):
    """variable-major (nodes * a + i) element matrix, as femshell_element_matrices and the oracle return it -> node-major"""
    p = np.array([nodes * a + i for i in range(nodes) for a in range(6)])
    return Ke[np.ix_(p, p)]


def class_masks(nodes, normal):
    """Boolean (6 nodes)^2 masks of the membrane, bending and drilling entries of a flat element whose normal is the
    global axis `normal`, and of the entries that couple two classes (structurally zero)."""
    cls = np.zeros(6, dtype=int)          # 0 membrane: the two in-plane translations
    cls[normal] = 1                       # 1 bending: the translation along the normal and the two in-plane rotations
    cls[3:] = 1
    cls[3 + normal] = 2                   # 2 drilling: the rotation about the normal
    c = np.tile(cls, nodes)
    same = c[:, None] == c[None, :]
    out = {name: same & (c[:, None] == k) for k, name in enumerate(("membrane", "bending", "drilling"))}
    out["cross"] = ~same
    return out


def element_errors(K, truth, normal=None):
    """Errors of one element matrix K against its truth: a dict over metrics_of (without "frame"), and "spurious", the number
    of entries that are exactly zero in the truth and not in K (asserted to be 0 where the classes are disjoint)."""
    nodes = K.shape[0] // 6
    nt = np.linalg.norm(truth)
    out = {"whole": np.linalg.norm(K - truth) / nt,
           "symmetry": np.linalg.norm(K - K.T) / np.linalg.norm(K)}
    worst = 0.0
    for d in range(3):  # the same translation of every node: no force (against K's own norm)
        v = np.zeros(6 * nodes)
        v[d::6] = 1.0
        worst = max(worst, np.linalg.norm(K @ v) / np.linalg.norm(K))
    out["translation"] = worst
    if normal is not None:
        masks = class_masks(nodes, int(normal))
        for name in ("membrane", "bending", "drilling"):
            m = masks[name]
            out[name] = np.linalg.norm((K - truth)[m]) / np.linalg.norm(truth[m])
        out["spurious"] = int(np.count_nonzero(K[truth == 0.0]))
    return out


def frame_defect(K_moved, K, Q):
    """|| K(Q X + c) - (Q x) K(X) (Q x)^T || / || K(X) ||: what moving the element rigidly does to its matrix, beyond
    rotating it.  Needs no formula of the oracle's."""
    nodes = K.shape[0] // 6
    R = np.kron(np.eye(2 * nodes), Q)
    return np.linalg.norm(K_moved - R @ K @ R.T) / np.linalg.norm(K)


def load():
    return np.load(FIXTURE)


def material_of(fx, fam, e):
    nu, E, t, flags = fx[fam + "_mat"][e]
    return float(nu), float(E), float(t), int(flags)


def truth_of(fx, fam, e):
    return full(fx[fam + "_K"][e], 6 * nodes_of(fam))


def family_errors(fx, fam, K, K_moved=None, elements=None):
    """Per-element errors of the matrices K[e] (node-major) of a family: dict metric -> array over `elements` (all)."""
    elements = range(PER_FAMILY) if elements is None else elements
    names = metrics_of(fam) + (["spurious"] if fam in CLASSWISE else [])
    out = {m: [] for m in names}
    for k, e in enumerate(elements):
        normal = fx[fam + "_normal"][e] if fam in CLASSWISE else None
        err = element_errors(K[k], truth_of(fx, fam, e), normal)
        if fam in FRAME:
            err["frame"] = frame_defect(K_moved[k], K[k], fx[fam + "_Q"][e])
        for m in names:
            out[m].append(err[m])
    return {m: np.array(v) for m, v in out.items()}


# ------------------------------------------------------------------ the device's matrices

KERNELS = {"k_assemble": "0", "k_assemble_pipe": "2"}  # FEMSHELL_ASM_PIPE: 0 two-phase, 2 pipelined wherever it can run
PRODUCT = "k_element_product"  # the matrix-free product (reactions, prescribed right-hand side): neither variable reaches it
# (kernel, FEMSHELL_SYMMETRIC, sections): sections False: none; True: one section equal to the context's material; "own": every
# element has a section with its own material, under a context whose material (OWN_CONTEXT) is none of theirs
PATHS = ([("k_element_matrices", None, False)] + [(k, s, sec) for sec in (False, True) for k in KERNELS for s in ("1", "0")]
         + [(PRODUCT, None, False), (PRODUCT, None, True)])
OWN_PATHS = [("k_element_matrices", None, "own")] + [(k, s, "own") for k in KERNELS for s in ("1", "0")] + [(PRODUCT, None, "own")]
OWN_FAMILIES = ("T3", "T6", "T7", "Q4")  # more than one material under one value of the flags
OWN_CONTEXT = (0.25, 1.0, 1.0)  # (nu, E, t) of an "own" context: no element of the fixture has this nu, this E or this t
MIN_ELEMENTS = 40  # a group is repeated up to this many elements: more than one slice of 32 nodes, lanes beyond the first


def path_id(path):
    kernel, symmetric, sectioned = path
    return (kernel + ("" if symmetric is None else ("-sym" if symmetric == "1" else "-full"))
            + ("-own" if sectioned == "own" else ("-sections" if sectioned else "")))


def groups_of(fx, fam, elements=None, own=False):
    """The family's elements by (nu, E, t, flags): a context has one material and one set of flags.  own: by the flags alone,
    under the material OWN_CONTEXT (the elements bring their materials along as sections)."""
    out = {}
    for e in (range(PER_FAMILY) if elements is None else elements):
        m = material_of(fx, fam, e)
        out.setdefault(OWN_CONTEXT + m[3:] if own else m, []).append(e)
    return out


def isolated_mesh(tri_xyz=None, quad_xyz=None, reps=1):
    """(xyz, tri, quad) of `reps` copies of the triangles tri_xyz (m, 3, 3) and quadrilaterals quad_xyz (m, 4, 3), every element
    with nodes of its own; copy r of triangle k is triangle r * m + k, and likewise for the quadrilaterals."""
    tri_xyz = np.zeros((0, 3, 3)) if tri_xyz is None else np.asarray(tri_xyz, dtype=np.float64).reshape(-1, 3, 3)
    quad_xyz = np.zeros((0, 4, 3)) if quad_xyz is None else np.asarray(quad_xyz, dtype=np.float64).reshape(-1, 4, 3)
    nt, nq = len(tri_xyz), len(quad_xyz)
    xyz = np.concatenate([np.tile(tri_xyz, (reps, 1, 1)).reshape(-1, 3), np.tile(quad_xyz, (reps, 1, 1)).reshape(-1, 3)])
    tri = np.arange(3 * nt * reps, dtype=np.int32).reshape(-1, 3)
    quad = (3 * nt * reps + np.arange(4 * nq * reps, dtype=np.int32)).reshape(-1, 4)
    return xyz, tri, quad


def section_table(mats):
    """The distinct (nu, E, t) of `mats` in the order of their first appearance, and every entry's row of that table."""
    rows, index = [], []
    for m in mats:
        m = tuple(float(v) for v in m[:3])
        if m not in rows:
            rows.append(m)
        index.append(rows.index(m))
    return np.array(rows, dtype=np.float64).reshape(-1, 3), np.array(index, dtype=np.int32)


def element_blocks(rowptr, colidx, vals, conn):
    """The matrix of an element that shares no node with another, node-major, from the blocks of the assembled K."""
    n = len(conn)
    K = np.zeros((6 * n, 6 * n))
    for i, a in enumerate(conn):
        cols = colidx[rowptr[a]:rowptr[a + 1]]
        assert sorted(cols) == sorted(conn), (a, cols, conn)
        for j, b in enumerate(conn):
            K[6 * i:6 * i + 6, 6 * j:6 * j + 6] = vals[rowptr[a] + int(np.searchsorted(cols, b))]
    return K


def probe_vector(n_nodes, conn_list, i, a):
    """(n_nodes, 6): 1 at dof a of local node i of every element that has such a node, 0 elsewhere"""
    x = np.zeros((n_nodes, 6))
    x[[c[i] for c in conn_list if len(c) > i], a] = 1.0
    return x


def probe_element_matrices(product, n_nodes, conn_list):
    """The matrices of elements that share no node with another, node-major (as element_blocks gives them), read back through
    `product`, a function x (6 n_nodes,) -> K x: the product with probe_vector(i, a) is column (i, a) of every element's matrix at
    once, 18 products for triangles, 24 where the mesh has a quadrilateral (a triangle has no local node 3 and ignores those).
    Exact: every entry is one K_ab * 1 plus exact zeros, in a row with one contributing element.  Both triangles of a matrix are
    read independently of each other."""
    conn_list = [np.asarray(c, dtype=np.int64) for c in conn_list]
    assert len(np.unique(np.concatenate(conn_list))) == sum(len(c) for c in conn_list), "the elements share nodes"
    K = [np.zeros((6 * len(c), 6 * len(c))) for c in conn_list]
    for i in range(max(len(c) for c in conn_list)):
        for a in range(6):
            y = np.asarray(product(probe_vector(n_nodes, conn_list, i, a).ravel()), dtype=np.float64).reshape(n_nodes, 6)
            for k, c in enumerate(conn_list):
                if len(c) > i:
                    K[k][:, 6 * i + a] = y[c].ravel()
    return K


def device_matrices(pkg, setenv, path, material, tri_xyz=None, quad_xyz=None, tri_mat=None, quad_mat=None, reached=None):
    """Element matrices (node-major, global axes) of triangles tri_xyz (m, 3, 3) and quadrilaterals quad_xyz (m, 4, 3) through
    one device path, under a context of `material` = (nu, E, t, flags); every element gets nodes of its own, so that after
    assembly every block of K holds exactly one contribution, and a product reads one element per row; no Dirichlet nodes, no
    loads.  On an "own" path tri_mat / quad_mat give every element its (nu, E, t), which it gets as a section.  Returns (list for
    the triangles, list for the quadrilaterals), each entry the list of the copies of one element.  reached: a list that gets
    (the plan has quadrilaterals, sections are set) of a product path, the instantiation of k_element_product it launches."""
    kernel, symmetric, sectioned = path
    nu, E, t, flags = material
    nt, nq = (0 if tri_xyz is None else len(tri_xyz)), (0 if quad_xyz is None else len(quad_xyz))
    reps = -(-MIN_ELEMENTS // (nt + nq))
    xyz, tri, quad = isolated_mesh(tri_xyz, quad_xyz, reps)
    if symmetric is not None:
        setenv("FEMSHELL_SYMMETRIC", symmetric)
        setenv("FEMSHELL_ASM_PIPE", KERNELS[kernel])  # (both read per femshell_set_mesh)
    fs = pkg.FemShell(nu, E, t, flags=flags)
    fs.set_mesh(xyz, tri, quad)
    if sectioned == "own":
        table, index = section_table(list(tri_mat or []) + list(quad_mat or []))
        assert len(index) == nt + nq and len(set(map(tuple, table))) > 1, table
        assert all(table[:, k].tolist().count(material[k]) == 0 for k in range(3)), "the context's material is an element's"
        fs.set_sections(table, np.tile(index[:nt], reps), np.tile(index[nt:], reps))
    elif sectioned:
        fs.set_sections([[nu, E, t]], np.zeros(len(tri), np.int32), np.zeros(len(quad), np.int32))
    if kernel == "k_element_matrices":
        Kt = [to_node_major(k, 3) for k in fs.element_matrices(0, len(tri))] if nt else []
        Kq = [to_node_major(k, 4) for k in fs.element_matrices(len(tri), len(quad))] if nq else []
    elif kernel == PRODUCT:
        if reached is not None:
            reached.append((pkg.build_plan(xyz, tri, quad)["n_lquad"] > 0, bool(sectioned)))
        K = probe_element_matrices(fs.element_product, len(xyz), list(tri) + list(quad))
        Kt, Kq = K[:len(tri)], K[len(tri):]
    else:
        assert fs.assembly_kernel() == kernel
        fs.assemble()
        rowptr, colidx, vals, _ = fs.export_bsr()
        Kt = [element_blocks(rowptr, colidx, vals, c) for c in tri]
        Kq = [element_blocks(rowptr, colidx, vals, c) for c in quad]
    fs.close()
    # copy r of element k of the group is element r * m + k: hand back the copies of each element together
    return ([[Kt[r * nt + k] for r in range(reps)] for k in range(nt)],
            [[Kq[r * nq + k] for r in range(reps)] for k in range(nq)])


def family_worst(fx, fam, path, evaluate, elements=None):
    """metric -> the worst error over the family (all copies of every element) of the matrices that
    evaluate(path, material, tri_xyz, quad_xyz, tri_mat, quad_mat) returns (as device_matrices does), context by context"""
    tri_fam = nodes_of(fam) == 3
    own = path[2] == "own"
    names = metrics_of(fam) + (["spurious"] if fam in CLASSWISE else [])
    worst = {m: 0.0 for m in names}
    for material, els in groups_of(fx, fam, elements, own).items():
        X = [fx[fam + "_xyz"][e] for e in els]
        mats = [material_of(fx, fam, e)[:3] for e in els] if own else None
        if fam in FRAME:  # the moved copies ride in the same mesh, behind the originals
            X = X + [fx[fam + "_xyz_moved"][e] for e in els]
            mats = mats + mats if own else None
        Kt, Kq = evaluate(path, material, X if tri_fam else None, None if tri_fam else X, mats if tri_fam else None,
                          None if tri_fam else mats)
        K = Kt if tri_fam else Kq
        for r in range(len(K[0])):
            err = family_errors(fx, fam, [K[k][r] for k in range(len(els))],
                                [K[len(els) + k][r] for k in range(len(els))] if fam in FRAME else None, els)
            for m in names:
                worst[m] = max(worst[m], float(err[m].max()))
    return worst


def device_family_errors(pkg, setenv, fx, fam, path, elements=None, reached=None):
    """metric -> the device's worst error over the family (all copies of every element) through one path"""
    def evaluate(path, material, tri_xyz, quad_xyz, tri_mat, quad_mat):
        return device_matrices(pkg, setenv, path, material, tri_xyz, quad_xyz, tri_mat, quad_mat, reached)
    return family_worst(fx, fam, path, evaluate, elements)


def check(fx, fam, worst, factors=None):
    """[(metric, device worst, oracle worst, bound)] of the metrics over their bound; "spurious" must be 0"""
    bad = []
    for m in metrics_of(fam):
        o = float(fx["%s_err_%s" % (fam, m)].max())
        b = bound(o, (factors or {}).get(m, 4.0))
        if not worst[m] <= b:
            bad.append((m, worst[m], o, b))
    if worst.get("spurious", 0):
        bad.append(("spurious", worst["spurious"], 0, 0))
    return bad
