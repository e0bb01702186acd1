"""Element loads (femshell_set_element_loads): the reference of the tests, numpy in longdouble, written from the definition of
include/femshell.h and not from the kernel.  Every function computes in `work` (longdouble unless a caller asks for the same
formulas in FP64: the reference's own error, tests/helpers/derived_truth.py).

Per element (p, qx, qy, qz).  With the two vectors of the element's cross product -- TRI3: the edges d1 = b - a, d2 = c - a,
QUAD4: the diagonals d1 = c - a, d2 = d - b -- the vector area is d1 x d2 / 2, the area A its length, and every node of the
element gets
    TRI3   p (d1 x d2) / 6 + q A / 3        QUAD4   p (d1 x d2) / 8 + q A / 4
on u, v, w and nothing on the rotations.  The scale of a node row, which the device's error is measured against:
    T_a = sum over the elements e that contain a of (|p_e| + ||q_e||_1) |d1_e| |d2_e|.
"""
import numpy as np

LD = np.longdouble


def cross_vectors(xyz, conn, work=LD):
    """(d1, d2) of every element of conn ((n, 3) triangles or (n, 4) quadrilaterals), in `work`"""
    x = np.asarray(xyz, dtype=np.float64).astype(work)
    conn = np.asarray(conn)
    if conn.shape[1] == 3:
        a, b, c = (x[conn[:, i]] for i in range(3))
        return b - a, c - a
    a, b, c, d = (x[conn[:, i]] for i in range(4))
    return c - a, d - b


def _kinds(tri, quad, tri_load, quad_load, work=LD):
    for conn, load, nn in ((tri, tri_load, 3), (quad, quad_load, 4)):
        if conn is None or len(conn) == 0:
            continue
        conn = np.asarray(conn).reshape(-1, nn)
        load = np.zeros((len(conn), 4)) if load is None else np.asarray(load, dtype=np.float64).reshape(len(conn), 4)
        yield conn, load.astype(work), nn


def element_terms(xyz, tri=None, quad=None, tri_load=None, quad_load=None, work=LD):
    """per element, triangles then quadrilaterals: (pressure resultant p vecarea (n, 3), traction resultant q A (n, 3)), in `work`"""
    fp, fq = [np.zeros((0, 3), work)], [np.zeros((0, 3), work)]
    for conn, load, nn in _kinds(tri, quad, tri_load, quad_load, work):
        d1, d2 = cross_vectors(xyz, conn, work)
        va = np.cross(d1, d2) / work(2)
        area = np.sqrt((va * va).sum(axis=1))
        fp.append(load[:, :1] * va)
        fq.append(load[:, 1:] * area[:, None])
    return np.concatenate(fp), np.concatenate(fq)


def element_shares(xyz, conn, load, work=LD):
    """(n, 3): what every node of each element of conn gets on u, v, w from the load rows (p, qx, qy, qz), in `work`"""
    conn = np.asarray(conn)
    nn = conn.shape[1]
    d1, d2 = cross_vectors(xyz, conn, work)
    cr = np.cross(d1, d2)
    area = np.sqrt((cr * cr).sum(axis=1)) / work(2)
    load = np.asarray(load, dtype=np.float64).reshape(len(conn), 4).astype(work)
    return load[:, :1] * cr / work(2 * nn) + load[:, 1:] * (area / work(nn))[:, None]


def load_vector(xyz, tri=None, quad=None, tri_load=None, quad_load=None, dtype=np.float64, work=LD):
    """(S, T): S (n_nodes, 6) the lumped nodal equivalents (summed in `work`, returned as dtype), T (n_nodes,) the row scale"""
    n = len(xyz)
    S = np.zeros((n, 6), work)
    T = np.zeros(n, work)
    for conn, load, nn in _kinds(tri, quad, tri_load, quad_load, work):
        d1, d2 = cross_vectors(xyz, conn, work)
        share = element_shares(xyz, conn, load, work)
        scale =np.abs(load).sum(axis=1) * np.sqrt((d1 * d1).sum(axis=1)) * np.sqrt((d2 * d2).sum(axis=1))
        for i in range(nn):
            np.add.at(S[:, :3], conn[:, i], share)
            np.add.at(T, conn[:, i], scale)
    return S.astype(dtype), T.astype(np.float64)


def random_loads(n_tri, n_quad, seed=3):
    """seeded (tri_load, quad_load), entries in (-1, 1) scaled so that pressure and tractions differ in size; None for an absent kind"""
    rng = np.random.default_rng(seed)
    tl = rng.uniform(-1.0, 1.0, (n_tri, 4)) * [300.0, 5.0, 7.0, 90.0] if n_tri else None
    ql = rng.uniform(-1.0, 1.0, (n_quad, 4)) * [300.0, 5.0, 7.0, 90.0] if n_quad else None
    return tl, ql


def bound_ratio(S, S_ref, T, tol=1e-12):
    """max over rows and translations of |S - S_ref| / (tol T_a); a row whose scale is zero must agree exactly"""
    diff = np.abs(np.asarray(S)[:, :3] - np.asarray(S_ref)[:, :3]).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(T > 0, diff / (tol * T), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def model_bytes(n_listed, n_nodes, n_own):
    """the byte model of femshell_time_kernel(FEMSHELL_KERNEL_ELEMENT_LOADS): per listed element 16 B of node ids, 4 B of element
    index, 32 B of load words; 24 B of coordinates per node; 48 B of base read and 48 B written per owned row"""
    return (16.0 + 4.0 + 32.0) * n_listed + 24.0 * n_nodes + 96.0 * n_own


def listed_elements(n_nodes, tri=None, quad=None):
    """entries of the slices' element lists without a renumbering: per slice of 32 consecutive node rows, the elements that
    contain one of its nodes"""
    total = 0
    for conn in (tri, quad):
        if conn is None or len(conn) == 0:
            continue
        slices = np.asarray(conn) // 32
        total += sum(len(set(row)) for row in slices.tolist())
    return total


def octahedron(r=(1.0, 1.3, 0.7)):
    """8 outward-oriented triangles on the six points (+-rx, 0, 0), (0, +-ry, 0), (0, 0, +-rz): a closed surface"""
    xyz = np.array([[r[0], 0, 0], [-r[0], 0, 0], [0, r[1], 0], [0, -r[1], 0], [0, 0, r[2]], [0, 0, -r[2]]], dtype=np.float64)
    tri = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return xyz, tri
