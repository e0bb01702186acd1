"""Elastic supports (femshell_set_foundation, femshell_set_springs): the reference of the tests, numpy in longdouble, written from
the definition of include/femshell.h and not from the kernels.  Every function computes in `work` (longdouble unless a caller asks
for the same formulas in FP64: the reference's own error).

Per element (kn, kt).  With the two vectors of the element's cross product -- TRI3: d1 = b - a, d2 = c - a, QUAD4: the diagonals
d1 = c - a, d2 = d - b -- c = d1 x d2, A = |c| / 2, n = c / |c|, and every node of the element gets the 3 x 3 block
    B_e = share [kt I + (kn - kt) n n^T],   share = A / 3 (TRI3), A / 4 (QUAD4)
(zero where |c| = 0).  The support table holds per node nine words: T_a = sum of the B_e as xx, yy, zz, xy, yz, zx with the
springs kx, ky, kz added to the first three, then krx, kry, krz.  The scale of a node row, which the device's error is measured
against:
    T_a = sum over the elements e that contain a of (kn_e + kt_e) |d1_e| |d2_e|  +  the largest of the node's six springs.
"""
import numpy as np

from tests.helpers import element_loads as el

LD = np.longdouble
WORDS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))  # xx yy zz xy yz zx


def _kinds(tri, quad, tri_k, quad_k, work=LD):
    for conn, k, nn in ((tri, tri_k, 3), (quad, quad_k, 4)):
        if conn is None or len(conn) == 0:
            continue
        conn = np.asarray(conn).reshape(-1, nn)
        k = np.zeros((len(conn), 2)) if k is None else np.asarray(k, dtype=np.float64).reshape(len(conn), 2)
        yield conn, k.astype(work), nn


def element_tensors(xyz, conn, k, work=LD):
    """(area (n,), G (n, 3, 3)): A_e and the per-area tensor kt I + (kn - kt) n n^T of every element of conn, in `work`; a
    degenerate element has A = 0 and G = kt I"""
    d1, d2 = el.cross_vectors(xyz, conn, work)
    c = np.cross(d1, d2)
    ln = np.sqrt((c * c).sum(axis=1))
    area = ln / work(2)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(ln[:, None] > 0, c / ln[:, None], work(0))
    k = np.asarray(k).astype(work)
    G = k[:, 1, None, None] * np.eye(3, dtype=work)[None] + (k[:, 0] - k[:, 1])[:, None, None] * n[:, :, None] * n[:, None, :]
    return area, G


def table(xyz, tri=None, quad=None, tri_k=None, quad_k=None, springs=None, dtype=np.float64, work=LD):
    """(S, T): S (n_nodes, 9) the support table (summed in `work`, returned as dtype), T (n_nodes,) the row scale.  springs: None
    or (n_nodes, 6)"""
    n = len(xyz)
    S = np.zeros((n, 9), work)
    T = np.zeros(n, work)
    for conn, k, nn in _kinds(tri, quad, tri_k, quad_k, work):
        d1, d2 = el.cross_vectors(xyz, conn, work)
        area, G = element_tensors(xyz, conn, k, work)
        B = (area / work(nn))[:, None, None] * G
        words = np.stack([B[:, i, j] for i, j in WORDS], axis=1)
        scale = k.sum(axis=1) * np.sqrt((d1 * d1).sum(axis=1)) * np.sqrt((d2 * d2).sum(axis=1))
        for i in range(nn):
            np.add.at(S[:, :6], conn[:, i], words)
            np.add.at(T, conn[:, i], scale)
    if springs is not None:
        sp = np.asarray(springs, dtype=np.float64).reshape(n, 6).astype(work)
        S[:, :3] += sp[:, :3]
        S[:, 6:] = sp[:, 3:]
        T += sp.max(axis=1)
    return S.astype(dtype), T.astype(np.float64)


def blocks(S):
    """(n_nodes, 6, 6): the diagonal blocks of K_sup of a table"""
    S = np.asarray(S)
    B = np.zeros((len(S), 6, 6), S.dtype)
    for w, (i, j) in enumerate(WORDS):
        B[:, i, j] = S[:, w]
        B[:, j, i] = S[:, w]
    for d in range(3):
        B[:, 3 + d, 3 + d] = S[:, 6 + d]
    return B


def masked_blocks(S, mask):
    """... with the rows and columns of the fixed dofs of the Dirichlet mask zeroed: mask(K_sup)"""
    B = blocks(S)
    if mask is None:
        return B
    free = ((np.asarray(mask, dtype=np.uint8)[:, None] >> np.arange(6)) & 1) == 0
    return B * (free[:, :, None] & free[:, None, :])


def apply(S, x, mask=None):
    """mask(K_sup) x, (n_nodes, 6)"""
    x = np.asarray(x).reshape(len(S), 6)
    return np.einsum("aij,aj->ai", masked_blocks(S, mask), x)


def diagonal_slots(rowptr, colidx):
    """index of the diagonal block of every block row"""
    rowptr, colidx = np.asarray(rowptr), np.asarray(colidx)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    slots = np.flatnonzero(colidx == rows)
    assert len(slots) == len(rowptr) - 1
    return slots


def add_to_bsr(K, S, mask=None):
    """(rowptr, colidx, vals) of K + mask(K_sup): one addition per entry of the diagonal blocks"""
    rowptr, colidx, vals = K
    vals = np.array(vals, dtype=np.float64).reshape(len(colidx), 6, 6)
    d = diagonal_slots(rowptr, colidx)
    vals[d] = vals[d] + masked_blocks(np.asarray(S, dtype=np.float64), mask)
    return rowptr, colidx, vals


def random_moduli(n_tri, n_quad, seed=5):
    """seeded (tri_k, quad_k), kn in [0, 4e3) and kt in [0, 5e2); every seventh element without a foundation, every eleventh
    with kt alone; None for an absent kind"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (n_tri, n_quad):
        if not n:
            out.append(None)
            continue
        k = rng.uniform(0.0, 1.0, (n, 2)) * [4e3, 5e2]
        k[::7] = 0.0
        k[3::11, 0] = 0.0
        out.append(k)
    return tuple(out)


def random_springs(n_nodes, seed=6):
    """(n_nodes, 6): seeded springs on every third node (from node 1), zero elsewhere; listed form: nodes_of(springs)"""
    rng = np.random.default_rng(seed)
    sp = np.zeros((n_nodes, 6))
    ids = np.arange(1, n_nodes, 3) if n_nodes > 1 else np.arange(n_nodes)
    sp[ids] = rng.uniform(0.0, 1.0, (len(ids), 6)) * [2e3, 1e3, 3e3, 40.0, 50.0, 60.0]
    return sp


def nodes_of(springs):
    """(ids, rows) of the nodes that carry a spring, in a shuffled order"""
    ids = np.flatnonzero(np.asarray(springs).any(axis=1)).astype(np.int32)
    ids = ids[np.random.default_rng(1).permutation(len(ids))]
    return ids, np.asarray(springs)[ids]


def bound_ratio(S, S_ref, T, tol=1e-12):
    """max over rows and the nine words of |S - S_ref| / (tol T_a); a row whose scale is zero must agree exactly"""
    diff = np.abs(np.asarray(S, dtype=np.float64) - np.asarray(S_ref, dtype=np.float64)).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(T > 0, diff / (tol * T), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def model_bytes(n_listed, n_nodes, n_slices):
    """the byte model of femshell_time_kernel(FEMSHELL_KERNEL_ELASTIC_SUPPORT): per listed element 16 B of node ids, 4 B of
    element index, 16 B of moduli; 24 B of coordinates per node; 72 B written per row of the slices"""
    return (16.0 + 4.0 + 16.0) * n_listed + 24.0 * n_nodes + 72.0 * 32 * n_slices


def navier_centre(a, D, q, k, terms=199):
    """centre deflection of a simply supported square plate of side a under uniform pressure q on a Winkler foundation k:
    w = sum over odd m, n of q_mn sin(m pi / 2) sin(n pi / 2) / (D pi^4 ((m/a)^2 + (n/a)^2)^2 + k), q_mn = 16 q / (pi^2 m n)"""
    w = 0.0
    for m in range(1, terms + 1, 2):
        for n in range(1, terms + 1, 2):
            qmn = 16.0 * q / (np.pi ** 2 * m * n)
            w += qmn * np.sin(m * np.pi / 2) * np.sin(n * np.pi / 2) / (D * np.pi ** 4 * ((m / a) ** 2 + (n / a) ** 2) ** 2 + k)
    return w
