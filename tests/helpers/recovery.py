"""Nodal stress recovery and the Zienkiewicz-Zhu indicator (femshell_nodal_resultants): the reference of the tests, numpy with
plain loops on top of tests/helpers/resultants.mesh_resultants.  include/femshell.h and DESIGN.md 8k have the definitions:

    T:T = xx^2 + yy^2 + zz^2 + 2 (xy^2 + yz^2 + zx^2),  tr T = xx + yy + zz          (tensors: xx yy zz xy yz zx, global axes)
    q_nu(S, T) = (1 + nu) S:T - nu tr S tr T,  cN = q_nu / (E t),  cM = 12 q_nu / (E t^3)
    a_e = (b - a) x (c - a) / 2 (TRI3),  d1 x d2 / 2 with d1 = c - a, d2 = d - b (QUAD4);  A_e = |a_e|
    node:     N* = sum_e A_e N_e / W,  M* = sum_e A_e M_e / W,  W = sum_e A_e,  fold = 1 - |sum_e a_e| / W;  W = 0: zeros
    element:  e2 = A_e c(sigma_e, sigma_e),  eta^2 = A_e sum_ij w_ij c(d_i, d_j),  d_i = (N*_i - N_e, M*_i - M_e)
              w_ij = (1 + delta_ij) / 12 (TRI3);  4/36 same corner, 2/36 shared side, 1/36 diagonal (QUAD4)

Every function works in the `dtype` it is given (float64, or numpy's long double for the second evaluation the tests compare the
first with) and returns float64.

The bounds a device result is held to (derived, not tuned; EPS = 2^-52):
    node tensors  |out - ref| <= sum_e A_e (1e-12 S_e) / W + (k + 16) EPS sum_e A_e |sigma_e| / W,  k elements at the node: the
                  convex combination of the per-element bounds of tests/test_gpu_resultants.py, and k - 1 additions, the products,
                  the two areas and the division
    W             (k + 8) EPS W;   fold  32 EPS
    e2, eta^2     with delta the component bounds of the differences (node bound + element bound for eta^2, element bound for
                  e2) and Q the quadratic form:  |Q(D + Delta) - Q(D)| <= 2 sqrt(Q(D) Q(delta)) + Q(delta) + 64 EPS Q(D)
                  (Cauchy-Schwarz for a positive semi-definite form)
"""
import numpy as np

from tests.helpers import oracle, resultants as rs

EPS = float(np.finfo(np.float64).eps)
W_TRI = [[(2.0 if i == j else 1.0) / 12.0 for j in range(3)] for i in range(3)]
W_QUAD = [[(4.0 if i == j else (1.0 if (i - j) % 4 == 2 else 2.0)) / 36.0 for j in range(4)] for i in range(4)]


def ddot(S, T):
    return S[0] * T[0] + S[1] * T[1] + S[2] * T[2] + 2 * (S[3] * T[3] + S[4] * T[4] + S[5] * T[5])


def trace(T):
    return T[0] + T[1] + T[2]


def q_form(S, T, nu):
    return (1 + nu) * ddot(S, T) - nu * trace(S) * trace(T)


def c_form(s, t, nu, E, th):
    """c(s, t) of two 12-vectors (N part, M part)"""
    return q_form(s[:6], t[:6], nu) / (E * th) + 12 * q_form(s[6:], t[6:], nu) / (E * th * th * th)


def vector_area(X):
    """a_e of an element's coordinates (3 or 4 rows)"""
    if len(X) == 3:
        return np.cross(X[1] - X[0], X[2] - X[0]) / 2
    return np.cross(X[2] - X[0], X[3] - X[1]) / 2


def elements_of(tri, quad):
    """the node lists of a mesh's elements in the caller's order: triangles, then quadrilaterals"""
    out = []
    if tri is not None:
        out += [list(map(int, c)) for c in np.asarray(tri).reshape(-1, 3)]
    if quad is not None:
        out += [list(map(int, c)) for c in np.asarray(quad).reshape(-1, 4)]
    return out


def materials_of(tri, quad, nu, E, t, sec=None):
    """(nu, E, t) per element, the section's where sec = (sections (n, 3), tri_section, quad_section) is given"""
    n_tri = 0 if tri is None else len(np.asarray(tri).reshape(-1, 3))
    n_quad = 0 if quad is None else len(np.asarray(quad).reshape(-1, 4))
    if sec is None:
        return [(nu, E, t)] * (n_tri + n_quad)
    table = np.asarray(sec[0], dtype=np.float64).reshape(-1, 3)
    ids = ([] if n_tri == 0 else list(sec[1])) + ([] if n_quad == 0 else list(sec[2]))
    return [tuple(table[int(s)]) for s in ids]


def recover(xyz, tri, quad, res, dtype=np.float64):
    """nodes (n_nodes, 14) from the element rows res (n_elem, >= 12), and the number of elements at every node"""
    X = np.asarray(xyz, dtype=dtype)
    res = np.asarray(res, dtype=dtype)
    n = len(X)
    acc = np.zeros((n, 12), dtype=dtype)
    W = np.zeros(n, dtype=dtype)
    av = np.zeros((n, 3), dtype=dtype)
    count = np.zeros(n, np.int64)
    for e, nodes in enumerate(elements_of(tri, quad)):
        a = vector_area(X[nodes])
        A = np.sqrt(a @ a)
        for i in nodes:
            acc[i] += A * res[e, :12]
            W[i] += A
            av[i] += a
            count[i] += 1
    out = np.zeros((n, 14), dtype=dtype)
    for i in range(n):
        if W[i] > 0:
            out[i, :12] = acc[i] / W[i]
            out[i, 12] = W[i]
            out[i, 13] = 1 - np.sqrt(av[i] @ av[i]) / W[i]
    return out.astype(np.float64), count


def indicator(xyz, tri, quad, res, nodes, mats, dtype=np.float64):
    """elems (n_elem, 2): e2 and eta^2 from the element rows, the recovered node rows and the elements' (nu, E, t)"""
    X = np.asarray(xyz, dtype=dtype)
    res = np.asarray(res, dtype=dtype)
    nodes = np.asarray(nodes, dtype=dtype)
    out = []
    for e, conn in enumerate(elements_of(tri, quad)):
        nu, E, th = (dtype(v) for v in mats[e])
        a = vector_area(X[conn])
        A = np.sqrt(a @ a)
        sig = res[e, :12]
        d = [nodes[i, :12] - sig for i in conn]
        w = W_TRI if len(conn) == 3 else W_QUAD
        eta = dtype(0)
        for i in range(len(conn)):
            for j in range(len(conn)):
                eta += dtype(w[i][j]) * c_form(d[i], d[j], nu, E, th)
        out.append([A * c_form(sig, sig, nu, E, th), A * eta])
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def relative_error(elems):
    """sqrt(sum eta^2 / (sum e2 + sum eta^2)), summed in the elements' order"""
    e2 = eta2 = 0.0
    for a, b in np.asarray(elems, dtype=np.float64).reshape(-1, 2):
        e2 += a
        eta2 += b
    return float(np.sqrt(eta2 / (e2 + eta2))) if e2 + eta2 > 0.0 else 0.0


class Recovery:
    """The reference of one mesh and one u: res, S (the element rows and their scales, tests/helpers/resultants.py), nodes, elems,
    and the bounds of the module's head as arrays of the same shapes (node_bound (n, 14), elem_bound (n_elem, 2)).  res_given: the
    element rows and scales from elsewhere (temperatures in force: tests/helpers/thermal.mesh_resultants)."""

    def __init__(self, xyz, tri, quad, u, nu=rs.NU, E=rs.E, t=rs.T, sec=None, flags=oracle.REF_DEFAULT, dtype=np.float64, res_given=None):
        self.xyz, self.tri, self.quad = np.asarray(xyz, dtype=np.float64), tri, quad
        if res_given is not None:
            self.res, self.S = res_given
        elif dtype is np.float64:
            self.res, self.S = rs.mesh_resultants(xyz, tri, quad, u, nu, E, t, sec=sec, flags=flags)
        else:  # the second evaluation, as tests/test_resultants_cpu.py takes it
            self.res, self.S = rs.mesh_resultants(xyz, tri, quad, u, nu, E, t, sec=sec, flags=flags, dtype=dtype, quad_parts=True)
        self.mats = materials_of(tri, quad, nu, E, t, sec)
        self.nodes, self.count = recover(xyz, tri, quad, self.res, dtype)
        self.elems = indicator(xyz, tri, quad, self.res, self.nodes, self.mats, dtype)
        self._bounds()

    def _bounds(self):
        n = len(self.xyz)
        conns = elements_of(self.tri, self.quad)
        wS, wabs, W = np.zeros((n, 12)), np.zeros((n, 12)), np.zeros(n)
        areas = []
        for e, conn in enumerate(conns):
            a = vector_area(self.xyz[conn])
            A = float(np.sqrt(a @ a))
            areas.append(A)
            for i in conn:
                wS[i] += A * rs.TINY * self.S[e, :12]
                wabs[i] += A * np.abs(self.res[e, :12])
                W[i] += A
        nb = np.zeros((n, 14))
        for i in range(n):
            if W[i] > 0:
                nb[i, :12] = wS[i] / W[i] + (self.count[i] + 16) * EPS * wabs[i] / W[i]
                nb[i, 12] = (self.count[i] + 8) * EPS * W[i]
                nb[i, 13] = 32 * EPS
        self.node_bound = nb
        eb = np.zeros((len(conns), 2))
        for e, conn in enumerate(conns):
            nu, E, th = self.mats[e]
            de = rs.TINY * self.S[e, :12]
            q0 = areas[e] * c_form(de, de, nu, E, th)
            eb[e, 0] = 2 * np.sqrt(self.elems[e, 0] * q0) + q0 + 64 * EPS * self.elems[e, 0]
            dl = [nb[i, :12] + de for i in conn]
            w = W_TRI if len(conn) == 3 else W_QUAD
            q1 = areas[e] * sum(w[i][j] * c_form(dl[i], dl[j], nu, E, th) for i in range(len(conn)) for j in range(len(conn)))
            eb[e, 1] = 2 * np.sqrt(self.elems[e, 1] * q1) + q1 + 64 * EPS * self.elems[e, 1]
        self.elem_bound = eb

    def ratios(self, nodes, elems):
        """largest |out - ref| / bound of (node tensors, W, fold, e2, eta^2); an entry whose bound is zero must agree exactly"""
        def ratio(out, ref, bound):
            diff = np.abs(np.asarray(out, dtype=np.float64) - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
            return float(r.max()) if r.size else 0.0
        nodes, elems = np.asarray(nodes), np.asarray(elems)
        return (ratio(nodes[:, :12], self.nodes[:, :12], self.node_bound[:, :12]), ratio(nodes[:, 12], self.nodes[:, 12], self.node_bound[:, 12]),
                ratio(nodes[:, 13], self.nodes[:, 13], self.node_bound[:, 13]), ratio(elems[:, 0], self.elems[:, 0], self.elem_bound[:, 0]),
                ratio(elems[:, 1], self.elems[:, 1], self.elem_bound[:, 1]))


# ------------------------------------------------------------------ the meshes the device is compared on (tests/test_gpu_recovery.py)

def panel_nodes(n):
    """the lifted, jittered panel of 8 x 4 nodes cut down to n = 31 or 32 nodes (its last node and the two triangles at it removed),
    or the 33 nodes of tests/helpers/prescribed.strip33: one below, exactly and one above a slice of 32 node rows"""
    from tests.helpers import prescribed as pr
    if n == 33:
        return pr.strip33()
    xyz, tri = pr.panel(nx=7, ny=3, lx=3.5, ly=1.5, jitter=0.2, seed=5, lift=True)
    if n == 32:
        return xyz, tri
    assert n == 31
    tri = tri[(tri != 31).all(axis=1)]
    assert sorted(np.unique(tri)) == list(range(31))
    return xyz[:31], tri


def folded_plate(cells=4, h=0.25):
    """two square panels of cells x cells quadrilaterals of side h that meet at a right angle along the line x = cells h: the first
    in the plane z = 0, the second in the plane x = cells h; node j * (2 cells + 1) + i, every element with the same sense along
    the developed surface.  Returns (xyz, quad, the ridge's nodes)."""
    ni = 2 * cells + 1
    xyz = []
    for j in range(cells + 1):
        for i in range(ni):
            xyz.append([min(i, cells) * h, j * h, max(i - cells, 0) * h])
    quad = [[j * ni + i, j * ni + i + 1, (j + 1) * ni + i + 1, (j + 1) * ni + i] for j in range(cells) for i in range(2 * cells)]
    return np.array(xyz, dtype=np.float64), np.array(quad, np.int32), np.array([j * ni + cells for j in range(cells + 1)])


def device_meshes():
    """name -> function returning (xyz, tri, quad, sec, env): those of tests/helpers/resultants.device_meshes and the smallest shapes
    at which the slice mapping of k_nodal_recovery can go wrong"""
    from tests.helpers import meshes
    cases = dict(rs.device_meshes())
    for n in (31, 32, 33):
        cases["panel_%d_nodes" % n] = (lambda n=n: panel_nodes(n) + (None, None, {}))
    cases["fan300_hub_first"] = lambda: meshes.coil(300, hub_last=False) + (None, None, {})  # one slice's list crosses the tile of 256
    cases["folded_plate"] = lambda: (folded_plate()[0], None, folded_plate()[1], None, {})
    return cases
