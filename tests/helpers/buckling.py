"""Linear buckling (femshell_geometric_product): the reference of the tests, numpy and scipy on
tests/helpers/resultants.py and the oracle's assemblies, written from the definition and not from the kernel.

Prestress of an element: its element-mean membrane force N_loc = (Nxx, Nyy, Nxy) of DESIGN.md 8d, from a displacement vector u.
With phi_a the membrane shape functions in the element frame (TRI3: linear, one point of weight A; QUAD4: bilinear at the 2 x 2
Gauss points of the stiffness, weight det J):
    g_ab = sum_gp w_gp grad phi_a(gp)^T [[Nxx, Nxy], [Nxy, Nyy]] grad phi_b(gp),    K_G,e[a, b] = g_ab I3 on the translations.
The gradients are read off the membrane strain operators of resultants.py: row 0 of Bm holds phi_a,x in the u columns, row 1
phi_a,y in the v columns.

The scale a device product is measured against, per node row a and column of X:
    T_a = sum_{e contains a} sum_b sum_gp |w_gp| |grad phi_a|^T S^N_e |grad phi_b| ||x_b||_1,
S^N_e the 2 x 2 matrix of 8d's absolute-sum scales of N_loc, ||x_b||_1 over the three translations of node b.

The pencil (K + lambda K_G) x = 0 on the free dofs is solved as -K_G x = mu K x, mu = 1 / lambda, by a dense scipy.linalg.eigh.
"""
import numpy as np
import scipy.linalg as sla

from tests.helpers import oracle, prescribed as pr, resultants as rs

TINY = 1e-12
CLUSTER_GAP = 1e-2


# ------------------------------------------------------------------ element level

def element_prestress(xyz, u, nu, E, t, flags=oracle.REF_DEFAULT, dtype=np.float64, restated=False):
    """(N_loc (3,), S_N (3,), ops): the element-mean membrane force in the element frame, its absolute-sum scale and the
    operators of resultants.py, all in `dtype`; restated: as rs.element_resultants has it"""
    xyz = np.asarray(xyz, dtype=np.float64)
    nn = len(xyz)
    ops = rs.tri3_operators(xyz, flags, dtype, restated=restated) if nn == 3 else rs.quad4_operators(xyz, dtype, relative=bool(restated))
    T = ops["trafo"]
    ul = np.asarray(u, dtype=dtype).reshape(nn, 6)[:, :3] @ T.T
    dm = ul[:, :2].reshape(-1)
    tDm, _ = rs.plane_material(nu, E, t, dtype)
    DBm = tDm @ rs.mean_operator(ops["Bm"], ops["wm"])
    return DBm @ dm, np.abs(DBm) @ np.abs(dm), ops


def element_g(ops, N, dtype=np.float64, absolute=False):
    """g (nn, nn) of one element from its operators and N = (Nxx, Nyy, Nxy); absolute: the same sum with |w|, |grad phi| (N is then
    the scale S_N): the element's part of T_a"""
    nn = ops["Bm"][0].shape[1] // 2
    Nm = np.array([[N[0], N[2]], [N[2], N[1]]], dtype=dtype)
    g = np.zeros((nn, nn), dtype=dtype)
    for B, w in zip(ops["Bm"], ops["wm"]):
        grad = np.stack([B[0, 0::2], B[1, 1::2]], axis=1).astype(dtype)  # (nn, 2)
        w = dtype(w)
        if absolute:
            grad, w = np.abs(grad), abs(w)
        g += w * (grad @ Nm @ grad.T)
    return g


def _elements(xyz, tri, quad, nu, E, t, sec):
    for conn, which in ((tri, 1), (quad, 2)):
        if conn is None or len(conn) == 0:
            continue
        for e, c in enumerate(np.asarray(conn).reshape(-1, 3 if which == 1 else 4)):
            m = (nu, E, t) if sec is None else tuple(np.asarray(sec[0], dtype=np.float64).reshape(-1, 3)[sec[which][e]])
            yield c, m


def element_coefficients(xyz, tri, quad, u, nu, E, t, sec=None, flags=oracle.REF_DEFAULT, dtype=np.float64, N_uniform=None,
                         restated=False):
    """list of (conn, g (nn, nn), |g| scale (nn, nn)) per element, triangles then quadrilaterals.  N_uniform = (Nxx, Nyy, Nxy)
    in the global x-y axes: that membrane force in every element, taken into its frame, instead of the one recovered from u (the
    plate checks)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    u = None if u is None else np.asarray(u, dtype=np.float64).reshape(len(xyz), 6)
    out = []
    for c, m in _elements(xyz, tri, quad, nu, E, t, sec):
        N, SN, ops = element_prestress(xyz[c], np.zeros((len(c), 6)) if u is None else u[c], *m, flags=flags, dtype=dtype,
                                       restated=restated)
        if N_uniform is not None:
            A = np.zeros((3, 3), dtype=dtype)
            A[0, 0], A[1, 1], A[0, 1], A[1, 0] = N_uniform[0], N_uniform[1], N_uniform[2], N_uniform[2]
            L = ops["trafo"] @ A @ ops["trafo"].T
            N = np.array([L[0, 0], L[1, 1], L[0, 1]], dtype=dtype)
            SN = np.abs(N)
        out.append((c, element_g(ops, N, dtype), element_g(ops, SN, dtype, absolute=True)))
    return out


# ------------------------------------------------------------------ mesh level

def dense_KG(n_nodes, coeffs, dtype=np.float64):
    """K_G (6 n, 6 n) dense: g_ab on the three translations of the blocks (a, b), zero on the rotations"""
    KG = np.zeros((6 * n_nodes, 6 * n_nodes), dtype=dtype)
    for c, g, _ in coeffs:
        for i, a in enumerate(c):
            for j, b in enumerate(c):
                for d in range(3):
                    KG[6 * a + d, 6 * b + d] += g[i, j]
    return KG


def product(n_nodes, coeffs, X, dtype=np.float64):
    """(Y, T): Y = K_G X for X (n_cols, n_nodes, 6), summed element by element in `dtype`; T (n_cols, n_nodes) the row scales"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, n_nodes, 6)
    Y = np.zeros(X.shape, dtype=dtype)
    T = np.zeros(X.shape[:2], dtype=dtype)
    Xd = X.astype(dtype)
    x1 = np.abs(Xd[:, :, :3]).sum(axis=2)
    for c, g, ga in coeffs:
        Y[:, c, :3] += np.einsum("ab,kbd->kad", g, Xd[:, c, :3])
        T[:, c] += x1[:, c] @ ga.T
    return Y, T.astype(np.float64)


def bound_ratio(Y, Y_ref, T, tol=TINY):
    """max over columns, rows and translations of |Y - Y_ref| / (tol T_a); a row whose scale is zero must agree exactly"""
    n_cols, n = T.shape
    diff = np.abs(np.asarray(Y, dtype=np.float64).reshape(n_cols, n, 6)[:, :, :3]
                  - np.asarray(Y_ref).reshape(n_cols, n, 6)[:, :, :3].astype(np.longdouble)).max(axis=2).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(T > 0, diff / (tol * T), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------ the pencil

def stiffness(xyz, tri, quad, nu, E, t, mask, sec=None):
    """the oracle's constrained K as a dense array (6 n, 6 n)"""
    K_c = pr.matrices(xyz, tri, quad, oracle.material(nu, E, t), mask, sec)[1]
    return oracle.to_scipy(*K_c).toarray()


def pencil(K, KG, mask, tie=0.0):
    """All pairs of -K_G x = mu K x on the free dofs of `mask`: (mu descending by |mu| with a positive one before a negative one of
    equal magnitude -- magnitudes within the relative distance `tie` count as equal, as the solver counts those within its tol --,
    V (n_free, n_free) K-orthonormal columns in that order, free)."""
    free = np.flatnonzero(~pr.fixed_dofs(mask))
    Kf = K[np.ix_(free, free)]
    Af = -KG[np.ix_(free, free)]
    mu, V = sla.eigh(0.5 * (Af + Af.T), 0.5 * (Kf + Kf.T))
    order = list(np.lexsort((-np.sign(mu), -np.abs(mu))))
    for j in range(len(order) - 1):
        a, b = mu[order[j]], mu[order[j + 1]]
        if a < 0.0 < b and abs(abs(a) - abs(b)) <= tie * abs(a):
            order[j], order[j + 1] = order[j + 1], order[j]
    return mu[order], V[:, order], free


def factors(mu, n):
    """the n load factors of smallest magnitude, signed, from the ordered mu of pencil()"""
    return 1.0 / mu[:n]


def clusters(mu, gap=CLUSTER_GAP):
    """lists of indices into mu (any order): values whose sorted neighbours differ by less than gap * |mu| share a cluster"""
    order = np.argsort(mu)
    out = [[int(order[0])]]
    for i, j in zip(order[:-1], order[1:]):
        if (mu[j] - mu[i]) < gap * max(abs(mu[i]), abs(mu[j])):
            out[-1].append(int(j))
        else:
            out.append([int(j)])
    return out


def cluster_of(index, groups):
    for g in groups:
        if index in g:
            return g
    raise IndexError(index)


def cluster_gap(mu, group):
    """distance of the cluster `group` from the rest of mu"""
    rest = np.delete(mu, group)
    return float(np.abs(rest[:, None] - mu[group][None, :]).min())


def subspace_distance(x, basis, Kf):
    """|| x - Q Q^T K x ||_K / || x ||_K for the K-orthonormal columns Q of `basis`: the sine of the K-angle between x and their span"""
    Kx = Kf @ x
    r = x - basis @ (basis.T @ Kx)
    return float(np.sqrt((r @ (Kf @ r)) / (x @ Kx)))


# ------------------------------------------------------------------ the cases of tests/test_gpu_buckling.py

class Case:
    """A small buckling problem and its dense reference.  Fields: xyz, tri, quad, sec, (nu, E, t), mask, loads (n, 6) or None,
    u (n, 6): the prestress displacements -- the oracle's own solution under `loads`, or a given field."""

    def __init__(self, xyz, tri, quad, sec, material, mask, loads=None, u=None):
        self.xyz, self.tri, self.quad, self.sec, self.material = xyz, tri, quad, sec, material
        self.mask, self.loads = mask, loads
        self.n = len(xyz)
        self.K = stiffness(xyz, tri, quad, *material, mask, sec)
        if u is None:
            u = np.linalg.solve(self.K, np.where(pr.fixed_dofs(mask), 0.0, loads.ravel())).reshape(-1, 6)
        self.u = u
        self._ref = None

    def reference(self, tie):
        """(mu ordered, V K-orthonormal, free, Kf) of the dense pencil, computed once"""
        if self._ref is None:
            co = element_coefficients(self.xyz, self.tri, self.quad, self.u, *self.material, sec=self.sec)
            mu, V, free = pencil(self.K, dense_KG(self.n, co), self.mask, tie)
            Kf = self.K[np.ix_(free, free)]
            self._ref = (mu, V, free, 0.5 * (Kf + Kf.T))
        return self._ref


def flat_panel_case():
    """the flat 0.3-jittered 7 x 5 panel, simply supported (w on all edges, u on x = 0, v at the first node), a uniaxial edge load on
    x = LX"""
    xyz, tri = pr.panel()
    mask = np.zeros(len(xyz), np.uint8)
    edge = np.unique(np.concatenate([pr.edge_nodes(xyz, 0, 0.0), pr.edge_nodes(xyz, 0, pr.LX), pr.edge_nodes(xyz, 1, 0.0), pr.edge_nodes(xyz, 1, pr.LY)]))
    mask[edge] |= 0x04
    mask[pr.edge_nodes(xyz, 0, 0.0)] |= 0x01
    mask[0] |= 0x02
    loads = np.zeros((len(xyz), 6))
    tip = pr.edge_nodes(xyz, 0, pr.LX)
    tip = tip[np.argsort(xyz[tip, 1])]
    for p, q in zip(tip[:-1], tip[1:]):
        share = -0.5 * abs(xyz[q, 1] - xyz[p, 1]) * 100.0
        loads[p, 0] += share
        loads[q, 0] += share
    return Case(xyz, tri, None, None, (rs.NU, rs.E, rs.T), mask, loads=loads)


def shear_plate_case(t=0.05, gamma=1e-4):
    """an 8 x 8 QUAD4 plate of side 1, u, v, w fixed on all edges, under the uniform shear strain gamma given as a displacement field"""
    xyz, tri, quad = plate(8, "q")
    mask = np.zeros(len(xyz), np.uint8)
    mask[boundary(xyz)] = 0x07
    u = np.zeros((len(xyz), 6))
    u[:, 0] = 0.5 * gamma * xyz[:, 1]
    u[:, 1] = 0.5 * gamma * xyz[:, 0]
    return Case(xyz, None, quad, None, (rs.NU, rs.E, t), mask, u=u)


def sections_panel_case():
    """the lifted panel with three sections, clamped on x = 0, under seeded random in-plane loads: a mixed-sign spectrum"""
    from tests.helpers import sections
    xyz, tri = pr.panel(lift=True)
    sec = (sections.THREE, sections.strips_of(xyz, tri), None)
    mask = np.zeros(len(xyz), np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    loads = np.zeros((len(xyz), 6))
    loads[:, :2] = np.random.default_rng(77).uniform(-100.0, 100.0, (len(xyz), 2))
    return Case(xyz, tri, None, sec, (rs.NU, rs.E, rs.T), mask, loads=loads)


CASES = {"flat_panel": flat_panel_case, "shear_plate": shear_plate_case, "sections_panel": sections_panel_case}


# ------------------------------------------------------------------ the plate of the closed forms

def plate(n, kind, a=1.0, jitter=0.0, seed=5):
    """square plate of side a in the x-y plane, n x n cells: (xyz, tri, quad); kind "t" (cells split alternately) or "q"""
    h = a / n
    jj, ii = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    xyz = np.stack([ii.ravel() * h, jj.ravel() * h, np.zeros((n + 1) ** 2)], axis=1)
    if jitter:
        rng = np.random.default_rng(seed)
        inner = ((ii > 0) & (ii < n) & (jj > 0) & (jj < n)).ravel()
        xyz[inner, :2] += jitter * h * rng.uniform(-1.0, 1.0, (inner.sum(), 2))
    tri, quad = [], []
    for j in range(n):
        for i in range(n):
            p, q, r, s = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i
            if kind == "q":
                quad.append([p, q, r, s])
            else:
                tri += [[p, q, r], [p, r, s]] if (i + j) % 2 == 0 else [[p, q, s], [q, r, s]]
    return xyz, (np.array(tri, np.int32) if tri else None), (np.array(quad, np.int32) if quad else None)


def boundary(xyz, a=1.0, tol=1e-12):
    x, y = xyz[:, 0], xyz[:, 1]
    return np.flatnonzero((np.abs(x) <= tol) | (np.abs(x - a) <= tol) | (np.abs(y) <= tol) | (np.abs(y - a) <= tol))


def plate_D(E, nu, t):
    return E * t ** 3 / (12.0 * (1.0 - nu * nu))


def edge_load_x(xyz, tri, quad, a=1.0, per_length=-1.0):
    """consistent nodal forces of a uniform edge traction Nxx = per_length on x = a and its opposite on x = 0 (linear edges:
    half the segment's share to each end node): (n, 6)"""
    f = np.zeros((len(xyz), 6))
    for x0, sign in ((a, 1.0), (0.0, -1.0)):
        nodes = pr.edge_nodes(xyz, 0, x0)
        nodes = nodes[np.argsort(xyz[nodes, 1])]
        for p, q in zip(nodes[:-1], nodes[1:]):
            share = 0.5 * abs(xyz[q, 1] - xyz[p, 1]) * per_length * sign
            f[p, 0] += share
            f[q, 0] += share
    return f
