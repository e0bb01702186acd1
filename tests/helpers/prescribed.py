"""Prescribed displacements and support reactions: the reference of the tests, built on tests/helpers/oracle.py only.

With u = u_h + u_bar (u_bar: the prescribed values at the fixed dofs, 0 elsewhere):
    K_unc  = oracle.assemble(..., dirichlet=None)          the stiffness without constraints
    K_c    = oracle.assemble(..., dirichlet=mask)          the constrained system (zero rows / columns, counting diagonal)
    rhs    = mask(F - K_unc u_bar)
    u_ref  = oracle.refined_solve(K_c, rhs) + u_bar
    r_ref  = K_unc u - loads                               reactions at fixed dofs, the negative residual at free ones
A sectioned shell takes both matrices from tests/helpers/sections.split_sum (the oracle section by section).
"""
import numpy as np

from tests.helpers import oracle, sections

NO_TRIS = np.zeros((0, 3), np.int32)
NO_QUADS = np.zeros((0, 4), np.int32)

# the panel of the issue's CPU run
LX, LY, NX, NY = 3.0, 2.0, 7, 5
NU, E, T = 0.3, 2.1e5, 0.37


def panel(nx=NX, ny=NY, lx=LX, ly=LY, jitter=0.3, seed=11, lift=False):
    """nx x ny cells of lx x ly, split into triangles alternately, interior nodes moved by up to `jitter` of a cell (fixed seed);
    lift: onto z = 0.3 sin 3x cos 2y.  Node j * (nx + 1) + i.  Returns (xyz, tri)."""
    hx, hy = lx / nx, ly / ny
    jj, ii = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    xyz = np.stack([ii.ravel() * hx, jj.ravel() * hy, np.zeros((nx + 1) * (ny + 1))], axis=1)
    rng = np.random.default_rng(seed)
    inner = ((ii > 0) & (ii < nx) & (jj > 0) & (jj < ny)).ravel()
    xyz[inner, 0] += jitter * hx * rng.uniform(-1.0, 1.0, inner.sum())
    xyz[inner, 1] += jitter * hy * rng.uniform(-1.0, 1.0, inner.sum())
    if lift:
        xyz[:, 2] = 0.3 * np.sin(3.0 * xyz[:, 0]) * np.cos(2.0 * xyz[:, 1])
    tri = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            tri += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return xyz, np.array(tri, dtype=np.int32)


def edge_nodes(xyz, axis, value, tol=1e-12):
    return np.flatnonzero(np.abs(xyz[:, axis] - value) <= tol)


def fixed_dofs(mask):
    """boolean (6 n,): the dofs the Dirichlet mask fixes"""
    mask = np.asarray(mask, dtype=np.uint8)
    return ((mask[:, None] >> np.arange(6)) & 1).astype(bool).ravel()


def matrices(xyz, tri, quad, mat, mask, sec=None):
    """(K_unc, K_c), each (rowptr, colidx, vals).  mat: an oracle.material; sec = (sections, tri_section, quad_section) instead:
    a sectioned shell."""
    tri = NO_TRIS if tri is None else tri
    quad = NO_QUADS if quad is None else quad
    if sec is not None:
        return (sections.split_sum(xyz, tri, quad, sec[0], sec[1], sec[2], None),
                sections.split_sum(xyz, tri, quad, sec[0], sec[1], sec[2], mask))
    pattern = oracle.bsr_pattern(len(xyz), tri, quad)
    return (oracle.assemble(xyz, tri, quad, mat, None, None, pattern=pattern)[:3],
            oracle.assemble(xyz, tri, quad, mat, mask, None, pattern=pattern)[:3])


def row_scale(K, x):
    """S_a = sum_b max|K_ab| * ||x_b||_1 per node row a, from the oracle's blocks"""
    rowptr, colidx, vals = K
    x1 = np.abs(np.asarray(x, dtype=np.float64).reshape(-1, 6)).sum(axis=1)
    per_block = np.abs(vals).reshape(len(colidx), -1).max(axis=1) * x1[colidx]
    return np.add.reduceat(per_block, rowptr[:-1])


def reactions(K_unc, u, loads):
    """r = K_unc u - loads, (n, 6)"""
    return (oracle.spmv(*K_unc, np.asarray(u, dtype=np.float64).ravel()) - np.asarray(loads, dtype=np.float64).ravel()).reshape(-1, 6)


class Reference:
    """u_ref, r_ref and the scales of one load case"""

    def __init__(self, xyz, tri, quad, mat, mask, loads, ubar, sec=None):
        n = len(xyz)
        self.mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self.fixed = fixed_dofs(self.mask)
        self.loads = np.zeros((n, 6)) if loads is None else np.asarray(loads, dtype=np.float64).reshape(n, 6)
        self.ubar = np.where(self.fixed, np.zeros(6 * n) if ubar is None else np.asarray(ubar, dtype=np.float64).ravel(), 0.0)
        self.K_unc, self.K_c = matrices(xyz, tri, quad, mat, self.mask, sec)
        self.rhs = np.where(self.fixed, 0.0, self.loads.ravel() - oracle.spmv(*self.K_unc, self.ubar))
        self.u = (oracle.refined_solve(*self.K_c, self.rhs) + self.ubar).reshape(n, 6)
        self.r = reactions(self.K_unc, self.u, self.loads)

    def scale(self, x):
        return row_scale(self.K_unc, x)


# ------------------------------------------------------------------ load cases shared by the CPU and the GPU tests

def membrane_patch(eps=1e-3):
    """the jittered panel, every boundary node clamped (0x3F) onto u = eps x, v = -nu eps y: uniaxial stress E eps along x.
    Returns (xyz, tri, mask, ubar (n, 6), exact (n, 6))."""
    xyz, tri = panel()
    exact = np.zeros((len(xyz), 6))
    exact[:, 0] = eps * xyz[:, 0]
    exact[:, 1] = -NU * eps * xyz[:, 1]
    boundary = (np.abs(xyz[:, 0]) < 1e-12) | (np.abs(xyz[:, 0] - LX) < 1e-12) | (np.abs(xyz[:, 1]) < 1e-12) | (np.abs(xyz[:, 1] - LY) < 1e-12)
    mask = np.where(boundary, 0x3F, 0).astype(np.uint8)
    ubar = np.where(boundary[:, None], exact, 0.0)
    return xyz, tri, mask, ubar, exact


def cantilever(w_tip=0.01):
    """the jittered panel clamped at x = 0, w = w_tip prescribed on the edge x = LX (mask bit 2 only there).
    Returns (xyz, tri, mask, ubar, tip nodes)."""
    xyz, tri = panel()
    mask = np.zeros(len(xyz), np.uint8)
    mask[edge_nodes(xyz, 0, 0.0)] = 0x3F
    tip = edge_nodes(xyz, 0, LX)
    mask[tip] = 0x04
    ubar = np.zeros((len(xyz), 6))
    ubar[tip, 2] = w_tip
    return xyz, tri, mask, ubar, tip


def supported_plate(delta=0.01):
    """the jittered panel simply supported on its four edges (w fixed; u, v fixed at the corner node 0, v at the corner NX), the
    edge y = LY moved to w = delta.  Returns (xyz, tri, mask, ubar)."""
    xyz, tri = panel()
    mask = np.zeros(len(xyz), np.uint8)
    for axis, value in ((0, 0.0), (0, LX), (1, 0.0), (1, LY)):
        mask[edge_nodes(xyz, axis, value)] |= 0x04
    mask[0] |= 0x03
    mask[NX] |= 0x02
    ubar = np.zeros((len(xyz), 6))
    ubar[edge_nodes(xyz, 1, LY), 2] = delta
    return xyz, tri, mask, ubar


def mixed_moved_edge(move=(1e-3, 2e-3, 3e-3)):
    """the mixed quadrilateral + triangle patch of tests/helpers/sections.mixed_patch (its mesh only), the clamped edge moved by
    `move`.  Returns (xyz, tri, quad, mask, ubar)."""
    c = sections.mixed_patch()
    ubar = np.zeros((c.n_nodes, 6))
    ubar[c.dmask != 0, :3] = move
    return c.xyz, c.tri, c.quad, c.dmask.copy(), ubar


def strip33():
    """33 nodes in a strip (11 x 3 nodes): the second slice holds one row.  Returns (xyz, tri)."""
    return panel(nx=10, ny=2, lx=5.0, ly=1.0, jitter=0.2, seed=5, lift=True)
