"""Structural dynamics (femshell_set_density, femshell_dynamics_*): the reference of the tests, numpy and scipy only.

lumped_mass restates the definition of include/femshell.h; Newmark runs the method on a sparse-LU factorisation of
K_eff = K + (a0 + alpha a1) M built from an exported block matrix (constrained rows as the assembly leaves them: zero rows and
columns, the element count on the diagonal); energy evaluates v.Mv / 2 and u.Ku / 2.  tests/test_dynamics_cpu.py pins all three
against closed-form results (total mass, free fall, energy conservation).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.helpers import oracle


def _norm(v, dtype):
    """row-wise 2-norm: np.linalg.norm where it keeps the type (FP64, bit for bit what it always was), else spelt out"""
    return np.linalg.norm(v, axis=1) if dtype is np.float64 else np.sqrt((v * v).sum(axis=1))


def element_areas(xyz, tri=None, quad=None, dtype=np.float64):
    """(areas of the triangles |(b-a) x (c-a)| / 2, areas of the quadrilaterals |d1 x d2| / 2 with the diagonals d1, d2), in `dtype`"""
    xyz = np.asarray(xyz, dtype=np.float64).astype(dtype)
    at = np.zeros(0, dtype)
    aq = np.zeros(0, dtype)
    if tri is not None and len(tri):
        a, b, c = (xyz[np.asarray(tri)[:, i]] for i in range(3))
        at = 0.5 * _norm(np.cross(b - a, c - a), dtype)
    if quad is not None and len(quad):
        a, b, c, d = (xyz[np.asarray(quad)[:, i]] for i in range(4))
        aq = 0.5 * _norm(np.cross(c - a, d - b), dtype)
    return at, aq


def lumped_mass(xyz, tri, quad, rho, thickness, tri_section=None, quad_section=None, dtype=np.float64):
    """m[n_nodes, 6]: rho t A / nn on u, v, w and rho t^3/12 A / nn on tx, ty, tz from every element to each of its nn nodes.
    rho, thickness: scalars, or one entry per section with tri_section / quad_section naming every element's.  Computed and
    returned in `dtype`."""
    xyz = np.asarray(xyz, dtype=np.float64)
    m = np.zeros((len(xyz), 6), dtype)
    at, aq = element_areas(xyz, tri, quad, dtype)
    for conn, area, sec in ((tri, at, tri_section), (quad, aq, quad_section)):
        if conn is None or len(conn) == 0:
            continue
        conn = np.asarray(conn)
        nn = conn.shape[1]
        r = np.broadcast_to(np.asarray(rho, dtype=np.float64), (len(conn),)) if np.ndim(rho) == 0 else np.asarray(rho, dtype=np.float64)[np.asarray(sec)]
        t = (np.broadcast_to(np.asarray(thickness, dtype=np.float64), (len(conn),)) if np.ndim(thickness) == 0
             else np.asarray(thickness, dtype=np.float64)[np.asarray(sec)])
        r, t = r.astype(dtype), t.astype(dtype)
        for i in range(nn):
            np.add.at(m[:, :3], conn[:, i], (r * t * area / nn)[:, None])
            np.add.at(m[:, 3:], conn[:, i], (r * t ** 3 / 12.0 * area / nn)[:, None])
    return m


def free_dofs(dmask, n_nodes):
    """bool[6 n]: True where the dof is not fixed by the Dirichlet mask (None: all free)"""
    if dmask is None:
        return np.ones(6 * n_nodes, dtype=bool)
    dm = np.asarray(dmask, dtype=np.uint8)
    return (((dm[:, None] >> np.arange(6)[None, :]) & 1) == 0).ravel()


def coefficients(dt, beta=0.25, gamma=0.5):
    return (1.0 / (beta * dt * dt), gamma / (beta * dt), 1.0 / (beta * dt), 1.0 / (2.0 * beta) - 1.0, gamma / beta - 1.0,
            0.5 * dt * (gamma / beta - 2.0))


def to_matrix(bsr):
    """scipy CSR of an exported (rowptr, colidx, vals[, F]) block matrix"""
    return oracle.to_scipy(bsr[0], bsr[1], bsr[2]).tocsr()


class Newmark:
    """Newmark's method with damping alpha M on a sparse LU of K_eff.  K: scipy matrix with the constraints applied as the
    assembly applies them; m: (n, 6) lumped mass; dmask: Dirichlet mask per node or None."""

    def __init__(self, K, m, dmask, dt, beta=0.25, gamma=0.5, alpha=0.0):
        self.K = sp.csr_matrix(K)
        self.m = np.asarray(m, dtype=np.float64).ravel()
        self.free = free_dofs(dmask, len(self.m) // 6)
        self.dt, self.beta, self.gamma, self.alpha = dt, beta, gamma, alpha
        self.c = coefficients(dt, beta, gamma)
        self.shift = self.c[0] + alpha * self.c[1]
        self.Keff = (self.K + sp.diags(self.shift * self.m * self.free)).tocsc()
        self.lu = spla.splu(self.Keff)

    def begin(self, F0, u0=None, v0=None):
        n = len(self.m)
        self.u = np.zeros(n) if u0 is None else np.asarray(u0, dtype=np.float64).ravel() * self.free
        self.v = np.zeros(n) if v0 is None else np.asarray(v0, dtype=np.float64).ravel() * self.free
        F0 = np.asarray(F0, dtype=np.float64).ravel() * self.free
        with np.errstate(divide="ignore", invalid="ignore"):
            a = (F0 - self.alpha * self.m * self.v - self.K @ self.u) / self.m
        self.a = np.where(self.free & (self.m > 0.0), a, 0.0)
        return self.u.copy(), self.v.copy(), self.a.copy()

    def rhs(self, F):
        a0, a1, a2, a3, a4, a5 = self.c
        u, v, a = self.u, self.v, self.a
        return self.free * (np.asarray(F, dtype=np.float64).ravel()
                            + self.m * ((a0 * u + a2 * v + a3 * a) + self.alpha * (a1 * u + a4 * v + a5 * a)))

    def step(self, F):
        """one accepted step under the loads F (6 n): returns the new (u, v, a)"""
        a0, a1, a2, a3, a4, a5 = self.c
        b = self.rhs(F)
        u1 = self.lu.solve(b)
        u1 += self.lu.solve(b - self.Keff @ u1)  # one pass of iterative refinement: the LU's own rounding, times kappa, goes
        u1 *= self.free
        acc = a0 * (u1 - self.u) - a2 * self.v - a3 * self.a
        vel = self.v + self.dt * ((1.0 - self.gamma) * self.a + self.gamma * acc)
        self.u, self.v, self.a = u1, vel * self.free, acc * self.free
        return self.u.copy(), self.v.copy(), self.a.copy()


def recurrence(u1, u, v, a, dt, beta=0.25, gamma=0.5):
    """(a', v') of the update from u', u, v, a, and the largest term of each sum (what a bound on its rounding refers to)"""
    a0, _, a2, a3, _, _ = coefficients(dt, beta, gamma)
    acc = a0 * (u1 - u) - a2 * v - a3 * a
    vel = v + dt * ((1.0 - gamma) * a + gamma * acc)
    big_a = max(np.abs(a0 * u1).max(), np.abs(a0 * u).max(), np.abs(a2 * v).max(), np.abs(a3 * a).max())
    big_v = max(np.abs(v).max(), np.abs(dt * (1.0 - gamma) * a).max(), np.abs(dt * gamma * acc).max())
    return acc, vel, big_a, big_v


def energy(K, m, u, v):
    """(kinetic v.Mv / 2, strain u.Ku / 2); u is zero on the constrained dofs, whose diagonal entries of K do not enter"""
    u = np.asarray(u, dtype=np.float64).ravel()
    v = np.asarray(v, dtype=np.float64).ravel()
    return 0.5 * float(v @ (np.asarray(m).ravel() * v)), 0.5 * float(u @ (K @ u))


def first_period(K, m, dmask):
    """T1 = 2 pi / omega_1 of K x = omega^2 M x on the free dofs (dense: small meshes only)"""
    import scipy.linalg as sla

    free = free_dofs(dmask, len(np.asarray(m).ravel()) // 6)
    Kf = sp.csr_matrix(K)[free][:, free].toarray()
    w2 = sla.eigh(Kf, np.diag(np.asarray(m).ravel()[free]), eigvals_only=True, subset_by_index=[0, 0])[0]
    return 2.0 * np.pi / np.sqrt(w2)
