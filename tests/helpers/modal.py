"""Modal analysis (femshell_modes): the reference of the tests, numpy and scipy only.

reference() solves K x = lambda M x on the free dofs of an exported block matrix with the lumped mass of tests/helpers/dynamics.py
by a dense scipy.linalg.eigh (a few thousand dofs at most).  clusters() groups eigenvalues whose adjacent relative gap is below
1e-2 -- inside a cluster only the subspace is defined -- and subspace_distance() measures how far a vector is from the span of a
cluster in the M inner product.  tests/test_modal_cpu.py pins the lowest eigenvalue against the closed form of the simply
supported square plate.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from tests.helpers import dynamics

CLUSTER_GAP = 1e-2


def reference(K, mass, dmask, n_pairs, shift=0.0):
    """(lam[n_pairs] ascending, X (n_pairs, 6 n) M-orthonormal and zero on the constrained dofs) of K x = lam M x on the free dofs.
    K: scipy matrix with the constraints as the assembly leaves them; mass: (n, 6); shift: eigh runs on K + shift M (a
    singular K), lam comes back with the shift subtracted."""
    m = np.asarray(mass, dtype=np.float64).ravel()
    free = dynamics.free_dofs(dmask, len(m) // 6)
    Kf = sp.csr_matrix(K)[free][:, free].toarray()
    Kf = 0.5 * (Kf + Kf.T) + shift * np.diag(m[free])
    lam, V = sla.eigh(Kf, np.diag(m[free]), subset_by_index=[0, n_pairs - 1])
    X = np.zeros((n_pairs, len(m)))
    X[:, free] = V.T
    return lam - shift, X


def clusters(lam, shift=0.0, gap=CLUSTER_GAP):
    """lists of consecutive indices: i and i + 1 share a cluster when (lam[i+1] - lam[i]) < gap * (lam[i+1] + shift)"""
    out = [[0]]
    for i in range(1, len(lam)):
        if (lam[i] - lam[i - 1]) < gap * (abs(lam[i]) + shift):
            out[-1].append(i)
        else:
            out.append([i])
    return out


def cluster_of(index, groups):
    for g in groups:
        if index in g:
            return g
    raise IndexError(index)


def subspace_distance(x, basis, mass):
    """|| x - Q Q^T M x ||_M / || x ||_M for the M-orthonormal rows Q of `basis`: the sine of the M-angle between x and their span"""
    m = np.asarray(mass, dtype=np.float64).ravel()
    x = np.asarray(x, dtype=np.float64).ravel()
    Q = np.asarray(basis, dtype=np.float64).reshape(len(basis), -1)
    r = x - Q.T @ (Q @ (m * x))
    return float(np.sqrt((r * m * r).sum() / (x * m * x).sum()))


def residual_norms(K, mass, dmask, lam, X, shift=0.0):
    """|| K x - lam M x ||_{M^-1} / (lam + shift) on the free dofs, per row of X"""
    m = np.asarray(mass, dtype=np.float64).ravel()
    free = dynamics.free_dofs(dmask, len(m) // 6)
    K = sp.csr_matrix(K)
    out = []
    for l, x in zip(lam, np.asarray(X).reshape(len(lam), -1)):
        r = (K @ x - l * m * x)[free]
        out.append(np.sqrt((r * r / m[free]).sum()) / (l + shift))
    return np.array(out)


def plate_first_eigenvalue(E, nu, t, rho, a=1.0):
    """lambda_11 = omega_11^2 of the simply supported square Kirchhoff plate of side a: 4 pi^4 D / (rho t a^4)"""
    D = E * t ** 3 / (12.0 * (1.0 - nu * nu))
    return 4.0 * np.pi ** 4 * D / (rho * t * a ** 4)
