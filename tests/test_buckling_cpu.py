"""Linear buckling without a GPU: the pins of the tests' own reference (tests/helpers/buckling.py) before any device result is held
to it -- closed forms of the simply supported square plate, the sign convention under shear and tension, the structure of K_G and
its FP64 evaluation against longdouble.  Nothing here touches the library: the file passes with or without the feature."""
import numpy as np
import pytest

from tests.helpers import buckling as bk, prescribed as pr, resultants as rs

NU, E, T = 0.3, 2.1e5, 0.01  # the plate of the closed forms: a = 1
PI2D = np.pi ** 2 * bk.plate_D(E, NU, T)


def _simply_supported(xyz):
    """w on all edges; u on the line x = 1/2 and v on the line y = 1/2 (n even): the in-plane supports that leave the uniform
    uniaxial state free of reactions"""
    mask = np.zeros(len(xyz), np.uint8)
    mask[bk.boundary(xyz)] |= 0x04
    mask[pr.edge_nodes(xyz, 0, 0.5)] |= 0x01
    mask[pr.edge_nodes(xyz, 1, 0.5)] |= 0x02
    return mask


def _uniaxial(n, kind, per_length):
    """the full pipeline: edge loads, the oracle's solve, N, K_G, the dense pencil.  Returns (mu ordered, Nxx of every element)"""
    xyz, tri, quad = bk.plate(n, kind)
    mask = _simply_supported(xyz)
    K = bk.stiffness(xyz, tri, quad, NU, E, T, mask)
    f = bk.edge_load_x(xyz, tri, quad, per_length=per_length)
    u = np.linalg.solve(K, np.where(pr.fixed_dofs(mask), 0.0, f.ravel()))
    co = bk.element_coefficients(xyz, tri, quad, u, NU, E, T)
    nxx = rs.mesh_resultants(xyz, tri, quad, u, NU, E, T)[0][:, 0]
    mu, _, _ = bk.pencil(K, bk.dense_KG(len(xyz), co), mask)
    return mu, nxx


@pytest.fixture(scope="module")
def compression():
    return {(kind, n): _uniaxial(n, kind, -1.0) for kind in "tq" for n in (8, 16)}


@pytest.mark.parametrize("kind,at8,at16", [("t", 2.47e-2, 6.16e-3), ("q", 1.52e-2, 3.78e-3)])
def test_plate_under_uniaxial_compression_converges_to_the_closed_form(compression, kind, at8, at16):
    """lambda_1 -> 4 pi^2 D / a^2 like h^2 (ratio of the errors at n = 8 and 16 in [3.5, 4.5]), lambda_2 within 3 % of 1.5625
    times the closed form at n = 16; the recovered Nxx is -1"""
    ref = 4.0 * PI2D
    err = {}
    for n in (8, 16):
        mu, nxx = compression[(kind, n)]
        lam = bk.factors(mu, 2)
        err[n] = (lam[0] - ref) / ref
        print("plate %s n %2d: lambda_1 / ref - 1 = %+.3e, lambda_2 / lambda_ref = %.4f, max |Nxx + 1| = %.1e" % (kind, n, err[n], lam[1] / ref, np.abs(nxx + 1.0).max()))
        assert np.abs(nxx + 1.0).max() <= 1e-10
        assert lam[0] > 0.0 and lam[1] > 0.0
    assert abs(err[8] - at8) <= 0.01 * at8 and abs(err[16] - at16) <= 0.01 * at16  # the table of DESIGN.md 8g
    assert 3.5 <= err[8] / err[16] <= 4.5
    lam2 = bk.factors(compression[(kind, 16)][0], 2)[1]
    assert abs(lam2 - 1.5625 * ref) <= 0.03 * 1.5625 * ref


@pytest.mark.parametrize("kind", ["t", "q"])
def test_uniform_prestress_gives_the_factor_of_the_recovered_one(compression, kind):
    xyz, tri, quad = bk.plate(8, kind)
    mask = _simply_supported(xyz)
    K = bk.stiffness(xyz, tri, quad, NU, E, T, mask)
    co = bk.element_coefficients(xyz, tri, quad, None, NU, E, T, N_uniform=(-1.0, 0.0, 0.0))
    mu = bk.pencil(K, bk.dense_KG(len(xyz), co), mask)[0]
    assert abs(mu[0] - compression[(kind, 8)][0][0]) <= 1e-9 * abs(mu[0])


@pytest.mark.parametrize("n", [8, 16])
def test_shear_gives_a_signed_pair(n):
    """uniform Nxy = 1, u, v, w fixed on all edges, QUAD4: the spectrum is a +- pair, equal in magnitude to 1e-9, between the
    classical 9.34 and 10.4 pi^2 D / a^2; the positive one is returned first"""
    xyz, tri, quad = bk.plate(n, "q")
    mask = np.zeros(len(xyz), np.uint8)
    mask[bk.boundary(xyz)] = 0x07
    K = bk.stiffness(xyz, tri, quad, NU, E, T, mask)
    co = bk.element_coefficients(xyz, tri, quad, None, NU, E, T, N_uniform=(0.0, 0.0, 1.0))
    mu = bk.pencil(K, bk.dense_KG(len(xyz), co), mask)[0]
    lam = bk.factors(mu, 2) / PI2D
    print("shear n %2d: lambda / (pi^2 D) = %+.4f, %+.4f" % (n, lam[0], lam[1]))
    assert lam[0] * lam[1] < 0.0
    assert abs(abs(lam[0]) - abs(lam[1])) <= 1e-9 * abs(lam[0])
    assert 9.34 <= abs(lam[0]) <= 10.4 and 9.34 <= abs(lam[1]) <= 10.4


def test_ordering_puts_the_positive_factor_first_on_exact_ties():
    K = np.eye(12)
    KG = np.zeros((12, 12))
    KG[0, 0], KG[1, 1], KG[2, 2] = 0.5, -0.5, 0.25
    mu = bk.pencil(K, KG, np.zeros(2, np.uint8))[0]
    assert list(bk.factors(mu, 3)) == [2.0, -2.0, -4.0]


def test_tension_has_no_positive_factor():
    mu, nxx = _uniaxial(8, "t", +1.0)
    assert np.abs(nxx - 1.0).max() <= 1e-10
    assert (bk.factors(mu, 6) < 0.0).all()


def _mesh_case(name):
    xyz, tri, quad, sec, _ = rs.device_meshes()[name]()
    u = rs.random_u(len(xyz))
    return xyz, tri, quad, sec, u


@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24", "panel_three_sections"])
def test_KG_is_symmetric_and_annihilates_rigid_translations(name):
    xyz, tri, quad, sec, u = _mesh_case(name)
    n = len(xyz)
    co = bk.element_coefficients(xyz, tri, quad, u, rs.NU, rs.E, rs.T, sec)
    KG = bk.dense_KG(n, co)
    assert np.abs(KG - KG.T).max() <= 8.0 * np.finfo(np.float64).eps * np.abs(KG).max()  # (the two orders of grad^T N grad)
    rot = np.arange(6 * n) % 6 >= 3
    assert not KG[rot].any() and not KG[:, rot].any()
    X = np.zeros((3, n, 6))
    X[0, :, :3] = (1.0, 0.0, 0.0)
    X[1, :, :3] = (0.3, -2.0, 0.7)
    X[2, :, :3] = (0.0, 0.0, 1.0)
    Y, Ta = bk.product(n, co, X)
    ratio = bk.bound_ratio(Y, np.zeros_like(Y), Ta)
    print("K_G times a rigid translation, %s: max |Y| / (1e-12 T_a) = %.3e" % (name, ratio))
    assert ratio <= 1.0
    assert np.abs(KG).max() > 0.0


@pytest.mark.parametrize("name", list(rs.device_meshes()))
def test_fp64_product_against_longdouble(name):
    """the FP64 evaluation of the definition against its longdouble evaluation, within 1e-12 T_a: the reference the device is
    held to is not the limit"""
    xyz, tri, quad, sec, u = _mesh_case(name)
    n = len(xyz)
    X = np.random.default_rng(31).uniform(-1.0, 1.0, (2, n, 6))
    Y, Ta = bk.product(n, bk.element_coefficients(xyz, tri, quad, u, rs.NU, rs.E, rs.T, sec), X)
    Yl, _ = bk.product(n, bk.element_coefficients(xyz, tri, quad, u, rs.NU, rs.E, rs.T, sec, dtype=np.longdouble), X, dtype=np.longdouble)
    ratio = bk.bound_ratio(Y, Yl, Ta)
    print("fp64 vs longdouble %-28s max |Y - Y_ld| / (1e-12 T_a) = %.3e" % (name, ratio))
    assert ratio <= 1.0 and Ta.max() > 0.0


def test_clusters_and_subspace_distance():
    mu = np.array([5.0, -5.0, 2.0, 2.001, -1.0])
    groups = bk.clusters(mu)
    assert sorted(map(sorted, groups)) == [[0], [1], [2, 3], [4]]
    assert bk.cluster_of(3, groups) == [2, 3]
    assert abs(bk.cluster_gap(mu, [2, 3]) - 2.999) <= 1e-12
    Kf = np.diag([1.0, 2.0, 3.0])
    Q = np.array([[1.0, 0.0], [0.0, 1.0 / np.sqrt(2.0)], [0.0, 0.0]])
    assert bk.subspace_distance(Q @ np.array([3.0, -1.0]), Q, Kf) <= 1e-15
    assert abs(bk.subspace_distance(np.array([0.0, 0.0, 1.0]), Q, Kf) - 1.0) <= 1e-15
