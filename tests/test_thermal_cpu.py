"""CPU tests of tests/helpers/thermal.py, the long-double reference of the thermal loads, against closed forms: the CST closed
form of the membrane part, self-equilibrium of the load vector, and the patch condition under which K u_free = T is an identity.
No GPU call is made."""
import numpy as np
import pytest

from tests.helpers import oracle, prescribed as pr, resultants as rs, thermal as th

LD = np.longdouble
ALPHA = 1.2e-5


def test_membrane_part_of_a_triangle_is_half_the_outward_side_normal():
    """f_m at a node = N_T / 2 (unit normal x side opposite): on every triangle of the lifted, jittered panel, with Tg = 0 the
    translations of the helper's element vector, to 1e-12 of their scale; the rotational rows are exactly zero then"""
    xyz, tri = pr.panel(lift=True)
    rng = np.random.default_rng(2)
    worst = 0.0
    for c in tri:
        Tm = rng.uniform(-80.0, 80.0)
        f, s = th.element_vector(xyz[c], rs.NU, rs.E, rs.T, ALPHA, Tm, 0.0)
        closed = th.cst_closed_form(xyz[c], rs.NU, rs.E, rs.T, ALPHA, Tm)
        worst = max(worst, th.bound_ratio(f[:, :3].astype(np.float64), closed.astype(np.float64), s[:, :3].astype(np.float64)))
        assert not f[:, 3:].any()
    print("CST closed form: max |f_m - closed| / (1e-12 scale) = %.3e" % worst)
    assert worst <= 1.0


def _equilibrium(xyz, tri, quad, sec=None, sec_alpha=None):
    """(force residual / scale, moment residual / scale) of the load vector under random (Tm, Tg), in long double"""
    nt, nq = (0 if tri is None else len(tri)), (0 if quad is None else len(quad))
    tt, qt = th.random_temps(nt, nq)
    xyz = np.asarray(xyz, dtype=np.float64)
    Tv, S = np.zeros((len(xyz), 6), LD), np.zeros((len(xyz), 6), LD)
    for conn, temp, which in th._kinds(tri, quad, tt, qt):
        for e, c in enumerate(conn):
            m = th.material_of(e, which, rs.NU, rs.E, rs.T, ALPHA, sec, sec_alpha)
            f, s = th.element_vector(xyz[c], m[0], m[1], m[2], m[3], temp[e, 0], temp[e, 1])
            Tv[c] += f
            S[c] += s
    X = xyz.astype(LD)
    force = np.abs(Tv[:, :3].sum(axis=0))
    force_scale = S[:, :3].sum(axis=0)
    moment = np.abs((np.cross(X, Tv[:, :3]) + Tv[:, 3:]).sum(axis=0))
    # |x x f| <= |x| x |f| component by component, with the scales in place of |f|
    aX = np.abs(X)
    moment_scale = (np.stack([aX[:, 1] * S[:, 2] + aX[:, 2] * S[:, 1], aX[:, 2] * S[:, 0] + aX[:, 0] * S[:, 2],
                              aX[:, 0] * S[:, 1] + aX[:, 1] * S[:, 0]], axis=1) + S[:, 3:]).sum(axis=0)
    assert (force_scale > 0).all() and (moment_scale > 0).all()
    return float((force / force_scale).max()), float((moment / moment_scale).max())


@pytest.mark.parametrize("name", ["lifted_panel", "rectangles", "mixed_petals24", "coil300", "panel_three_sections"])
def test_the_load_vector_is_in_equilibrium_with_itself(name):
    """sum_a T_a = 0 and sum_a (x_a x T_a,force + T_a,moment) = 0 to 1e-12 of their scales: the free thermal state strains no
    rigid-body motion (B annihilates translations and rotations), whatever the temperatures and materials are"""
    if name == "rectangles":
        xyz, quad = th.rectangle_panel()
        args = (xyz, None, quad)
    else:
        xyz, tri, quad, sec, _ = rs.device_meshes()[name]()
        args = (xyz, tri, quad, sec, None if sec is None else [1.1e-5, 2.3e-5, 0.7e-5])
    rf, rm = _equilibrium(*args)
    print("self-equilibrium %-22s force %.3e  moment %.3e of their scales" % (name, rf, rm))
    assert rf <= 1e-12 and rm <= 1e-12


@pytest.mark.parametrize("kind", ["isosceles_triangles", "rectangles"])
def test_the_operators_return_the_free_strains_of_the_free_state(kind):
    """the patch condition: the helper's Gauss-point operators applied to the nodal values of u_free return (eps0, kappa0) at
    every Gauss point, on the two meshes the free-state GPU tests use (it need not hold on scalene triangles under REF_Y21)"""
    Tm, Tg = 37.0, -11.0
    if kind == "rectangles":
        xyz, conn = th.rectangle_panel()
    else:
        xyz, conn = th.isosceles_panel()
    u = th.free_state(xyz, ALPHA, rs.T, Tm, Tg, x0=(0.7, 0.3))
    eps0, kap0 = th.free_strains(ALPHA, rs.T, Tm, Tg)
    worst = 0.0
    for c in conn:
        ops = th.element_operators(xyz[c])
        dm, dp = th.local_dofs(ops["trafo"], u[c])
        for B in ops["Bm"]:
            worst = max(worst, float((np.abs(B @ dm - eps0) / (np.abs(B) @ np.abs(dm))).max()))
        for B in ops["Bp"]:
            worst = max(worst, float((np.abs(B @ dp - kap0) / (np.abs(B) @ np.abs(dp))).max()))
    print("patch condition %-20s max |B d - strain0| / (|B| |d|) = %.3e" % (kind, worst))
    assert worst <= 1e-12


def test_free_state_balances_the_load_vector_on_the_oracle_matrix():
    """K_unc u_free = T on the isosceles panel, K_unc the oracle's: the identity the free-state GPU tests stand on, to 1e-12 of
    sum |K| |u| + scale of T"""
    Tm, Tg = 37.0, -11.0
    xyz, tri = th.isosceles_panel()
    u = th.free_state(xyz, ALPHA, rs.T, Tm, Tg)
    temps = np.tile([Tm, Tg], (len(tri), 1))
    Tv, S = th.load_vector(xyz, tri, None, temps, None, ALPHA)
    K_unc, _ = pr.matrices(xyz, tri, None, oracle.material(rs.NU, rs.E, rs.T), np.zeros(len(xyz), np.uint8))
    r = pr.reactions(K_unc, u, Tv)
    scale = pr.row_scale(K_unc, u)[:, None] + S
    ratio = float((np.abs(r) / (1e-12 * scale)).max())
    print("K u_free - T: max / (1e-12 (sum |K||u| + |T|)) = %.3e" % ratio)
    assert ratio <= 1.0
