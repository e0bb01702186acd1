"""Thermal loads (femshell_set_expansion, femshell_set_thermal): the reference of the tests, numpy in longdouble, written from the
definition of include/femshell.h on top of the Gauss-point operators of tests/helpers/resultants.py, not from the kernel.

Per element (Tm, Tg): Tm the temperature change of the mid-surface, Tg = T_top - T_bottom, top at z = +t/2 along the element's ez.
Free thermal state in the element frame, kappa = (w,xx, w,yy, 2 w,xy):
    eps0 = alpha Tm (1, 1, 0),   kappa0 = -(alpha Tg / t) (1, 1, 0)
Equivalent nodal loads, with the operators and weights the stiffness uses (resultants.tri3_operators restated="twofold",
resultants.quad4_operators relative=True, both in longdouble):
    f_m = sum_g w_g Bm_g^T (t Dm eps0),   f_p = sum_g w_g Bp_g^T (Dp kappa0)
local (u, v | w, tx, ty) per node, to global axes with the frame (rotations tx = w,y, ty = -w,x; the drilling row gets nothing).
Beside every value its scale, the same sum with the absolute value of every term, carried through the rotation with |trafo|:
a device result agrees when |out - ref| <= 1e-12 scale, entry by entry, and is exactly zero where the scale is.
"""
import numpy as np

from tests.helpers import oracle, resultants as rs

LD = np.longdouble
TINY = rs.TINY


def free_strains(alpha, t, Tm, Tg, work=LD):
    """(eps0, kappa0) in `work`"""
    alpha, t, Tm, Tg = work(alpha), work(t), work(Tm), work(Tg)
    one = np.array([1, 1, 0], dtype=work)
    return alpha * Tm * one, -(alpha * Tg / t) * one


def element_operators(xyz_e, flags=oracle.REF_DEFAULT, work=LD):
    xyz_e = np.asarray(xyz_e, dtype=np.float64)
    if len(xyz_e) == 3:
        return rs.tri3_operators(xyz_e, flags, work, restated="twofold")
    return rs.quad4_operators(xyz_e, work, relative=True)


def element_vector(xyz_e, nu, E, t, alpha, Tm, Tg, flags=oracle.REF_DEFAULT, work=LD, with_local=False):
    """(f, scale), each (nn, 6) in `work`, global axes: the equivalent nodal loads of one element and their absolute-sum scale"""
    nn = len(xyz_e)
    ops = element_operators(xyz_e, flags, work)
    T = ops["trafo"]
    tDm, Dp = rs.plane_material(nu, E, t, work)
    eps0, kap0 = free_strains(alpha, t, Tm, Tg, work)
    sm, sp = tDm @ eps0, Dp @ kap0
    fm = sum(w * (B.T @ sm) for w, B in zip(ops["wm"], ops["Bm"]))
    fp = sum(w * (B.T @ sp) for w, B in zip(ops["wp"], ops["Bp"]))
    am = sum(abs(w) * (np.abs(B).T @ np.abs(sm)) for w, B in zip(ops["wm"], ops["Bm"]))
    ap = sum(abs(w) * (np.abs(B).T @ np.abs(sp)) for w, B in zip(ops["wp"], ops["Bp"]))
    loc, aloc = np.zeros((nn, 6), work), np.zeros((nn, 6), work)
    for src, dst in ((fm, loc), (am, aloc)):
        dst[:, 0:2] = src.reshape(nn, 2)
    for src, dst in ((fp, loc), (ap, aloc)):
        p = src.reshape(nn, 3)
        dst[:, 2] = p[:, 0]
        dst[:, 3:5] = p[:, 1:]
    f = np.concatenate([loc[:, :3] @ T, loc[:, 3:] @ T], axis=1)
    s = np.concatenate([aloc[:, :3] @ np.abs(T), aloc[:, 3:] @ np.abs(T)], axis=1)
    if with_local:
        return f, s, loc
    return f, s


def _kinds(tri, quad, tri_temp, quad_temp):
    for conn, temp, nn, which in ((tri, tri_temp, 3, 1), (quad, quad_temp, 4, 2)):
        if conn is None or len(conn) == 0:
            continue
        conn = np.asarray(conn).reshape(-1, nn)
        temp = np.zeros((len(conn), 2)) if temp is None else np.asarray(temp, dtype=np.float64).reshape(len(conn), 2)
        yield conn, temp, which


def material_of(e, which, nu, E, t, alpha, sec=None, sec_alpha=None):
    """(nu, E, t, alpha) of element e of kind `which` (1 triangles, 2 quadrilaterals)"""
    if sec is None:
        return nu, E, t, alpha
    s = int(sec[which][e])
    m = np.asarray(sec[0], dtype=np.float64).reshape(-1, 3)[s]
    return m[0], m[1], m[2], (alpha if sec_alpha is None else float(np.asarray(sec_alpha)[s]))


def load_vector(xyz, tri=None, quad=None, tri_temp=None, quad_temp=None, alpha=0.0, nu=rs.NU, E=rs.E, t=rs.T, sec=None, sec_alpha=None,
                flags=oracle.REF_DEFAULT, work=LD):
    """(T, scale), each (n_nodes, 6) float64: the thermal load vector summed in `work`, and the scale of every entry"""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    Tv, S = np.zeros((n, 6), work), np.zeros((n, 6), work)
    for conn, temp, which in _kinds(tri, quad, tri_temp, quad_temp):
        for e, c in enumerate(conn):
            m = material_of(e, which, nu, E, t, alpha, sec, sec_alpha)
            f, s = element_vector(xyz[c], m[0], m[1], m[2], m[3], temp[e, 0], temp[e, 1], flags, work)
            Tv[c] += f
            S[c] += s
    return Tv.astype(np.float64), S.astype(np.float64)


def bound_ratio(out, ref, scale, tol=TINY):
    """max |out - ref| / (tol scale) over all entries; an entry whose scale is zero must agree exactly"""
    diff = np.abs(np.asarray(out, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    scale = np.asarray(scale, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, diff / (tol * scale), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def cst_closed_form(xyz_e, nu, E, t, alpha, Tm, work=LD):
    """(3, 3): f_m of a triangle's nodes in global axes -- N_T / 2 times the in-plane normal of the side opposite the node,
    scaled by the side's length: N_T / 2 (n x side), n the unit normal of the triangle, the side taken counter-clockwise.  The
    normal is the one that points from the side towards the node, outward AT THE NODE: a heated element pushes its nodes apart
    (A grad N_i is half that vector; the normal that leaves the triangle through the side is its negative)."""
    X = np.asarray(xyz_e, dtype=np.float64).astype(work)
    nT = work(E) * work(t) * work(alpha) * work(Tm) / (1 - work(nu))
    nrm = np.cross(X[1] - X[0], X[2] - X[0])
    nrm = nrm / np.sqrt(nrm @ nrm)
    out = np.zeros((3, 3), work)
    for i in range(3):
        side = X[(i + 2) % 3] - X[(i + 1) % 3]  # from node i + 1 to node i + 2: the side opposite node i
        out[i] = nT / 2 * np.cross(nrm, side)
    return out


def random_temps(n_tri, n_quad, seed=5):
    """seeded (tri_temp, quad_temp), rows (Tm, Tg) of different size; None for an absent kind"""
    rng = np.random.default_rng(seed)
    tt = rng.uniform(-1.0, 1.0, (n_tri, 2)) * [80.0, 25.0] if n_tri else None
    qt = rng.uniform(-1.0, 1.0, (n_quad, 2)) * [80.0, 25.0] if n_quad else None
    return tt, qt


# ------------------------------------------------------------------ the free state and the meshes it is an identity on

def isosceles_panel(nx=6, ny=4, h=0.5):
    """nx x ny square cells of side h in the plane z = 0, each split into two right-isosceles triangles (alternately): (xyz, tri)"""
    from tests.helpers import prescribed as pr
    return pr.panel(nx=nx, ny=ny, lx=nx * h, ly=ny * h, jitter=0.0)


def rectangle_panel(nx=5, ny=4, hx=0.6, hy=0.4):
    """nx x ny rectangular quadrilaterals in the plane z = 0, counter-clockwise: (xyz, quad)"""
    jj, ii = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    xyz = np.stack([ii.ravel() * hx, jj.ravel() * hy, np.zeros((nx + 1) * (ny + 1))], axis=1)
    quad = [[j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i] for j in range(ny) for i in range(nx)]
    return xyz, np.array(quad, dtype=np.int32)


def free_state(xyz, alpha, t, Tm, Tg, x0=(0.0, 0.0)):
    """(n, 6): the displacement of a flat shell in the plane z = 0 (normal +z) that expands freely under uniform (Tm, Tg):
    u = alpha Tm (x - x0), w = -(alpha Tg / 2t) (x^2 + y^2), rotations (w,y, -w,x) as resultants.to_local reads them"""
    xyz = np.asarray(xyz, dtype=np.float64)
    x, y = xyz[:, 0], xyz[:, 1]
    k = alpha * Tg / t
    u = np.zeros((len(xyz), 6))
    u[:, 0] = alpha * Tm * (x - x0[0])
    u[:, 1] = alpha * Tm * (y - x0[1])
    u[:, 2] = -0.5 * k * (x * x + y * y)
    u[:, 3] = -k * y
    u[:, 4] = k * x
    return u


def local_dofs(T, u_e, work=LD):
    """(dm (2 nn,), dp (3 nn,)): the local membrane and plate values of an element's nodal displacements, as element_resultants"""
    u_e = np.asarray(u_e, dtype=work)
    ul, rl = u_e[:, :3] @ T.T, u_e[:, 3:] @ T.T
    return ul[:, :2].reshape(-1), np.stack([ul[:, 2], rl[:, 0], rl[:, 1]], axis=1).reshape(-1)


def model_bytes(n_listed, n_nodes, n_own, sections=False):
    """the byte model of femshell_time_kernel(FEMSHELL_KERNEL_ELEMENT_THERMAL): per listed element 16 B of node ids, 4 B of element
    index, 16 B of temperatures (4 B of section index with sections); 24 B of coordinates per node; 48 B of base read and 48 B
    written per owned row"""
    return (16.0 + 4.0 + 16.0 + (4.0 if sections else 0.0)) * n_listed + 24.0 * n_nodes + 96.0 * n_own


# ------------------------------------------------------------------ the stress state of a heated shell

def element_resultants(xyz_e, u_e, nu, E, t, alpha, Tm, Tg, flags=oracle.REF_DEFAULT, work=LD):
    """(out[14], scale[14]) float64 as resultants.element_resultants, with N_loc = t Dm (eps - eps0), M_loc = -Dp (kappa - kappa0);
    the scales gain |t Dm eps0| and |Dp kappa0|"""
    nn = len(xyz_e)
    ops = element_operators(xyz_e, flags, work)
    T = ops["trafo"]
    dm, dp = local_dofs(T, np.asarray(u_e, dtype=np.float64).reshape(nn, 6), work)
    tDm, Dp = rs.plane_material(nu, E, t, work)
    eps0, kap0 = free_strains(alpha, t, Tm, Tg, work)
    DBm = tDm @ rs.mean_operator(ops["Bm"], ops["wm"])
    DBp = -(Dp @ rs.mean_operator(ops["Bp"], ops["wp"]))
    N, M = DBm @ dm - tDm @ eps0, DBp @ dp + Dp @ kap0
    SN = np.abs(DBm) @ np.abs(dm) + np.abs(tDm) @ np.abs(eps0)
    SM = np.abs(DBp) @ np.abs(dp) + np.abs(Dp) @ np.abs(kap0)
    t = work(t)
    top, bot = N / t + 6 * M / (t * t), N / t - 6 * M / (t * t)
    out = np.concatenate([rs.to_global(T, N), rs.to_global(T, M), [rs.von_mises(top), rs.von_mises(bot)]])
    s_vm = 4 * (SN / t + 6 * SM / (t * t)).max()
    scale = np.concatenate([rs.to_global(np.abs(T), SN), rs.to_global(np.abs(T), SM), [s_vm, s_vm]])
    return out.astype(np.float64), scale.astype(np.float64)


def mesh_resultants(xyz, tri, quad, u, tri_temp, quad_temp, alpha, nu=rs.NU, E=rs.E, t=rs.T, sec=None, sec_alpha=None,
                    flags=oracle.REF_DEFAULT, work=LD):
    """(out, scale), each (n_tri + n_quad, 14): triangles in their order, then quadrilaterals"""
    xyz = np.asarray(xyz, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64).reshape(len(xyz), 6)
    out, scale = [], []
    for conn, temp, which in _kinds(tri, quad, tri_temp, quad_temp):
        for e, c in enumerate(conn):
            m = material_of(e, which, nu, E, t, alpha, sec, sec_alpha)
            o, s = element_resultants(xyz[c], u[c], m[0], m[1], m[2], m[3], temp[e, 0], temp[e, 1], flags, work)
            out.append(o)
            scale.append(s)
    return np.array(out).reshape(-1, 14), np.array(scale).reshape(-1, 14)


def clamped_closed_form(xyz_e, nu, E, t, alpha, Tm, Tg, flags=oracle.REF_DEFAULT, work=LD):
    """[14]: the stress state of an element held at u = 0 -- N_loc = -N_T (1,1,0), M_loc = -M_T (1,1,0) rotated to global axes,
    sigma_top/bot = -(E alpha / (1 - nu)) (Tm +- Tg / 2) on the in-plane diagonals and its magnitude as von Mises value"""
    T = element_operators(xyz_e, flags, work)["trafo"]
    nu, E, t, alpha, Tm, Tg = (work(v) for v in (nu, E, t, alpha, Tm, Tg))
    nT, mT = E * t * alpha * Tm / (1 - nu), E * t * t * alpha * Tg / (12 * (1 - nu))
    one = np.array([1, 1, 0], dtype=work)
    s = E * alpha / (1 - nu)
    return np.concatenate([rs.to_global(T, -nT * one), rs.to_global(T, -mT * one),
                           [abs(s * (Tm + Tg / 2)), abs(s * (Tm - Tg / 2))]]).astype(np.float64)
