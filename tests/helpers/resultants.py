"""Element stress resultants and surface stresses (femshell_element_resultants): the reference of the tests, numpy on top of
tests/helpers/oracle.py.

Per element, from the nodal displacements u (nn x 6, global axes), 14 numbers:
    [0:6]   membrane force tensor N, global axes, xx yy zz xy yz zx
    [6:12]  moment tensor M, same order
    [12]    von Mises stress at the top surface (z = +t/2 along the element's ez), [13] at the bottom surface
with, in the element frame (rows of `trafo`: ex, ey, ez),
    N_loc = t Dm eps,  M_loc = -Dp kappa  (M = integral of sigma z dz),
    eps = (u,x, v,y, u,y + v,x),  kappa = (w,xx, w,yy, 2 w,xy)  with the rotations tx = w,y, ty = -w,x,
eps and kappa the element means of the element's own strain operators by the quadrature its stiffness uses:
    TRI3   the CST strain (constant) and the mean of Specht's curvature Y B~(g) over its three Gauss points, Y with the same
           FSO_REF_Y21 switch as the stiffness;
    QUAD4  the det-J-weighted mean over the 2 x 2 Gauss points of the bilinear membrane strain and of the DKQ curvature.  The DKQ
           operator of the stiffness is written in the section rotations beta_x = -w,x, beta_y = -w,y: what it returns is
           -(w,xx, w,yy, 2 w,xy), so its negative is the kappa above.  (The stiffness, quadratic in it, does not see the sign; the
           bending patch test of tests/test_resultants_cpu.py fixes it.)
The QUAD4 operators restate oracle/femshell_oracle.c (quad4_membrane, quad4_dkq_B, quad4_plate) in numpy; the TRI3 ones come from
the oracle itself (element_tri3 parts, specht_B), or, with restated=True, from their restatement here (tri3_frame, specht_B), which
a call with dtype=np.longdouble evaluates without rounding anything to double on the way.

Beside the values every function returns the absolute-sum scale of each: S = sum_j |(D B)_j| |d_j| for the local components,
carried through the rotation to global axes with absolute values; for the two von Mises values four times the largest scale of a
surface-stress component, S_N / t + 6 S_M / t^2 (the gradient of the von Mises form has 2-norm <= 2, times sqrt 3 from the
max-norm to the 2-norm).  A result `out` agrees with the reference when |out - ref| <= 1e-12 * scale, entry by entry.
"""
import numpy as np

from tests.helpers import oracle

TINY = 1e-12  # the bar the project holds element math to

GAUSS_TRI = ((1.0 / 6.0, 1.0 / 6.0), (2.0 / 3.0, 1.0 / 6.0), (1.0 / 6.0, 2.0 / 3.0))
VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))  # xx yy zz xy yz zx


def plane_material(nu, E, t, dtype=np.float64):
    """(t Dm, Dp) as fso_material_matrices forms them, in `dtype`"""
    nu, E, t = dtype(nu), dtype(E), dtype(t)
    D = np.array([[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]], dtype=dtype)
    return t * (E / (1 - nu * nu)) * D, (E * t ** 3 / (12 * (1 - nu * nu))) * D


# ------------------------------------------------------------------ TRI3

def specht_Y(dphi, area, flags):
    """SA:578-588, the matrix tri3_plate of the oracle and tri3_record of the device build (Y21 as coded unless the flag is cleared)"""
    x31, y31, x23, y23 = dphi[1, 0], dphi[1, 1], dphi[2, 0], dphi[2, 1]
    Y = np.array([[y23 * y23, y31 * y31, y23 * y31],
                  [x23 * x23, x31 * x31, x31 * x23],
                  [-2 * x23 * y23, (-2 * x31 * x31) if (flags & oracle.REF_Y21) else (-2 * x31 * y31), -x23 * y31 - x31 * y23]],
                 dtype=dphi.dtype)
    return Y / (4 * area * area)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product on Veltkamp's split, for the type of a and b)"""
    half = (np.finfo(type(a)).nmant + 2) // 2
    c = type(a)(2 ** half + 1)
    ah = c * a - (c * a - a)
    bh = c * b - (c * b - b)
    al, bl = a - ah, b - bh
    p = a * b
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dot2(a, b):
    """sum_i a_i b_i with the rounding errors of the products and of the partial sums carried along and added at the end: the
    result as if formed in twice the precision of the entries' type and rounded once (Ogita, Rump and Oishi's Dot2)"""
    s = c = type(a[0])(0)
    for x, y in zip(a, b):
        p, e = _two_prod(x, y)
        s, f = _two_sum(s, p)
        c = c + (e + f)
    return s + c


def cross2(a, b):
    """a x b, every component by dot2"""
    return np.array([dot2((a[1], -a[2]), (b[2], b[1])), dot2((a[2], -a[0]), (b[0], b[2])), dot2((a[0], -a[1]), (b[1], b[0]))],
                    dtype=a.dtype)


def tri3_frame(xyz, dtype=np.float64, twofold=False):
    """SA:306-341, 378-411 as tri3_frame of the oracle states it, every step in `dtype`: ex along the first edge, ez along
    (B - A) x (C - A), ey = ez x ex; node A is the local origin.  Returns (trafo (3,3), dphi (3,2): rows (12), (31), (23), area).
    twofold: the same frame from products that keep their digits on slivers and needles -- the sides are differences of doubles,
    exact in long double; their dot and cross products are formed by dot2; and the local coordinates are written with what the
    frame makes of them in exact arithmetic: ex . U = |U|, ex . V = U . V / |U|, ey . V = |U x V| / |U|, x23 = U . (B - C) / |U|,
    where projecting V on a rounded ex, or differencing two projections, cancels up to four digits on the family T4."""
    X = np.asarray(xyz, dtype=dtype)
    U, V = X[1] - X[0], X[2] - X[0]
    W = cross2(U, V) if twofold else np.cross(U, V)
    lw, lu = (np.sqrt(dot2(W, W)), np.sqrt(dot2(U, U))) if twofold else (np.sqrt(W @ W), np.sqrt(U @ U))
    if not (lw > 0 and lu > 0):
        raise ValueError("degenerate TRI3 element")
    ex, ez = U / lu, W / lw
    T = np.stack([ex, np.cross(ez, ex), ez])
    if twofold:  # (y12 = -ey . U is zero in exact arithmetic: its residue stays where the oracle has one, and goes nowhere else)
        dphi = np.array([[-lu, -(T[1] @ U)], [dot2(U, V) / lu, lw / lu], [dot2(U, X[1] - X[2]) / lu, -lw / lu]], dtype=dtype)
    else:
        tU, tV = T @ U, T @ V
        dphi = np.array([[-tU[0], -tU[1]], [tV[0], tV[1]], [tU[0] - tV[0], tU[1] - tV[1]]], dtype=dtype)
    return T, dphi, lw / 2


def tri3_side_ratios(xyz, dtype=np.float64):
    """Specht's mu (SA:702-704) from the sides in space: C_a - C_b = (s_a - s_b) . (s_a + s_b) by dot2 instead of the difference
    of two squared lengths, which on a needle (two sides of length 1, one of 1e-4) cancels eight digits before it is divided by
    the third"""
    X = np.asarray(xyz, dtype=dtype)
    s = [X[0] - X[1], X[2] - X[0], X[1] - X[2]]  # rows (12), (31), (23) of dphi
    C = [dot2(v, v) for v in s]
    return [dot2(s[a] - s[b], s[a] + s[b]) / C[c] for a, b, c in ((0, 1, 2), (2, 0, 1), (1, 2, 0))]


def _p_mul(x, y):
    r = np.zeros_like(x)
    for i in range(5):
        for j in range(5 - i):
            if x[i, j] != 0:
                for k in range(5 - i - j):
                    for m in range(5 - i - j - k):
                        r[i + k, j + m] += x[i, j] * y[k, m]
    return r


def _ipow(x, k):
    """x^k for a small integer k >= 0 by repeated multiplication (the same bits wherever the type's multiplication is IEEE)"""
    r = x.dtype.type(1)
    for _ in range(k):
        r = r * x
    return r


def _p_curv(p, L1, L2):
    """(d2/dL1^2, d2/dL2^2, 2 d2/dL1 dL2) of the polynomial sum p[i, j] L1^i L2^j at (L1, L2)"""
    d11 = d22 = d12 = p.dtype.type(0)
    for i in range(5):
        for j in range(5 - i):
            c = p[i, j]
            if c == 0:
                continue
            if i >= 2:
                d11 += c * (i * (i - 1)) * _ipow(L1, i - 2) * _ipow(L2, j)
            if j >= 2:
                d22 += c * (j * (j - 1)) * _ipow(L1, i) * _ipow(L2, j - 2)
            if i >= 1 and j >= 1:
                d12 += c * (i * j) * _ipow(L1, i - 1) * _ipow(L2, j - 1)
    return np.array([d11, d22, 2 * d12], dtype=p.dtype)


def specht_B(C, L1, L2, dphi, dtype=np.float64, mu=None):
    """Specht's B~ (3,9) at the area coordinates (L1, L2), columns (w, tx, ty) per node: fso_tri3_specht_B of the oracle restated
    in `dtype` -- the functions chi_1..chi_9 as polynomials in (L1, L2) for the side ratios mu, the shape functions as their
    linear combinations, the rows their second derivatives.  C (3,): squared side lengths, dphi (3,2) as tri3_frame gives it;
    mu: the side ratios, where the caller has them more accurately than C gives them (tri3_side_ratios)."""
    C, dphi, L1, L2 = np.asarray(C, dtype=dtype), np.asarray(dphi, dtype=dtype), dtype(L1), dtype(L2)
    if mu is None:
        mu = [(C[0] - C[1]) / C[2], (C[2] - C[0]) / C[1], (C[1] - C[2]) / C[0]]

    def lin(c0, c1, c2):
        p = np.zeros((5, 5), dtype=dtype)
        p[0, 0], p[1, 0], p[0, 1] = c0, c1, c2
        return p

    L = [lin(0, 1, 0), lin(0, 0, 1), lin(1, -1, -1)]
    chi = list(L) + [_p_mul(L[0], L[1]), _p_mul(L[1], L[2]), _p_mul(L[2], L[0])]
    L123 = _p_mul(chi[3], L[2])
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        m = mu[k]  # chi7 uses mu3, chi8 mu1, chi9 mu2
        lead = _p_mul(L[j], _p_mul(L[i], L[i]))
        a = (3 * (1 - m)) * L[i] + (-(1 + 3 * m)) * L[j]
        chi.append(lead + dtype(0.5) * _p_mul(L123, a + (1 + 3 * m) * L[k]))
    cc = [_p_curv(p, L1, L2) for p in chi]
    row_ki, row_ji = (1, 0, 2), (0, 2, 1)
    B = np.zeros((3, 9), dtype=dtype)
    for i in range(3):
        k = (i + 2) % 3
        xki, yki = dphi[row_ki[i]]
        xji, yji = -dphi[row_ji[i]]
        d = cc[6 + k] - cc[3 + k]
        e = cc[6 + i] - cc[6 + k]
        B[:, 3 * i + 0] = cc[i] - cc[3 + i] + cc[3 + k] + 2 * e
        B[:, 3 * i + 1] = -yki * d + yji * cc[6 + i]
        B[:, 3 * i + 2] = xki * d - xji * cc[6 + i]
    return B


def tri3_operators(xyz, flags=oracle.REF_DEFAULT, dtype=np.float64, quad_parts=False, restated=False):
    """Frame and strain operators of one triangle.  Returns dict: trafo (3,3); Bm [(3,6)] and wm [area] (one point);
    Bp [three (3,9)] and wp [area / 3 each]: the Gauss-point operators and weights of the stiffness, node-major columns
    (u, v) and (w, tx, ty).  quad_parts: frame, side vectors and area from the quad-precision build of the oracle.
    restated: nothing from the oracle -- frame, side vectors, area (tri3_frame), B~ (specht_B) and the Gauss points computed
    here in `dtype` from the double coordinates, no intermediate rounded to double.  restated="twofold": the same, with the
    frame and the side ratios from products that carry their rounding errors (tri3_frame twofold, tri3_side_ratios): with
    dtype=np.longdouble the extended-precision truth of tests/helpers/derived_truth.py, within an ulp of double of binary128
    on slivers too."""
    if restated:
        twofold = restated == "twofold"
        T, dphi, area = tri3_frame(xyz, dtype, twofold)
        C = (dphi * dphi).sum(axis=1)
        mu = tri3_side_ratios(xyz, dtype) if twofold else None
        sixth, two_thirds = dtype(1) / dtype(6), dtype(2) / dtype(3)
        gauss = ((sixth, sixth), (two_thirds, sixth), (sixth, two_thirds))
        B_of = lambda L1, L2: specht_B(C, L1, L2, dphi, dtype, mu)  # noqa: E731
    else:
        probe = oracle.material(0.3, 1.0, 1.0, flags)
        if quad_parts:
            from tests.helpers import oracle_quad
            p = oracle_quad.element_tri3(xyz, probe)[1]
        else:
            p = oracle.element_tri3(xyz, probe, want_parts=True)[1]
        dphi = p["dphi"].astype(dtype)
        area = dtype(p["area"])
        T = p["trafo"].astype(dtype)
        C = (p["dphi"] ** 2).sum(axis=1)
        gauss = GAUSS_TRI
        B_of = lambda L1, L2: oracle.specht_B(C, L1, L2, p["dphi"]).astype(dtype)  # noqa: E731
    (x12, y12), (x31, y31), (x23, y23) = dphi
    s = 1 / (2 * area)
    Bm = np.zeros((3, 6), dtype=dtype)
    Bm[0, 0::2] = [y23 * s, y31 * s, y12 * s]
    Bm[1, 1::2] = [-x23 * s, -x31 * s, -x12 * s]
    Bm[2, 0::2] = Bm[1, 1::2]
    Bm[2, 1::2] = Bm[0, 0::2]
    Y = specht_Y(dphi, area, flags)
    Bp = [Y @ B_of(L1, L2) for L1, L2 in gauss]
    return {"trafo": T, "Bm": [Bm], "wm": [area], "Bp": Bp, "wp": [area / 3] * 3}


# ------------------------------------------------------------------ QUAD4

def quad4_frame(xyz, dtype=np.float64, relative=False):
    """SA:342-375: frame from the mid-side points; local coordinates trafo @ X without translation.  Returns (trafo, loc (3,4)).
    relative: X - X_first in place of X (formed in `dtype`; in long double the difference of two doubles of similar size is
    exact).  Frame and operators use coordinate differences alone, so in exact arithmetic nothing changes; in floating point
    the projections of coordinates at a distance D from the origin no longer cancel D / size digits when they are differenced."""
    X = np.asarray(xyz, dtype=dtype)
    if relative:
        X = X - X[0]
    mid = np.array([X[s] + 0.5 * (X[(s + 1) % 4] - X[s]) for s in range(4)])
    ex = mid[1] - mid[3]
    vr = mid[2] - mid[0]
    ex = ex / np.sqrt(ex @ ex)
    ez = np.cross(ex, vr)
    ez = ez / np.sqrt(ez @ ez)
    ey = np.cross(ez, ex)
    T = np.stack([ex, ey, ez])
    return T, T @ X.T


def _dkq_B(H, xi, eta, Jinv, dtype):
    """SA:901-990 as quad4_dkq_B of the oracle states it: (3,12), columns (w, tx, ty) per node"""
    xn, en = (-1.0, 1.0, 1.0, -1.0), (-1.0, -1.0, 1.0, 1.0)
    Nx, Ne = np.zeros(8, dtype=dtype), np.zeros(8, dtype=dtype)
    for n in range(4):
        Nx[n] = 0.25 * xn[n] * (1 + eta * en[n]) * (2 * xi * xn[n] + eta * en[n])
        Ne[n] = 0.25 * en[n] * (1 + xi * xn[n]) * (2 * eta * en[n] + xi * xn[n])
    Nx[4:] = [-xi * (1 - eta), 0.5 * (1 - eta * eta), -xi * (1 + eta), -0.5 * (1 - eta * eta)]
    Ne[4:] = [-0.5 * (1 - xi * xi), -eta * (1 + xi), 0.5 * (1 - xi * xi), -eta * (1 - xi)]
    Hx, Hy = np.zeros((2, 12), dtype=dtype), np.zeros((2, 12), dtype=dtype)
    for n in range(4):
        sa, sb = n, (n + 3) % 4
        for d, N in enumerate((Nx, Ne)):
            Na, Nb, Nn = N[4 + sa], N[4 + sb], N[n]
            Hx[d, 3 * n + 0] = 1.5 * (H[0][sa] * Na - H[0][sb] * Nb)
            Hx[d, 3 * n + 1] = H[1][sa] * Na + H[1][sb] * Nb
            Hx[d, 3 * n + 2] = Nn - H[2][sa] * Na - H[2][sb] * Nb
            Hy[d, 3 * n + 0] = 1.5 * (H[3][sa] * Na - H[3][sb] * Nb)
            Hy[d, 3 * n + 1] = -Nn + H[4][sa] * Na + H[4][sb] * Nb
            Hy[d, 3 * n + 2] = -Hx[d, 3 * n + 1]
    return np.stack([Jinv[0] * Hx[0] + Jinv[1] * Hx[1],
                     Jinv[2] * Hy[0] + Jinv[3] * Hy[1],
                     Jinv[0] * Hy[0] + Jinv[1] * Hy[1] + Jinv[2] * Hx[0] + Jinv[3] * Hx[1]])


def quad4_operators(xyz, dtype=np.float64, relative=False):
    """Frame and strain operators of one quadrilateral at the 2 x 2 Gauss points (the order of the oracle's loops).  Returns dict:
    trafo; Bm [four (3,8)], Bp [four (3,12)], wm = wp = [det J at the point].  Bp is MINUS the DKQ operator of the stiffness: the
    curvature (w,xx, w,yy, 2 w,xy), see the module's head.  relative: as quad4_frame has it."""
    T, loc = quad4_frame(xyz, dtype, relative)
    x, y = loc[0], loc[1]
    dphi = np.array([[x[s] - x[(s + 1) % 4], y[s] - y[(s + 1) % 4]] for s in range(4)])
    H = [[None] * 4 for _ in range(5)]
    for s in range(4):
        dx, dy = dphi[s]
        l2 = dx * dx + dy * dy
        H[0][s], H[1][s], H[2][s] = -dx / l2, 0.75 * dx * dy / l2, (0.25 * dx * dx - 0.5 * dy * dy) / l2
        H[3][s], H[4][s] = -dy / l2, (0.25 * dy * dy - 0.5 * dx * dx) / l2
    rn, sn = (-1.0, 1.0, 1.0, -1.0), (-1.0, -1.0, 1.0, 1.0)
    root = np.sqrt(dtype(1) / dtype(3))
    Bm, Bp, w = [], [], []
    for ii in range(2):
        for jj in range(2):
            r, s = (-root if ii else root), (-root if jj else root)
            dr = np.array([0.25 * rn[n] * (1 + sn[n] * s) for n in range(4)], dtype=dtype)
            ds = np.array([0.25 * sn[n] * (1 + rn[n] * r) for n in range(4)], dtype=dtype)
            J = np.array([dr @ x, dr @ y, ds @ x, ds @ y])
            det = J[0] * J[3] - J[1] * J[2]
            Jinv = np.array([J[3], -J[1], -J[2], J[0]]) / det
            dNx, dNy = Jinv[0] * dr + Jinv[1] * ds, Jinv[2] * dr + Jinv[3] * ds
            B = np.zeros((3, 8), dtype=dtype)
            B[0, 0::2], B[1, 1::2], B[2, 0::2], B[2, 1::2] = dNx, dNy, dNy, dNx
            Bm.append(B)
            Bp.append(-_dkq_B(H, r, s, Jinv, dtype))
            w.append(det)
    return {"trafo": T, "Bm": Bm, "wm": w, "Bp": Bp, "wp": list(w)}


# ------------------------------------------------------------------ from operators to the 14 values

def mean_operator(Bs, ws):
    tot = sum(ws)
    return sum(w * B for w, B in zip(ws, Bs)) / tot


def to_global(T, a3):
    """R^T [[a_xx, a_xy, 0], [a_xy, a_yy, 0], [0, 0, 0]] R as its six components xx yy zz xy yz zx"""
    A = np.zeros((3, 3), dtype=a3.dtype)
    A[0, 0], A[1, 1], A[0, 1], A[1, 0] = a3[0], a3[1], a3[2], a3[2]
    G = T.T @ A @ T
    return np.array([G[p, q] for p, q in VOIGT])


def von_mises(s):
    return np.sqrt(s[0] * s[0] + s[1] * s[1] - s[0] * s[1] + 3 * s[2] * s[2])


def element_resultants(xyz, u, nu, E, t, flags=oracle.REF_DEFAULT, dtype=np.float64, quad_parts=False, with_local=False, uniform_abs=None,
                       restated=False):
    """xyz (nn, 3), u (nn, 6), nn = 3 or 4.  Returns (out[14], scale[14]) in float64 (and the local N, M with with_local).
    uniform_abs: the scale is formed with |d_j| = uniform_abs for every local nodal value instead: what an error of that size in
    every entry of u can do to the element's values.  restated: as tri3_operators has it; a quadrilateral's operators, restated
    in `dtype` in any case, are then formed with relative=True."""
    xyz = np.asarray(xyz, dtype=np.float64)
    nn = len(xyz)
    ops = tri3_operators(xyz, flags, dtype, quad_parts, restated) if nn == 3 else quad4_operators(xyz, dtype, relative=bool(restated))
    T = ops["trafo"]
    u = np.asarray(u, dtype=dtype).reshape(nn, 6)
    ul, rl = u[:, :3] @ T.T, u[:, 3:] @ T.T
    dm = ul[:, :2].reshape(-1)
    dp = np.stack([ul[:, 2], rl[:, 0], rl[:, 1]], axis=1).reshape(-1)
    tDm, Dp = plane_material(nu, E, t, dtype)
    DBm = tDm @ mean_operator(ops["Bm"], ops["wm"])
    DBp = -(Dp @ mean_operator(ops["Bp"], ops["wp"]))
    N, M = DBm @ dm, DBp @ dp
    if uniform_abs is None:
        SN, SM = np.abs(DBm) @ np.abs(dm), np.abs(DBp) @ np.abs(dp)
    else:
        SN, SM = np.abs(DBm).sum(axis=1) * dtype(uniform_abs), np.abs(DBp).sum(axis=1) * dtype(uniform_abs)
    t = dtype(t)
    top, bot = N / t + 6 * M / (t * t), N / t - 6 * M / (t * t)
    out = np.concatenate([to_global(T, N), to_global(T, M), [von_mises(top), von_mises(bot)]])
    s_vm = 4 * (SN / t + 6 * SM / (t * t)).max()
    scale = np.concatenate([to_global(np.abs(T), SN), to_global(np.abs(T), SM), [s_vm, s_vm]])
    if with_local:
        return out.astype(np.float64), scale.astype(np.float64), N.astype(np.float64), M.astype(np.float64)
    return out.astype(np.float64), scale.astype(np.float64)


def mesh_resultants(xyz, tri, quad, u, nu, E, t, sec=None, flags=oracle.REF_DEFAULT, dtype=np.float64, quad_parts=False, uniform_abs=None,
                    restated=False):
    """(out, scale), each (n_tri + n_quad, 14): triangles in their order, then quadrilaterals.  sec = (sections (n, 3) of
    (nu, E, t), tri_section, quad_section) gives every element its own material."""
    xyz = np.asarray(xyz, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64).reshape(len(xyz), 6)
    out, scale = [], []
    for conn, which in ((tri, 1), (quad, 2)):
        if conn is None:
            continue
        for e, c in enumerate(np.asarray(conn).reshape(-1, 3 if which == 1 else 4)):
            m = (nu, E, t) if sec is None else tuple(np.asarray(sec[0], dtype=np.float64).reshape(-1, 3)[sec[which][e]])
            o, s = element_resultants(xyz[c], u[c], *m, flags=flags, dtype=dtype, quad_parts=quad_parts, uniform_abs=uniform_abs,
                                      restated=restated)
            out.append(o)
            scale.append(s)
    return np.array(out).reshape(-1, 14), np.array(scale).reshape(-1, 14)


def bound_ratio(out, ref, scale):
    """max |out - ref| / (1e-12 scale); entries whose scale is zero must agree exactly (they count as 0 or inf)"""
    diff = np.abs(np.asarray(out) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, diff / (TINY * scale), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------ the meshes the device is compared on (tests/test_gpu_resultants.py)

NU, E, T = 0.3, 2.1e5, 0.37
WORKGROUP = 256  # elements per workgroup of k_element_resultants (one lane each)


def trimmed_panel(n_tri):
    """the first n_tri triangles of a lifted 13 x 10 panel (260 triangles), the nodes they leave unattached removed"""
    from tests.helpers import prescribed as pr
    xyz, tri = pr.panel(nx=13, ny=10, lift=True)
    tri = tri[:n_tri]
    used = np.unique(tri)
    new = -np.ones(len(xyz), np.int64)
    new[used] = np.arange(len(used))
    return xyz[used], new[tri].astype(np.int32)


def device_meshes():
    """name -> function returning (xyz, tri, quad, sec, env): the meshes of tests/test_gpu_prescribed.py and the smallest shapes
    of the lane-per-element mapping.  sec: None or (sections, tri_section, quad_section); env: variables the context is made under.
    The grid of k_element_resultants is not capped (one workgroup per 256 elements, no stride loop): no mesh past a cap."""
    from tests.helpers import meshes, prescribed as pr, sections
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], dtype=np.float64), np.array([[0, 1, 2]], np.int32))
    two = (np.array([[0, 0, 0], [1, 0, 0.1], [1, 1, 0], [0, 1, 0.2]], dtype=np.float64), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    quad = (np.array([[0, 0, 0.1], [1.2, 0.1, 0], [1.4, 1.0, 0.2], [-0.1, 0.8, 0]], dtype=np.float64), np.array([[0, 1, 2, 3]], np.int32))
    lifted = pr.panel(lift=True)

    def three():
        xyz, tri = lifted
        return xyz, tri, None, (sections.THREE, sections.strips_of(xyz, tri), None), {}

    cases = {
        "one_triangle": lambda: one + (None, None, {}),
        "two_triangles": lambda: two + (None, None, {}),
        "one_quadrilateral": lambda: (quad[0], None, quad[1], None, {}),
        "strip33": lambda: pr.strip33() + (None, None, {}),
        "lifted_panel": lambda: lifted + (None, None, {}),
        "mixed_petals24": lambda: meshes.mixed_petals(24) + (None, {}),
        "coil300": lambda: meshes.coil(300) + (None, None, {}),
        "delaunay600_rcm": lambda: meshes.delaunay_patch(600, 2, strips=False) + (None, None, {"FEMSHELL_REORDER": "rcm"}),
        "panel_three_sections": three,
        "lifted_panel_full_storage": lambda: lifted + (None, None, {"FEMSHELL_SYMMETRIC": "0"}),
    }
    for n in (1, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1):
        cases["trimmed_panel_%d" % n] = (lambda n=n: trimmed_panel(n) + (None, None, {}))
    return cases


def random_u(n_nodes, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n_nodes, 6))
