"""tests/golden/derived_truth.npz is what the long-double evaluation of the numpy reference computes here, that evaluation is
pinned against the binary128 stiffness parts of the oracle, the errors of the FP64 reference stored in the fixture are the FP64
reference's, and the check of tests/test_gpu_derived_truth.py sees defects that the older 1e-12 bounds accept (no GPU).

The pins of the long-double path (restated="twofold" of tests/helpers/resultants.py) against oracle/libfemshell_oracle_quad.so,
measured when this file was written, worst over all families:
    triangle geometry (trafo, dphi, area), entries in ulps of double     0 on T1 .. T7
    sum_g w B^T D B against Ke_m, Ke_p, normwise, in units of 2^-52      Ke_m 0.00; Ke_p 0.06 (T3) on triangles, 0.14 (Q3) on
                                                                         quadrilaterals
A plain long-double evaluation (restated=True) misses both pins on the slivers and needles of T4, at 3 ulps and 1195 x 2^-52
(2.65e-13 in Ke_p): projecting a side on a rounded ex, the cross product of nearly parallel sides and the difference of two
squared side lengths cancel four to eight digits there, and at 2^-64 per operation fewer than 53 bits are left.  The twofold
path forms those products with their rounding errors carried along (rs.dot2) and is what the fixture is made with; the quadrilaterals
need none of it once their coordinates are taken relative to the first node (Q3 without that: 371 x 2^-52).
"""
import numpy as np
import pytest

from tests.helpers import buckling as bk, derived_truth as dt, element_loads as el, oracle, oracle_quad, resultants as rs, truth

FX = dict(truth.load())
DX = dict(dt.load())
LD = dt.LD
EPS = truth.EPS
needs_long_double = pytest.mark.skipif(not dt.long_double_is_extended(),
                                       reason="numpy's long double has fewer than 64 bits of mantissa on this platform")
# the families on which the FP64 reference is within 2.5e-14 of the truth in every metric (asserted below): a defect of 1e-13
# is more than four times that
WELL = [f for f in truth.FAMILIES if f != "T4"]


def _material(fam, e):
    nu, E, t, flags = truth.material_of(FX, fam, e)
    return (nu, E, t), flags


# ------------------------------------------------------------------ 1. the long-double path against binary128

@needs_long_double
@pytest.mark.parametrize("fam", truth.TRI_FAMILIES)
def test_long_double_triangle_geometry_is_the_quad_builds(fam):
    """trafo, dphi and area of rs.tri3_frame in long double, rounded to double, equal the parts of oracle_quad.element_tri3
    (binary128 rounded once) to 1 ulp of double per entry.  One entry is not compared in ulps: y12 = -ey . (B - A) is zero in exact
    arithmetic (ex lies along B - A), both evaluations return their own rounding residue there (1e-35 and 1e-20 of the side), and
    it is held to 2^-60 of the side's length instead.  Measured: 0 ulps on every family."""
    worst = 0.0
    for e in range(truth.PER_FAMILY):
        mat, flags = _material(fam, e)
        xyz = FX[fam + "_xyz"][e]
        p = oracle_quad.element_tri3(xyz, oracle.material(*mat, flags))[1]
        T, dphi, area = rs.tri3_frame(xyz, LD, twofold=True)
        side = np.linalg.norm(xyz[1] - xyz[0])
        assert abs(float(dphi[0, 1])) <= 2.0 ** -60 * side and abs(p["dphi"][0, 1]) <= 2.0 ** -60 * side
        keep = np.ones((3, 2), dtype=bool)
        keep[0, 1] = False
        for got, want in ((T.astype(np.float64), p["trafo"]), (dphi.astype(np.float64)[keep], p["dphi"][keep]),
                          (np.float64(area), np.float64(p["area"]))):
            ulps = np.abs(np.asarray(got) - want) / np.spacing(np.abs(want))
            worst = max(worst, float(np.max(ulps)))
    print("%s long-double triangle geometry against binary128: %.0f ulp" % (fam, worst))
    assert worst <= 1.0


@needs_long_double
@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_long_double_operators_give_the_quad_builds_stiffness_parts(fam):
    """test_gauss_point_operators_give_the_oracles_stiffness_parts (tests/test_resultants_cpu.py) in long double, for every
    element of the fixture with its own material and flags: sum_g w_g B_g^T D B_g, rounded to double, is within 4 x 2^-52,
    normwise, of Ke_m and of Ke_p of the quad build (the truth is rounded once; the rest is slack for the norm).  Measured: at
    most 0.06 x 2^-52 on the triangle families (T3, Ke_p) and 0.14 x 2^-52 on the quadrilaterals (Q3, Ke_p)."""
    worst_m = worst_p = 0.0
    for e in range(truth.PER_FAMILY):
        (nu, E, t), flags = _material(fam, e)
        xyz = FX[fam + "_xyz"][e]
        if fam[0] == "T":
            p = oracle_quad.element_tri3(xyz, oracle.material(nu, E, t, flags))[1]
            ops = rs.tri3_operators(xyz, flags, LD, restated="twofold")
        else:
            p = oracle_quad.element_quad4(xyz, oracle.material(nu, E, t, flags))[1]
            ops = rs.quad4_operators(xyz, LD, relative=True)
            assert np.abs(ops["trafo"].astype(np.float64) - p["trafo"]).max() <= 2 * EPS
        tDm, Dp = rs.plane_material(nu, E, t, LD)
        Km = sum(w * (B.T @ tDm @ B) for w, B in zip(ops["wm"], ops["Bm"])).astype(np.float64)
        Kp = sum(w * (B.T @ Dp @ B) for w, B in zip(ops["wp"], ops["Bp"])).astype(np.float64)
        worst_m = max(worst_m, np.linalg.norm(Km - p["Ke_m"]) / np.linalg.norm(p["Ke_m"]))
        worst_p = max(worst_p, np.linalg.norm(Kp - p["Ke_p"]) / np.linalg.norm(p["Ke_p"]))
    print("%s long-double operators against binary128: Ke_m %.2e, Ke_p %.2e (%.2f, %.2f x 2^-52)" % (fam, worst_m, worst_p, worst_m / EPS, worst_p / EPS))
    assert worst_m <= 4 * EPS and worst_p <= 4 * EPS


@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_restated_fp64_reference_agrees_with_the_one_built_on_the_oracle(fam):
    """restated=True with dtype=np.float64 (the "FP64 reference" of the fixture) and the evaluation the older tests use (frame,
    sides, area and B~ from the FP64 oracle; absolute coordinates in a quadrilateral) are two FP64 evaluations of one quantity: they
    agree within the sum of their distances from the truth, which for the older one is 2e-10 on Q3 and T4 and 3e-14 elsewhere"""
    tol = 1e-9 if fam in ("T4", "Q3") else 1e-13
    for s in range(len(dt.STATES)):
        for e in range(truth.PER_FAMILY):
            mat, flags = _material(fam, e)
            xyz, u = FX[fam + "_xyz"][e], DX[fam + "_u"][s][e]
            a, _ = rs.element_resultants(xyz, u, *mat, flags=flags)
            b, _ = rs.element_resultants(xyz, u, *mat, flags=flags, restated=True)
            for k in (slice(0, 6), slice(6, 12), slice(12, 14)):
                assert np.linalg.norm(a[k] - b[k]) <= tol * np.linalg.norm(a[k]), (fam, s, e, k)


# ------------------------------------------------------------------ 2. the fixture

@needs_long_double
@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_fixture_is_what_the_long_double_reference_computes(fam):
    nn = truth.nodes_of(fam)
    assert DX[fam + "_u"].shape == (2, truth.PER_FAMILY, nn, 6) and DX[fam + "_load"].shape == (truth.PER_FAMILY, 4)
    for e in range(truth.PER_FAMILY):
        for s in range(len(dt.STATES)):
            tr = dt.reference(FX, DX, fam, e, s, LD)
            np.testing.assert_array_equal(tr["res"], DX[fam + "_res"][s][e])
            np.testing.assert_array_equal(truth.upper(tr["g"]), DX[fam + "_g"][s][e])
            # the truth's g is symmetric to long double's own rounding: the stored upper triangle is all of it
            assert np.abs(tr["g"] - tr["g"].T).max() <= 2.0 ** -60 * np.abs(tr["g"]).max()
            if fam in dt.FLAT:
                ref = dt.reference(FX, DX, fam, e, s)
                np.testing.assert_array_equal((tr["res"][:12] == 0.0) & (ref["res"][:12] == 0.0), DX[fam + "_zero"][s][e])
        np.testing.assert_array_equal(tr["share"], DX[fam + "_share"][e])
        np.testing.assert_array_equal(tr["mass"], DX[fam + "_mass"][e])


@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_inputs_of_the_fixture_are_what_it_says_they_are(fam):
    u = DX[fam + "_u"]
    assert np.abs(u[0]).max() <= 1.0 and np.abs(u[0]).max() > 0.9 and u[0, :, :, 3:].any()
    # smooth: zero translation at the first node, strains and rotations of 1e-4
    assert not u[1, :, 0, :3].any() and 1e-5 < np.abs(u[1, :, :, 3:]).max() < 1e-3
    for e in range(truth.PER_FAMILY):
        X = FX[fam + "_xyz"][e]
        size = np.linalg.norm(X[1:] - X[0], axis=1).max()
        assert np.abs(u[1, e, :, :3]).max() <= 1e-3 * size
    for e in range(truth.PER_FAMILY):  # one density per distinct material, no two materials share one
        for f2 in truth.FAMILIES:
            for e2 in range(truth.PER_FAMILY):
                same = truth.material_of(FX, fam, e)[:3] == truth.material_of(FX, f2, e2)[:3]
                assert (DX[fam + "_rho"][e] == DX[f2 + "_rho"][e2]) == same
    np.testing.assert_array_equal(DX[fam + "_load"], el.random_loads(truth.PER_FAMILY, 0, seed=100 + truth.FAMILIES.index(fam))[0])
    if fam in truth.FRAME:
        for s in range(2):
            for e in range(truth.PER_FAMILY):
                Q = FX[fam + "_Q"][e]
                want = np.concatenate([u[s, e, :, :3] @ Q.T, u[s, e, :, 3:] @ Q.T], axis=1)
                np.testing.assert_allclose(DX[fam + "_u_moved"][s][e], want, rtol=0, atol=4 * EPS * np.abs(u[s, e]).max())
    if fam in dt.FLAT:  # N and M of a flat element in a coordinate plane: the three components across the plane are exact zeros
        assert (DX[fam + "_zero"].sum(axis=2) == 6).all()


def _reference_results(fam, planted=None):
    results = [[dt.reference(FX, DX, fam, e, s) for s in range(len(dt.STATES))] for e in range(truth.PER_FAMILY)]
    moved = None
    if fam in truth.FRAME:
        moved = [[dt.reference(FX, DX, fam, e, s, moved=True) for s in range(len(dt.STATES))] for e in range(truth.PER_FAMILY)]
    if planted is not None:
        for e in range(truth.PER_FAMILY):
            for s in range(len(dt.STATES)):
                planted(fam, e, s, results[e][s])
                if moved is not None:
                    planted(fam, e, s, moved[e][s])
    return results, moved


@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_stored_reference_errors_are_the_fp64_references_and_it_passes_its_own_check(fam):
    results, moved = _reference_results(fam)
    worst = dt.family_worst(FX, DX, fam, results, moved)
    for m in dt.metrics_of(fam):
        # (the differences are exact doubles; only the order of the sums inside the norms may differ between numpy builds)
        np.testing.assert_allclose(worst[m], DX["%s_err_%s" % (fam, m)].max(axis=-1), rtol=1e-9, atol=1e-30, err_msg=m)
    for m in dt.CONDITIONED:
        assert DX["%s_err_%s" % (fam, m)].max() <= dt.CONDITION
    assert dt.check(DX, fam, worst) == []
    if fam in dt.FLAT:
        assert not np.any(worst["spurious"])
    if fam in WELL:
        assert max(DX["%s_err_%s" % (fam, m)].max() for m in dt.metrics_of(fam)) <= 2.5e-14


def test_every_copy_and_every_member_is_held_to_the_bound():
    """family_worst over lists of copies (what the device hands in) takes the worst copy, and a subset of a family (a mixed mesh)
    is held to the bound of the whole family"""
    fam = "T1"
    results, moved = _reference_results(fam)
    bad = [dict(r) for r in results[3]]
    bad[1]["res"] = bad[1]["res"] * (1.0 + 1e-12)
    copies = [[r, r] for r in results]
    copies[3] = [results[3], bad]
    worst = dt.family_worst(FX, DX, fam, copies, [[m, m] for m in moved])
    over = {(b[0], b[1]) for b in dt.check(DX, fam, worst)}
    assert {("N", "smooth"), ("M", "smooth"), ("vm", "smooth")} <= over and not any(s == "random" for _, s in over if _ != "frame")
    part = dt.family_worst(FX, DX, fam, [results[3]], elements=[3])
    assert "frame" not in part and dt.check(DX, fam, part, metrics=dt.MIXED_METRICS) == []


def test_where_the_factor_of_q5_g_comes_from():
    """FACTORS of tests/test_gpu_derived_truth.py, Q5, g: in the smooth state element 0 of Q5 has |g| at 1/82 of its absolute sum,
    and FP64 evaluations of the same formulas that differ only by an exact shift of the coordinates (absolute; relative to node 2;
    relative to node 0) are 1.7e-14, 7.9e-15 and 4.3e-16 from the truth: the reference's own error on this element is a draw from
    that spread, and the family's stored worst (1.09e-15, element 4) is no bound for it."""
    fam, e, s = "Q5", 0, 1
    (nu, E, t), flags = _material(fam, e)
    xyz, u = FX[fam + "_xyz"][e], DX[fam + "_u"][s][e]
    conn = np.arange(4, dtype=np.int32)[None]
    tr = dt.truth_of(DX, fam, e, s)["g"]
    errs = []
    for X in (xyz, xyz - xyz[2], xyz - xyz[0]):
        _, g, ga = bk.element_coefficients(X, None, conn, u, nu, E, t, flags=flags)[0]
        errs.append(np.linalg.norm(g - tr) / np.linalg.norm(tr))
    print("Q5 element 0, smooth: |ga| / |g| = %.1f, g of three FP64 evaluations against the truth: %s" % (
        np.linalg.norm(ga) / np.linalg.norm(g), ", ".join("%.1e" % v for v in errs)))
    assert np.linalg.norm(ga) / np.linalg.norm(g) > 50.0
    stored = dt.reference_worst(DX, fam, "g", s)
    assert max(errs) > 8.0 * stored and min(errs) < stored and 82.0 * EPS > 8.0 * stored


# ------------------------------------------------------------------ 3. defects the older bounds accept and this check reports

def _scaled_M(fam, e, s, r):
    r["res"] = r["res"].copy()
    r["res"][6:12] *= 1.0 + 1e-13


def _scaled_g(fam, e, s, r):
    r["g"] = r["g"] * (1.0 + 1e-13)


def _context_t(fam, e, s, r):
    """the von Mises values with the thickness of the context (truth.OWN_CONTEXT) where the section's belongs"""
    mat, flags = _material(fam, e)
    _, _, N, M = rs.element_resultants(FX[fam + "_xyz"][e], DX[fam + "_u"][s][e], *mat, flags=flags, restated=True, with_local=True)
    t = truth.OWN_CONTEXT[2]
    r["res"] = r["res"].copy()
    r["res"][12], r["res"][13] = rs.von_mises(N / t + 6 * M / (t * t)), rs.von_mises(N / t - 6 * M / (t * t))


def _single_sqrt(fam, e, s, r):
    """g of a triangle with 1 / (2 |cr|^3) from a single-precision square root of |cr|^2"""
    X = FX[fam + "_xyz"][e]
    cr = np.cross(X[1] - X[0], X[2] - X[0])
    c2 = cr @ cr
    r["g"] = r["g"] * (np.sqrt(c2) / float(np.sqrt(np.float32(c2))))


def _over(fam, planted):
    results, moved = _reference_results(fam, planted)
    return {b[0] for b in dt.check(DX, fam, dt.family_worst(FX, DX, fam, results, moved))}


@pytest.mark.parametrize("fam", WELL)
def test_a_moment_wrong_at_1e_13_is_reported_and_the_older_bound_accepts_it(fam):
    """M scaled by (1 + 1e-13), g likewise: over the budget here on every well-conditioned family; rs.bound_ratio and
    bk.bound_ratio at 1e-12 of the absolute-sum scales (tests/test_gpu_resultants.py, tests/test_gpu_geometric_product.py) accept
    both when they are planted in those tests' own reference.  That difference is the gap this check closes."""
    assert _over(fam, _scaled_M) == {"M"}
    assert _over(fam, _scaled_g) == {"g"}
    nn = truth.nodes_of(fam)
    conn = np.arange(nn, dtype=np.int32)[None]
    tri, quad = (conn, None) if nn == 3 else (None, conn)
    X = np.stack([truth.probe_vector(nn, [conn[0]], b, d) for b in range(nn) for d in range(3)])
    for s in range(len(dt.STATES)):
        for e in range(truth.PER_FAMILY):
            mat, flags = _material(fam, e)
            xyz, u = FX[fam + "_xyz"][e], DX[fam + "_u"][s][e]
            ref, S = rs.element_resultants(xyz, u, *mat, flags=flags)
            out = ref.copy()
            out[6:12] *= 1.0 + 1e-13
            assert rs.bound_ratio(out, ref, S) <= 1.0
            co = bk.element_coefficients(xyz, tri, quad, u, *mat, flags=flags)
            Y_ref, T = bk.product(nn, co, X)
            Y, _ = bk.product(nn, [(co[0][0], co[0][1] * (1.0 + 1e-13), co[0][2])], X)
            assert bk.bound_ratio(Y, Y_ref, T) <= 1.0


@pytest.mark.parametrize("fam", [f for f in WELL if f[0] == "T"])
def test_a_single_precision_third_in_the_gauss_mean_is_reported(fam, monkeypatch):
    """the mean over the triangle's three Gauss points with 1/3 = float(np.float32(1 / 3)): M and the von Mises values are off
    by 1e-8"""
    mean = rs.mean_operator

    def single_third(Bs, ws):
        return float(np.float32(1.0 / 3.0)) * sum(Bs) if len(Bs) == 3 else mean(Bs, ws)

    monkeypatch.setattr(rs, "mean_operator", single_third)
    over = _over(fam, None)
    assert "M" in over and "vm" in over and not over & {"N", "g", "load", "mass"}


@pytest.mark.parametrize("fam", truth.OWN_FAMILIES)
def test_the_thickness_of_the_context_in_the_von_mises_values_is_reported(fam):
    assert fam in WELL and _over(fam, _context_t) == {"vm"}


@pytest.mark.parametrize("fam", [f for f in WELL if f[0] == "T"])
def test_a_single_precision_square_root_in_the_normalisation_of_g_is_reported(fam):
    assert _over(fam, _single_sqrt) == {"g"}
