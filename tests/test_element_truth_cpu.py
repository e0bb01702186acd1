"""tests/golden/element_truth.npz is what the quad-precision build of the oracle's element path computes here, the errors
of the FP64 oracle stored in it are the FP64 oracle's, and the statements the GPU test (tests/test_gpu_element_truth.py)
leans on hold: every stored element is well enough conditioned, the two builds agree on the committed goldens, and on the
flat families the FP64 oracle itself has exact zeros wherever the truth has them."""
import os

import numpy as np
import pytest

from tests.helpers import meshes, oracle, oracle_quad, prescribed as pr, truth

FX = dict(truth.load())


def _elements(fam):
    nodes = truth.nodes_of(fam)
    quad_el = oracle_quad.element_tri3 if nodes == 3 else oracle_quad.element_quad4
    fp64_el = oracle.element_tri3 if nodes == 3 else oracle.element_quad4
    mats = [oracle.material(*truth.material_of(FX, fam, e)) for e in range(truth.PER_FAMILY)]
    return quad_el, fp64_el, mats


@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_fixture_is_what_the_quad_build_computes(fam):
    quad_el, _, mats = _elements(fam)
    assert FX[fam + "_xyz"].shape == (truth.PER_FAMILY, truth.nodes_of(fam), 3)
    for e in range(truth.PER_FAMILY):
        Ke, parts = quad_el(FX[fam + "_xyz"][e], mats[e])
        np.testing.assert_array_equal(truth.upper(parts["K_global_nm"]), FX[fam + "_K"][e])
        np.testing.assert_array_equal(parts["trafo"], FX[fam + "_trafo"][e])
        # the two layouts of the quad build are one matrix, and the truth is symmetric: the stored upper triangle is all of it
        # (up to binary128's own rounding, seen where an entry cancels to 1e-34 of the matrix instead of 0)
        np.testing.assert_array_equal(truth.to_node_major(Ke, truth.nodes_of(fam)), parts["K_global_nm"])
        np.testing.assert_allclose(parts["K_global_nm"], truth.truth_of(FX, fam, e), rtol=0,
                                   atol=1e-30 * np.abs(parts["K_global_nm"]).max())
    if fam in truth.FRAME:
        moved = np.stack([FX[fam + "_xyz"][e] @ FX[fam + "_Q"][e].T + FX[fam + "_c"][e] for e in range(truth.PER_FAMILY)])
        np.testing.assert_allclose(FX[fam + "_xyz_moved"], moved, rtol=0, atol=1e-13)
        for Q in FX[fam + "_Q"]:
            assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-14 and np.linalg.det(Q) > 0


@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_stored_oracle_errors_are_the_fp64_oracles_and_the_family_is_well_conditioned(fam):
    _, fp64_el, mats = _elements(fam)
    K = [fp64_el(FX[fam + "_xyz"][e], mats[e], want_parts=True)[1]["K_global_nm"] for e in range(truth.PER_FAMILY)]
    moved = None
    if fam in truth.FRAME:
        moved = [fp64_el(FX[fam + "_xyz_moved"][e], mats[e], want_parts=True)[1]["K_global_nm"] for e in range(truth.PER_FAMILY)]
    err = truth.family_errors(FX, fam, K, moved)
    for m in truth.metrics_of(fam):
        # (the differences are exact doubles; only the order of the sums inside the norms may differ between numpy builds)
        np.testing.assert_allclose(FX["%s_err_%s" % (fam, m)], err[m], rtol=1e-9, atol=1e-30, err_msg=m)
    assert err["whole"].max() <= truth.FAMILY_CONDITION
    if fam in truth.CLASSWISE:
        # the oracle has exact zeros wherever the truth has them, and the truth has them wherever two dof classes meet
        assert err["spurious"].sum() == 0
        for e in range(truth.PER_FAMILY):
            cross = truth.class_masks(truth.nodes_of(fam), int(FX[fam + "_normal"][e]))["cross"]
            assert not truth.truth_of(FX, fam, e)[cross].any()
            assert not K[e][cross].any()


def test_families_are_what_the_fixture_says_they_are():
    """the edges the families are there for: thickness, Poisson's ratio, units, distance, flags"""
    assert sorted(set(FX["T3_mat"][:, 2])) == [1e-5, 1e-3, 1e-1] and sorted(set(FX["Q4_mat"][:, 2])) == [1e-5, 1e-3, 1e-1]
    assert sorted(set(FX["T6_mat"][:, 0])) == [0.0, 0.499, 0.4999999]
    assert sorted(set(FX["T7_mat"][:, 1])) == [1e-3, 1e11]
    for fam in ("T1", "T2", "Q1"):
        assert sorted(set(FX[fam + "_mat"][:, 3])) == [0.0, 1.0, 2.0, 3.0]
    for fam, far in (("T5", 1e8), ("Q3", 1e6)):
        d = np.linalg.norm(FX[fam + "_xyz"].mean(axis=1), axis=1)
        assert d.min() > 50.0 and 0.9 * far < d.max() < 1.1 * far
    # T2: half of the frames are made of exact zeros and +-1
    exact = [np.isin(np.abs(T), (0.0, 1.0)).all() for T in FX["T2_trafo"]]
    assert sum(exact) == 4
    # Q6 is warped: its nodes are out of their mean plane by 0.01 and 0.1 of the side
    for e, X in enumerate(FX["Q6_xyz"]):
        n = np.cross(X[2] - X[0], X[3] - X[1])
        out = abs((X[1] - X[0]) @ n / np.linalg.norm(n)) / 2
        assert out == pytest.approx(0.01 if e % 2 == 0 else 0.1, rel=0.35)
    assert os.path.getsize(truth.FIXTURE) < 512 * 1024


@pytest.mark.parametrize("name,nodes", [("tri3_elements", 3), ("quad4_elements", 4)])
def test_quad_and_fp64_builds_agree_on_the_committed_goldens(name, nodes):
    g = np.load(meshes.GOLDEN + "/%s.npz" % name)
    mat = oracle.material(float(g["nu"]), float(g["E"]), float(g["t"]))
    conn = g["tri"] if nodes == 3 else g["quad"]
    worst = 0.0
    for e, c in enumerate(conn):
        Kq = (oracle_quad.element_tri3 if nodes == 3 else oracle_quad.element_quad4)(g["xyz"][c], mat)[0]
        worst = max(worst, np.linalg.norm(g["Ke"][e] - Kq) / np.linalg.norm(Kq))
    print(name, "FP64 goldens against quad: %.2e" % worst)
    assert worst <= 1e-13, worst


def test_quad_material_matrices_round_to_the_fp64_ones():
    mat = oracle.material(0.3, 2.1e5, 0.37)
    for a, b in zip(oracle.material_matrices(mat), oracle_quad.material_matrices(mat)):
        assert np.abs(a - b).max() <= 4 * truth.EPS * np.abs(b).max()


# ------------------------------------------------------------------ the helpers of the GPU test, with the FP64 oracle as the device

def test_paths_of_the_gpu_test():
    """the product paths reach the four instantiations of k_element_product (triangles or quadrilaterals in the plan, sections
    set or not; the GPU test asserts each from its mesh), and the "own" paths run where they can tell one material from another"""
    product = [p for p in truth.PATHS + truth.OWN_PATHS if p[0] == truth.PRODUCT]
    assert {(fam[0] == "Q", bool(p[2])) for fam in truth.FAMILIES for p in product if p[2] != "own"} == \
        {(False, False), (False, True), (True, False), (True, True)}
    ids = [truth.path_id(p) for p in truth.PATHS + truth.OWN_PATHS]
    assert len(set(ids)) == len(ids) and "k_element_product" in ids and "k_element_product-sections" in ids
    assert [i for i in ids if i.endswith("-own")] == ["k_element_matrices-own", "k_assemble-sym-own", "k_assemble-full-own",
                                                     "k_assemble_pipe-sym-own", "k_assemble_pipe-full-own", "k_element_product-own"]
    for fam in truth.FAMILIES:
        by_flags = {}
        for m in truth.groups_of(FX, fam):
            by_flags.setdefault(m[3], set()).add(m[:3])
        assert (fam in truth.OWN_FAMILIES) == any(len(v) > 1 for v in by_flags.values()), fam
        for k in range(3):  # the material of an "own" context is no element's, in no component
            assert truth.OWN_CONTEXT[k] not in FX[fam + "_mat"][:, k]
    for fam in truth.OWN_FAMILIES:
        (material, els), = truth.groups_of(FX, fam, own=True).items()
        assert material == truth.OWN_CONTEXT + (3,) and els == list(range(truth.PER_FAMILY))


def _dense_product(K, conn, n_nodes):
    """x -> sum_e K_e x_e for node-major element matrices K_e on the nodes conn[e]"""
    def product(x):
        x = np.asarray(x, dtype=np.float64).reshape(n_nodes, 6)
        y = np.zeros((n_nodes, 6))
        for Ke, c in zip(K, conn):
            y[c] += (Ke @ x[c].ravel()).reshape(-1, 6)
        return y.ravel()
    return product


@pytest.mark.parametrize("kinds", ["triangles", "quadrilaterals", "mixed"])
def test_probing_reads_the_element_matrices_back_exactly(kinds):
    mat = oracle.material(*truth.material_of(FX, "T1", 0))
    Xt = list(FX["T1_xyz"]) if kinds != "quadrilaterals" else None
    Xq = list(FX["Q1_xyz"]) if kinds != "triangles" else None
    xyz, tri, quad = truth.isolated_mesh(Xt, Xq, reps=2)
    K_unc, _ = pr.matrices(xyz, tri, quad, mat, np.zeros(len(xyz), np.uint8))
    calls = []

    def product(x):
        calls.append(1)
        return oracle.spmv(*K_unc, x)

    K = truth.probe_element_matrices(product, len(xyz), list(tri) + list(quad))
    assert len(calls) == (18 if kinds == "triangles" else 24)
    assert len(K) == len(tri) + len(quad) == 2 * truth.PER_FAMILY * (2 if kinds == "mixed" else 1)
    for k, c in enumerate(tri):
        np.testing.assert_array_equal(K[k], truth.to_node_major(oracle.element_tri3(xyz[c], mat), 3))
    for k, c in enumerate(quad):
        np.testing.assert_array_equal(K[len(tri) + k], truth.to_node_major(oracle.element_quad4(xyz[c], mat), 4))
    # ... and what the assembly paths read from the blocks of K
    for k, c in enumerate(list(tri) + list(quad)):
        np.testing.assert_array_equal(K[k], truth.element_blocks(*K_unc, c))


@pytest.mark.parametrize("planted", [1e-9, 0.0])
def test_a_bending_error_the_product_test_accepts_is_over_the_budget(planted):
    """The gap the product paths of the GPU test close: the bending entries of a thin flat triangle (T3, t = 1e-3) wrong by 1e-9
    of themselves pass the bound of test_element_product_matches_the_oracle (1e-12 of a row scale that the membrane entries
    make), and are over the bending budget; with nothing planted both pass."""
    from tests import test_gpu_prescribed as product_test  # (its import builds the library where it is missing; no GPU)

    e = int(np.flatnonzero(FX["T3_mat"][:, 2] == 1e-3)[0])
    mat = oracle.material(*truth.material_of(FX, "T3", e))
    xyz, tri, quad = truth.isolated_mesh([FX["T3_xyz"][e]])
    K = truth.to_node_major(oracle.element_tri3(xyz, mat), 3)
    K[truth.class_masks(3, int(FX["T3_normal"][e]))["bending"]] *= 1.0 + planted
    product = _dense_product([K], tri, 3)
    x = np.random.default_rng(7).uniform(-1.0, 1.0, 18)
    K_unc, _ = pr.matrices(xyz, tri, quad, mat, np.zeros(3, np.uint8))
    ratio = product_test.product_bound_ratio(product(x), oracle.spmv(*K_unc, x), K_unc, x)
    print("planted %.0e: max |y - y_ref| / (1e-12 S_a) = %.2e" % (planted, ratio))
    assert ratio <= 1.0
    Kp = truth.probe_element_matrices(product, 3, tri)
    worst = {m: float(v.max()) for m, v in truth.family_errors(FX, "T3", Kp, elements=[e]).items()}
    over = [b[0] for b in truth.check(FX, "T3", worst)]
    print("planted %.0e: over the budget %s, bending %.2e" % (planted, over, worst["bending"]))
    if planted:  # (the whole-matrix norm may or may not see it: that depends on the element's size)
        assert "bending" in over and "membrane" not in over and "drilling" not in over
    else:
        assert over == []


def _oracle_own(bending_from_context):
    """truth.family_worst's `evaluate` by the FP64 oracle for an "own" path: every element with its row of the section table;
    bending_from_context: the bending entries scaled as if cp = E t^3 / 12 (1 - nu^2) were the context's"""
    def cp(nu, E, t):
        return E * t ** 3 / (12.0 * (1.0 - nu * nu))

    def evaluate(path, material, tri_xyz, quad_xyz, tri_mat, quad_mat):
        assert path[2] == "own" and material[:3] == truth.OWN_CONTEXT
        X = list(tri_xyz or []) + list(quad_xyz or [])
        table, index = truth.section_table(list(tri_mat or []) + list(quad_mat or []))
        assert len(table) > 1 and len(index) == len(X)
        out = []
        for x, row in zip(X, index):
            nodes = len(x)
            m = oracle.material(*table[row], material[3])
            K = truth.to_node_major((oracle.element_tri3 if nodes == 3 else oracle.element_quad4)(x, m), nodes)
            if bending_from_context:
                normal = int(np.argmax(np.abs(np.cross(x[1] - x[0], x[2] - x[0]))))
                K[truth.class_masks(nodes, normal)["bending"]] *= cp(*material[:3]) / cp(*table[row])
            out.append([K])
        nt = 0 if tri_xyz is None else len(tri_xyz)
        return out[:nt], out[nt:]
    return evaluate


def test_a_section_that_is_ignored_is_over_the_budget():
    """Q4 in one mesh with a section per thickness: evaluated by the oracle it is within the budgets (they are made of the
    oracle's own errors: the reference alone stays within them); with the bending constant of the context instead of the
    section's it is not."""
    path = ("k_element_matrices", None, "own")
    right = truth.family_worst(FX, "Q4", path, _oracle_own(False))
    assert truth.check(FX, "Q4", right) == []
    for m in truth.metrics_of("Q4"):  # (the oracle through the helper's plumbing is the oracle of the fixture)
        np.testing.assert_allclose(right[m], FX["Q4_err_" + m].max(), rtol=1e-9, atol=1e-30)
    wrong = truth.family_worst(FX, "Q4", path, _oracle_own(True))
    over = [b[0] for b in truth.check(FX, "Q4", wrong)]
    print("bending constant of the context: over the budget", over, "bending %.2e" % wrong["bending"])
    assert "bending" in over and "membrane" not in over and "drilling" not in over
