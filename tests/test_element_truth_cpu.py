"""tests/golden/element_truth.npz is what the quad-precision build of the oracle's element path computes here, the errors
of the FP64 oracle stored in it are the FP64 oracle's, and the statements the GPU test (tests/test_gpu_element_truth.py)
leans on hold: every stored element is well enough conditioned, the two builds agree on the committed goldens, and on the
flat families the FP64 oracle itself has exact zeros wherever the truth has them."""
import os

import numpy as np
import pytest

from tests.helpers import meshes, oracle, oracle_quad, truth

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
