"""The truths, bounds and models of tests/helpers/modal_truth.py without a GPU: every clean model passes the assertion the GPU
tests hold its kernel to (tests/test_gpu_modal_truth.py), every planted defect fails it at the shapes those tests run, and the
bitwise restatements (splitmix64, the start vectors, the sums in index order) agree with themselves."""
import numpy as np
import pytest

from tests.helpers import modal_truth as mt

# (nodes, padded nodes) of the GPU tests' meshes: 33 nodes in two slices, the 475-node patch, the 128-node grid whose last
# residual workgroup holds a node, and the large mesh of the grid-stride cases
GEOMETRIES = {"two_slices": (33, 64), "patch": (475, 480), "full_grid": (128, 128), "large": (177241, 177248)}


def masks(n, seed):
    """a Dirichlet mask with whole nodes, partial patterns and free nodes"""
    rng = np.random.default_rng(seed)
    dmask = np.zeros(n, np.uint8)
    pick = rng.choice(n, max(n // 4, 3), replace=False)
    dmask[pick] = rng.choice(np.array([0x3F, 0x07, 0x15], np.uint8), len(pick))
    dmask[-1] = 0x15  # the last node keeps free dofs
    return dmask


def fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


# ------------------------------------------------------------------ combine

def combine_inputs(q, n_out, extra, n6, seed=0):
    rng = np.random.default_rng(1000 + seed + sum(q) + 7 * n_out)
    sources = [rng.normal(size=(k, n6)) if k else None for k in q]
    return sources, rng.normal(size=(sum(q), n_out + extra))


@pytest.mark.parametrize("q,n_out,extra", mt.COMBINE_SHAPES)
def test_combine_model_passes_and_every_defect_that_can_show_fails(q, n_out, extra):
    n6 = 6 * 33
    sources, Cm = combine_inputs(q, n_out, extra, n6)
    share = mt.assert_combine(mt.combine_model(sources, Cm, n_out), sources, Cm, n_out)
    assert share <= 1.0
    for defect in mt.COMBINE_DEFECTS:
        Y = mt.combine_model(sources, Cm, n_out, defect)
        if mt.combine_defect_shows(defect, q, n_out, extra):
            fails(mt.assert_combine, Y, sources, Cm, n_out)
        else:
            mt.assert_combine(Y, sources, Cm, n_out)


def test_every_combine_defect_shows_at_some_shape_of_both_lists():
    for shapes in (mt.COMBINE_SHAPES, mt.COMBINE_SHAPES_THIN):
        for defect in mt.COMBINE_DEFECTS:
            assert any(mt.combine_defect_shows(defect, *s) for s in shapes), defect
    # every value the lists are to cover appears
    assert {s[0][0] for s in mt.COMBINE_SHAPES if len(s[0]) == 1} == {1, 31, 32, 33, 64, 65, 96}
    assert {s[0] for s in mt.COMBINE_SHAPES if len(s[0]) == 3} == {(12, 7, 12), (32, 32, 32), (5, 0, 3)}
    assert {s[1] for s in mt.COMBINE_SHAPES} == {1, 2, 3, 4, 5, 17, 63, 64} and ((96,), 64, 0) in mt.COMBINE_SHAPES
    assert {s[2] for s in mt.COMBINE_SHAPES} == {0, 3}  # ldc = n_out and ldc = n_out + 3


def test_selection_matrices_are_exact_and_catch_the_defects():
    n6 = 6 * 33
    caught = {d: 0 for d in mt.COMBINE_DEFECTS}
    for q, n_out, extra in mt.COMBINE_SHAPES:
        sources, _ = combine_inputs(q, n_out, extra, n6)
        Cm, pi, k = mt.selection(q, n_out, n_out + extra)
        assert Cm.shape == (sum(q), n_out + extra) and (np.count_nonzero(Cm[:, :n_out], axis=0) == 1).all()
        mt.assert_selection(mt.combine_model(sources, Cm, n_out), sources, pi, k)
        for defect in mt.COMBINE_DEFECTS:
            try:
                mt.assert_selection(mt.combine_model(sources, Cm, n_out, defect), sources, pi, k)
            except AssertionError:
                assert mt.combine_defect_shows(defect, q, n_out, extra)
                caught[defect] += 1
    assert all(caught.values()), caught
    # the map crosses sources and chunks, and repeats
    _, pi, _ = mt.selection((32, 32, 32), 64, 67)
    assert len(set(pi // 32)) == 3 and len(set(pi)) < len(pi)


# ------------------------------------------------------------------ residual

def residual_inputs(geometry, mb, seed=0):
    n, n_pad = GEOMETRIES[geometry]
    rng = np.random.default_rng(2000 + seed + mb)
    free = mt.free_dofs(masks(n, 3), n)
    KX, X = rng.normal(size=(mb, 6 * n)), rng.normal(size=(mb, 6 * n))  # non-zero on the constrained dofs too
    theta = 10.0 ** rng.uniform(0.0, 3.0, mb) + np.arange(mb)  # all distinct
    mass = rng.uniform(0.5, 2.0, 6 * n) * 1e-3
    return n, n_pad, free, KX, X, theta, mass


def residual_checks(R, norms, partials, KX, X, theta, cols, mass, free, n_pad):
    mt.assert_residual_rows(R, KX, X, theta, cols, mass, free)
    mt.assert_residual_sums(norms, partials)
    mt.assert_residual_partials(partials, R, mass, free, n_pad)
    mt.assert_residual_norms(norms, KX, X, theta, cols, mass, free, n_pad)


@pytest.mark.parametrize("geometry,shapes", [("two_slices", mt.RESIDUAL_SHAPES), ("patch", mt.RESIDUAL_SHAPES),
                                             ("full_grid", mt.RESIDUAL_SHAPES[:2]), ("large", mt.RESIDUAL_SHAPES[:1])])
def test_residual_model_passes_and_every_defect_that_can_show_fails(geometry, shapes):
    for mb, cols in shapes:
        n, n_pad, free, KX, X, theta, mass = residual_inputs(geometry, mb)
        args = (KX, X, theta, cols, mass, free, n_pad)
        residual_checks(*mt.residual_model(*args), *args)
        for defect in mt.RESIDUAL_DEFECTS:
            out = mt.residual_model(*args, defect=defect)
            if mt.residual_defect_shows(defect, cols, n, n_pad):
                fails(residual_checks, *out, *args)
            else:
                residual_checks(*out, *args)


def test_every_residual_defect_shows_somewhere_and_names_its_stage():
    shown = {d: 0 for d in mt.RESIDUAL_DEFECTS}
    for geometry, (n, n_pad) in GEOMETRIES.items():
        for mb, cols in mt.RESIDUAL_SHAPES:
            for d in mt.RESIDUAL_DEFECTS:
                shown[d] += mt.residual_defect_shows(d, cols, n, n_pad)
    assert all(shown.values()), shown
    # the defect of one stage fails the check of that stage alone
    n, n_pad, free, KX, X, theta, mass = residual_inputs("full_grid", 12)
    cols = (5, 0, 11, 3)
    args = (KX, X, theta, cols, mass, free, n_pad)
    R, norms, partials = mt.residual_model(*args, defect="sum_misses_last")
    mt.assert_residual_rows(R, *args[:6])
    mt.assert_residual_partials(partials, R, mass, free, n_pad)
    fails(mt.assert_residual_sums, norms, partials)
    R, norms, partials = mt.residual_model(*args, defect="stretch_loses_last")
    mt.assert_residual_rows(R, *args[:6])
    mt.assert_residual_sums(norms, partials)
    fails(mt.assert_residual_partials, partials, R, mass, free, n_pad)
    fails(mt.assert_residual_norms, norms, *args)
    R, norms, partials = mt.residual_model(*args, defect="theta_i")
    fails(mt.assert_residual_rows, R, *args[:6])
    mt.assert_residual_sums(norms, partials)
    mt.assert_residual_partials(partials, R, mass, free, n_pad)  # (they are held to the R they were formed from)


def test_stretches_and_the_index_order_sum():
    assert mt.stretches(64)[:2] == [(0, 1), (1, 2)] and mt.stretches(64)[64:] == [(64, 64)] * 64
    assert mt.stretches(480)[119] == (476, 480) and mt.stretches(480)[120] == (480, 480)
    s = mt.stretches(177248)
    assert s[0] == (0, 1385) and s[-1] == (127 * 1385, 177248) and 1385 > 256
    # index order, not any other: 1 + 2^-53 + 2^-53 rounds differently from the back
    p = np.array([[1.0, 2.0 ** -53, 2.0 ** -53] + [0.0] * 125, [2.0 ** -53, 2.0 ** -53, 1.0] + [0.0] * 125])
    np.testing.assert_array_equal(mt.index_order_sum(p), [1.0, 1.0 + 2.0 ** -52])
    # a NaN never passes a bound
    fails(mt.within, np.array([np.nan]), np.array([0.0], dtype=np.longdouble), np.array([1.0]))


# ------------------------------------------------------------------ block-Jacobi, mask

@pytest.mark.parametrize("n_cols", [1, 5, 32])
def test_block_jacobi_model_passes_and_every_defect_fails(n_cols):
    n = 475
    rng = np.random.default_rng(3000 + n_cols)
    A = rng.normal(size=(n, 6, 6))
    Dinv = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(6)  # symmetric, as the export unpacks the 21 stored words
    free = mt.free_dofs(masks(n, 4), n)
    R = rng.normal(size=(n_cols, 6 * n))  # non-zero on the constrained dofs
    assert mt.assert_block_jacobi(mt.bj_model(Dinv, R, free), Dinv, R, free) <= 1.0
    for defect in mt.BJ_DEFECTS:
        fails(mt.assert_block_jacobi, mt.bj_model(Dinv, R, free, defect), Dinv, R, free)


def test_mask_assertion():
    n = 33
    free = mt.free_dofs(masks(n, 5), n)
    X = np.random.default_rng(6).normal(size=(2, 6 * n))
    mt.assert_mask(np.where(free, X, 0.0), X, free)
    fails(mt.assert_mask, X, X, free)
    fails(mt.assert_mask, np.where(free, X, -0.0), X, free)  # -0.0 is not +0.0
    Y = np.where(free, X, 0.0)
    Y[1, np.flatnonzero(free)[0]] = np.nextafter(Y[1, np.flatnonzero(free)[0]], 1.0)
    fails(mt.assert_mask, Y, X, free)


# ------------------------------------------------------------------ start vectors

def test_splitmix64_restatements_agree():
    # the first outputs of the generator seeded with 0 (Vigna's splitmix64.c: the state advances by the golden gamma)
    assert mt.splitmix64(0) == 0xE220A8397B1DCDAF
    assert mt.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    xs = [0, 1, 5, 6 * 177240 + 5, (1 << 64) - 1, 0xD1B54A32D192ED03, 1 << 63]
    got = mt.splitmix64_np(np.array(xs, dtype=np.uint64))
    assert [int(v) for v in got] == [mt.splitmix64(x) for x in xs]
    # the mapping: the cell centres, the one rounding at the top, both ends
    assert mt.start_value(0) == 2.0 ** -53 - 1.0 and mt.start_value(((1 << 52) - 1) << 11) == -(2.0 ** -53)
    assert mt.start_value(((1 << 52) + 1) << 11) == 2.0 ** -51  # (2^52 + 1.5 rounds to the even 2^52 + 2)
    assert mt.start_value(1 << 63) == 0.0         # the one k in 2^53 that gives zero: 2^52 + 0.5 rounds to 2^52
    assert mt.start_value((1 << 64) - 1) == 1.0   # ... and the one that reaches the end
    assert mt.start_value(((1 << 53) - 2) << 11) < 1.0


@pytest.mark.parametrize("n_cols", [1, 12, 32, 96])
def test_start_model_is_self_consistent_and_every_defect_fails(n_cols):
    n = 475
    free = mt.free_dofs(masks(n, 7), n)
    X = mt.start_model(n, free, n_cols)
    mt.assert_start(X, free, n_cols)
    # against Python integers alone, entry by entry, on a sample
    rng = np.random.default_rng(8)
    for col, node, dof in zip(rng.integers(0, n_cols, 200), rng.integers(0, n, 200), rng.integers(0, 6, 200)):
        want = mt.start_entry(int(node), int(dof), int(col)) if free[6 * node + dof] else 0.0
        assert X[col, 6 * node + dof] == want
    internal_of = np.random.default_rng(9).permutation(n)
    fails(mt.assert_start, mt.start_model(n, free, n_cols, internal_of, "internal_id"), free, n_cols)
    inside = mt.start_model(n, free, n_cols, defect="column_inside")
    if n_cols > 1:
        fails(mt.assert_start, inside, free, n_cols)
    else:
        mt.assert_start(inside, free, n_cols)  # (column 0 has the key 0: one column cannot show it)
    unmasked = mt.start_model(n, np.ones(6 * n, dtype=bool), n_cols)
    fails(mt.assert_start, unmasked, free, n_cols)
