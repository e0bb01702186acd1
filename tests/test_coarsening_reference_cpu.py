"""Why tests/test_gpu_coarsening.py holds the device-built hierarchy to the restatement operator by operator: slips a coarsening kernel
could make, planted into one step of the restatement itself, move that step's P or A_c at least a hundred times past the bound the
GPU case holds it to, while flexible PCG around the planted hierarchy still converges -- the solve tests cannot see them.  Each bug
is planted on the mesh, knobs and step of the GPU case that targets it.  CPU only (the CPU oracle's K, amg_oracle.setup)."""
import numpy as np
import pytest

from oracle import amg_oracle
from tests.helpers import hierarchy, oracle


def _problem(kind):
    from tests.test_gpu_amg import _fan_mesh, _poor_shell

    if kind in ("roof", "cylinder"):
        from tests.helpers import meshes

        m = meshes.scordelis_lo(48) if kind == "roof" else meshes.pinched_cylinder(80, 80)
        xyz, tri, dm, loads, mat = m.xyz, m.tri, m.dirichlet_mask(), m.loads, m.material
        opts = dict(coarsest_nodes=60, tri=tri)
    elif kind == "fan":
        xyz, tri = _fan_mesh(80, 12)
        dm = np.zeros(len(xyz), dtype=np.uint8)
        dm[np.hypot(xyz[:, 0], xyz[:, 1]) > 11.5] = 0x3F
        loads = np.zeros((len(xyz), 6))
        loads[:, 2] = 1.0
        mat = (0.3, 1e7, 0.2)
        opts = dict(coarsest_nodes=20, tri=tri)
    else:  # the 3,000-point shell of poor element quality, with the clusters of the patch smoother
        xyz, tri, dm, loads = _poor_shell(3000, 2)
        mat = (0.3, 7.0e4, 0.03)
        opts = dict(coarsest_nodes=60, tri=tri, patch_tau=0.8, patch_max=8)
    rp, ci, vals, F = oracle.assemble(xyz, tri, np.zeros((0, 4), dtype=np.int32), oracle.material(*mat), dm, loads)
    A = hierarchy.bsr(rp, ci, vals, len(xyz)).tobsr((6, 6))
    return A, F, xyz, dm, opts


def _z_sign(monkeypatch):
    """near_null_row: the z term of the rotation about x with the wrong sign, u = (0, z, y)"""
    plain = amg_oracle.rigid_body_modes

    def planted(xyz, dmask, normals=None):
        B = plain(xyz, dmask, normals)
        B[:, 1, 3] *= -1.0
        return B
    monkeypatch.setattr(amg_oracle, "rigid_body_modes", planted)


def _no_projection(monkeypatch):
    """near_null_row: the rotation modes without the projection onto the tangent plane (normals never arrived)"""
    plain = amg_oracle.rigid_body_modes
    monkeypatch.setattr(amg_oracle, "rigid_body_modes", lambda xyz, dmask, normals=None: plain(xyz, dmask, None))


def _at_step(monkeypatch, step, planted):
    """planted(A, B, lam, patch) takes the place of coarsen() in coarsening step `step`"""
    plain = amg_oracle.coarsen
    calls = []

    def coarsen(A, B, lam, bounds=None, patch=None):
        calls.append(1)
        return planted(A, B, lam, patch) if len(calls) - 1 == step else plain(A, B, lam, bounds, patch)
    monkeypatch.setattr(amg_oracle, "coarsen", coarsen)


def _cut_rows(monkeypatch, step=1):
    """k_amg_galerkin_mfma: only the first pass of 16 coarse columns per stored row (diagonal first, then ascending; with symmetric
    storage the diagonal and upper blocks, whose mirrors go with them), the rest left zero"""
    plain = amg_oracle.coarsen

    def planted(A, B, lam, patch):
        agg, P, Ac, Bc = plain(A, B, lam, patch=patch)
        n = Ac.shape[0] // 6
        sym = hierarchy.coarse_symmetric(n)
        Ab = Ac.tobsr((6, 6))
        Ab.sort_indices()
        rows = np.repeat(np.arange(n), np.diff(Ab.indptr))
        slot = np.zeros(len(Ab.indices), dtype=np.int64)
        for i in range(n):
            cols = Ab.indices[Ab.indptr[i]:Ab.indptr[i + 1]]
            pos = np.arange(len(cols))
            if sym:  # stored: the diagonal in slot 0, the upper blocks after it
                slot[Ab.indptr[i]:Ab.indptr[i + 1]] = np.where(cols >= i, pos - np.searchsorted(cols, i), -1)
            else:  # ELL order of a full row: the diagonal in slot 0
                slot[Ab.indptr[i]:Ab.indptr[i + 1]] = np.where(cols == i, 0, 1 + pos - (cols > i))
        keep = (slot >= 0) & (slot < hierarchy.GALERKIN_PASS)
        if sym:  # a lower block is the mirror of a stored upper one
            key = dict(zip(zip(rows[keep], Ab.indices[keep]), [True] * int(keep.sum())))
            lower = slot < 0
            keep[lower] = [(c, r) in key for r, c in zip(rows[lower], Ab.indices[lower])]
        data = Ab.data * keep[:, None, None]
        return agg, P, amg_oracle.sp.bsr_matrix((data, Ab.indices, Ab.indptr), shape=Ab.shape), Bc
    _at_step(monkeypatch, step, planted)


def _no_patch_correction(monkeypatch):
    """k_patch_prolongator not launched: P of level 0 smoothed with the point blocks on the clustered rows as well"""
    plain = amg_oracle.coarsen

    def planted(A, B, lam, patch):
        point = amg_oracle.bd_matrix(amg_oracle.block_diag_inverse(A))
        return plain(A, B, lam, patch=(patch[0], point))
    _at_step(monkeypatch, 0, planted)


def _large_aggregates_skipped(monkeypatch):
    """k_amg_tentative_qr: aggregates of more than 42 nodes left to an instantiation that skips them (zero rows of Q and R)"""
    plain = amg_oracle.tentative

    def planted(agg, na, B, ratios=None):
        Q, Bc = plain(agg, na, B, ratios)
        big = np.flatnonzero(np.bincount(agg, minlength=na) > hierarchy.QR_REGISTER_NODES)
        Q[np.isin(agg, big)] = 0.0
        Bc[big] = 0.0
        return Q, Bc
    monkeypatch.setattr(amg_oracle, "tentative", planted)


# bug: (mesh, planter, step it targets, operator, bound of the GPU case)
BUGS = {
    "z_sign": ("roof", _z_sign, 0, "P", hierarchy.P_TOL),
    "no_normal_projection": ("roof", _no_projection, 0, "P", hierarchy.P_TOL),
    "rows_cut_after_16_blocks": ("cylinder", _cut_rows, 1, "A", hierarchy.A_TOL),
    "no_patch_correction": ("poor_shell", _no_patch_correction, 0, "P", 2e-6),
    "aggregates_over_42_skipped": ("fan", _large_aggregates_skipped, 1, "P", hierarchy.P_TOL),
}

_cache = {}


def _reference(kind):
    if kind not in _cache:
        A, F, xyz, dm, opts = _problem(kind)
        levels = amg_oracle.setup(A, xyz, dm, **opts)
        _, h = amg_oracle.flexible_pcg(A, F, lambda v: amg_oracle.cycle(levels, 0, v, True), rtol=1e-10, max_it=2000)
        assert h[-1] <= 1e-10
        _cache[kind] = (A, F, xyz, dm, opts, levels, len(h))
    return _cache[kind]


def test_the_target_meshes_reach_what_the_bugs_touch():
    """The cylinder's second step and the fan's first build rows of more than 16 blocks, the fan's second step has aggregates on both
    sides of 42 nodes; the roof is curved; the poor shell has clusters."""
    cylinder = _reference("cylinder")[5]
    assert hierarchy.stored_widths(cylinder[2].A).max() > hierarchy.GALERKIN_PASS
    _, _, _, _, _, fan, _ = _reference("fan")
    assert hierarchy.stored_widths(fan[1].A).max() > hierarchy.GALERKIN_PASS
    sizes = np.bincount(fan[1].agg)
    assert sizes.max() > hierarchy.QR_REGISTER_NODES >= sizes.min(), (sizes.min(), sizes.max())
    _, _, xyz, _, opts, roof, _ = _reference("roof")
    nrm = amg_oracle.node_normals(xyz, opts["tri"])
    assert np.abs(nrm @ nrm[0]).min() < 0.99
    shell = _reference("poor_shell")[5]
    assert shell[0].patch is not None and shell[0].patch_label.max() + 1 > 500


@pytest.mark.parametrize("bug", list(BUGS))
def test_planted_coarsening_bugs_break_the_operator_bound_but_not_the_solve(monkeypatch, bug):
    kind, plant, step, op, bound = BUGS[bug]
    A, F, xyz, dm, opts, ref, its = _reference(kind)
    plant(monkeypatch)
    planted = amg_oracle.setup(A, xyz, dm, **opts)
    monkeypatch.undo()
    if op == "P":
        X, Y = planted[step].P, ref[step].P
    else:
        X, Y = planted[step + 1].A, ref[step + 1].A
    assert X.shape == Y.shape
    err = abs(X - Y).max() / abs(Y).max()
    assert err >= 100.0 * bound, (bug, err)
    _, h = amg_oracle.flexible_pcg(A, F, lambda v: amg_oracle.cycle(planted, 0, v, True), rtol=1e-10, max_it=2000)
    assert h[-1] <= 1e-10, (bug, len(h), its)
    print("%s: %s of step %d off by %.1e (bound %.0e), PCG %d iterations against %d" % (bug, op, step, err, bound, len(h), its))


def test_restated_patterns_are_the_structural_ones():
    """The library's patterns are structural (csrc/amg_setup.cpp bsr_multiply, csrc/amg_symbolic.hip): row i of P holds the aggregate
    of every neighbour of i, row I of A_c every column of the A P rows that reach I -- zero blocks included, such as the rows of P at
    clamped nodes.  The next aggregation sees those edges, so the restatement has to keep them: on the jittered Delaunay shell of
    tests/test_gpu_coarsening.py it otherwise ends with a level of 62 nodes where the library's has 45."""
    from tests.test_gpu_parity import delaunay_shell

    xyz, tri = delaunay_shell(6000, 4, jittered=True)
    dm = np.zeros(len(xyz), dtype=np.uint8)
    dm[xyz[:, 0] < 0.15] = 0x3F
    loads = np.zeros((len(xyz), 6))
    loads[:, 2] = 1.0
    rp, ci, vals, _ = oracle.assemble(xyz, tri, np.zeros((0, 4), dtype=np.int32), oracle.material(0.3, 7.0e4, 0.03), dm, loads)
    A = hierarchy.bsr(rp, ci, vals, len(xyz)).tobsr((6, 6))
    levels = amg_oracle.setup(A, xyz, dm, coarsest_nodes=60, tri=tri)
    assert [L.n for L in levels] == [5929, 705, 45]
    for L, N in zip(levels[:-1], levels[1:]):
        A_, P, Ac = L.A.tobsr((6, 6)), L.P.tobsr((6, 6)), N.A.tobsr((6, 6))
        prow = [sorted({int(L.agg[k]) for k in A_.indices[A_.indptr[i]:A_.indptr[i + 1]]}) for i in range(L.n)]
        for i in range(L.n):
            assert list(P.indices[P.indptr[i]:P.indptr[i + 1]]) == prow[i], i
        aprow = [sorted({J for k in A_.indices[A_.indptr[i]:A_.indptr[i + 1]] for J in prow[k]}) for i in range(L.n)]
        crow = [set() for _ in range(N.n)]
        for i in range(L.n):
            for I in prow[i]:
                crow[I].update(aprow[i])
        for I in range(N.n):
            assert list(Ac.indices[Ac.indptr[I]:Ac.indptr[I + 1]]) == sorted(crow[I]), I
    assert (np.abs(levels[0].P.tobsr((6, 6)).data).max(axis=(1, 2)) == 0.0).any()  # (zero blocks kept)
