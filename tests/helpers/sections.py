"""Shell sections (femshell_set_sections): the reference of the tests and their meshes.

K is a sum over elements, so the CPU oracle -- which knows one material per call -- gives the matrix of a sectioned shell as
the sum of its assemblies of every section's elements, each with that section's material, on the pattern of the whole mesh
(split_sum).  libMesh's constrain_element_matrix_and_vector puts a 1.0 on a constrained diagonal per element, so those
entries add up to the element count as in one assembly.  F does not depend on the material.
"""
import numpy as np

from tests.helpers import meshes, oracle

NO_QUADS = np.zeros((0, 4), np.int32)
NO_TRIS = np.zeros((0, 3), np.int32)


class Case:
    """A mesh with sections: xyz, tri, quad, sections (n,3) of (nu, E, t), tri_section, quad_section, dmask, loads."""

    def __init__(self, xyz, tri, quad, sections, tri_section, quad_section, dmask, loads):
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        self.tri = NO_TRIS if tri is None else np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.quad = NO_QUADS if quad is None else np.ascontiguousarray(quad, dtype=np.int32).reshape(-1, 4)
        self.sections = np.ascontiguousarray(sections, dtype=np.float64).reshape(-1, 3)
        self.tri_section = np.zeros(0, np.int32) if tri_section is None else np.ascontiguousarray(tri_section, dtype=np.int32)
        self.quad_section = np.zeros(0, np.int32) if quad_section is None else np.ascontiguousarray(quad_section, dtype=np.int32)
        self.dmask = np.ascontiguousarray(dmask, dtype=np.uint8)
        self.loads = np.ascontiguousarray(loads, dtype=np.float64).reshape(len(self.xyz), 6)
        assert len(self.tri_section) == len(self.tri) and len(self.quad_section) == len(self.quad)

    @property
    def n_nodes(self):
        return len(self.xyz)

    def apply(self, fs, bc=True, loads=True):
        fs.set_mesh(self.xyz, self.tri, self.quad)
        if bc:
            fs.set_dirichlet(self.dmask)
        if loads:
            fs.set_loads(self.loads)
        fs.set_sections(self.sections, self.tri_section if len(self.tri) else None, self.quad_section if len(self.quad) else None)
        return fs


def split_sum(xyz, tri, quad, sections, tri_section, quad_section, dirichlet=None, flags=oracle.REF_DEFAULT):
    """(rowptr, colidx, vals_ref): the oracle's assembly section by section on the whole mesh's pattern, summed."""
    tri = NO_TRIS if tri is None else np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    quad = NO_QUADS if quad is None else np.ascontiguousarray(quad, dtype=np.int32).reshape(-1, 4)
    rowptr, colidx = oracle.bsr_pattern(len(xyz), tri, quad)
    vals = np.zeros((len(colidx), 6, 6))
    for s, (nu, E, t) in enumerate(np.asarray(sections, dtype=np.float64).reshape(-1, 3)):
        ts = tri[np.asarray(tri_section) == s] if len(tri) else NO_TRIS
        qs = quad[np.asarray(quad_section) == s] if len(quad) else NO_QUADS
        if len(ts) + len(qs) == 0:
            continue
        vals += oracle.assemble(xyz, ts, qs, oracle.material(nu, E, t, flags), dirichlet, None, pattern=(rowptr, colidx))[2]
    return rowptr, colidx, vals


def reference(case, flags=oracle.REF_DEFAULT):
    """(rowptr, colidx, vals_ref, F) of a case with its constraints and loads."""
    r, c, v = split_sum(case.xyz, case.tri, case.quad, case.sections, case.tri_section, case.quad_section, case.dmask, flags)
    nu, E, t = case.sections[0]
    F = oracle.assemble(case.xyz, case.tri, case.quad, oracle.material(nu, E, t, flags), case.dmask, case.loads, pattern=(r, c))[3]
    return r, c, v, F


def element_sum(case, flags=oracle.REF_DEFAULT):
    """The unconstrained K of a case from single elements (oracle.element_tri3 / element_quad4, each with its own material),
    scattered in Python onto the block pattern: pins split_sum itself."""
    rowptr, colidx = oracle.bsr_pattern(case.n_nodes, case.tri, case.quad)
    vals = np.zeros((len(colidx), 6, 6))
    where = {}
    for a in range(case.n_nodes):
        for q in range(rowptr[a], rowptr[a + 1]):
            where[(a, int(colidx[q]))] = q
    mats = [oracle.material(nu, E, t, flags) for nu, E, t in case.sections]
    for conn, sec, elem in ((case.tri, case.tri_section, oracle.element_tri3), (case.quad, case.quad_section, oracle.element_quad4)):
        for e in range(len(conn)):
            nn = conn.shape[1]
            Ke = elem(case.xyz[conn[e]], mats[sec[e]]).reshape(6, nn, 6, nn)  # variable-major: Ke[nn*al + i, nn*be + j]
            for i in range(nn):
                for j in range(nn):
                    vals[where[(int(conn[e, i]), int(conn[e, j]))]] += Ke[:, i, :, j]
    return rowptr, colidx, vals


# ------------------------------------------------------------------ cases

THREE = np.array([[0.3, 2e5, 0.05], [0.25, 7e4, 0.1], [0.33, 1e5, 0.025]])


def curved_patch(nx, ny, seed=3):
    """the curved, slightly irregular triangle patch of tests/test_gpu_parity.py (curved_mesh)"""
    m = meshes.structured(nx, ny, 0, 0, 4, 3, kind="t", ul_lr=bool(seed & 1), bcids=(0, -1, 1, -1))
    rng = np.random.default_rng(seed)
    m.xyz[:, 2] = 0.3 * np.sin(1.3 * m.xyz[:, 0]) * np.cos(0.7 * m.xyz[:, 1])
    m.xyz[:, :2] += rng.uniform(-0.02, 0.02, size=(m.n_nodes, 2))
    m.loads = rng.normal(size=(m.n_nodes, 6))
    return m


def strips_of(xyz, conn, n_strips=3):
    """section of an element: the strip along x its centroid lies in"""
    cx = xyz[conn][:, :, 0].mean(axis=1)
    lo, hi = xyz[:, 0].min(), xyz[:, 0].max()
    return np.minimum((n_strips * (cx - lo) / (hi - lo)).astype(np.int32), n_strips - 1)


def three_strips(nx=24, ny=18, sections=THREE):
    """curved patch in three strips along x (nodes are numbered row by row along x: the rows of a rank of a row partition
    are bands in y, so every section boundary crosses every rank cut)"""
    m = curved_patch(nx, ny)
    return Case(m.xyz, m.tri, None, sections, strips_of(m.xyz, m.tri), None, m.dirichlet_mask(), m.loads)


def ibeam(t_web=0.25, t_flange=0.5, E=1e4, nu=0.3):
    """the thesis' Test E I-beam (80 triangles): web and flanges by the largest component of the element normal"""
    m = meshes.load_example("test_E_uvw_t")
    a, b, c = (m.xyz[m.tri[:, i]] for i in range(3))
    k = np.abs(np.cross(b - a, c - a)).argmax(axis=1)
    counts = np.bincount(k, minlength=3)
    web_axis = int(np.flatnonzero(counts == 16)[0])
    assert counts.sum() == 80 and counts[web_axis] == 16
    sec = np.where(k == web_axis, 0, 1).astype(np.int32)
    return Case(m.xyz, m.tri, None, [[nu, E, t_web], [nu, E, t_flange]], sec, None, m.dirichlet_mask(), m.loads)


def mixed_patch(sections=THREE):
    """the mixed quadrilateral + triangle patch of tests/test_gpu_parity.py (test_mixed_tri_quad_mesh_matches_oracle),
    in three strips along x"""
    q = meshes.structured(6, 9, 0, 0, 3, 4.5, kind="q", bcids=(-1, 1, -1, -1))
    t = meshes.structured(6, 9, 3, 0, 6, 4.5, kind="t", ul_lr=True)
    nq = q.n_nodes
    remap = np.arange(t.n_nodes) + nq
    for j in range(10):
        remap[j * 7] = j * 7 + 6
    keep = np.ones(t.n_nodes, dtype=bool)
    keep[::7] = False
    new_id = np.cumsum(keep) - 1 + nq
    final = np.where(keep, new_id, remap)
    xyz = np.vstack([q.xyz, t.xyz[keep]])
    tri = final[t.tri].astype(np.int32)
    xyz[:, 2] = 0.4 * np.sin(0.9 * xyz[:, 0])
    dmask = np.zeros(len(xyz), dtype=np.uint8)
    dmask[:7] = 0x3F
    loads = np.random.default_rng(2).normal(size=(len(xyz), 6))
    return Case(xyz, tri, q.quad, sections, strips_of(xyz, tri), strips_of(xyz, q.quad), dmask, loads)


def wide_sections(n, seed):
    """n sections: nu in [0, 0.45], E over three decades, t over two"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.0, 0.45, n), 10.0 ** rng.uniform(3.0, 6.0, n), 10.0 ** rng.uniform(-2.0, 0.0, n)], axis=1)


def delaunay_random(n_pts=3000, seed=2, n_sections=7):
    """the Delaunay shell of tests/test_gpu_parity.py (test_unstructured_delaunay_shell), a random section per element"""
    from tests.test_gpu_parity import delaunay_shell

    xyz, tri = delaunay_shell(n_pts, seed)
    n = len(xyz)
    rng = np.random.default_rng(seed)
    dmask = np.zeros(n, dtype=np.uint8)
    dmask[xyz[:, 0] < 0.15] = 0x3F
    dmask[rng.integers(0, n, 5)] |= 0x07
    loads = rng.normal(size=(n, 6))
    sec = rng.integers(0, n_sections, len(tri)).astype(np.int32)
    return Case(xyz, tri, None, wide_sections(n_sections, seed + 100), sec, None, dmask, loads)


def tapered_panel(nx=70, ny=45, ratio=4.0, swaps=()):
    """structured curved panel (the pipelined assembly kernel's kind of mesh), ONE SECTION PER ELEMENT: the thickness
    tapers linearly along x by `ratio`.  swaps: positions inside every 32-node slice whose nodes change places with the
    next slice's -- every foreign node brings elements of its own into the slice's list (slices that touch more elements)."""
    m = meshes.structured(nx, ny, 0, 0, 0.1 * nx, 0.1 * ny, kind="t", ul_lr=True)
    xyz, tri = m.xyz.copy(), m.tri
    xyz[:, 2] = 0.3 * np.sin(0.9 * xyz[:, 0]) * np.cos(0.7 * xyz[:, 1])
    n = len(xyz)
    if len(swaps):
        perm = np.arange(n)
        for k in range(0, n // 32 - 1, 2):
            for off in swaps:
                a, b = 32 * k + off, 32 * (k + 1) + off
                perm[a], perm[b] = perm[b], perm[a]
        new_of_old = np.empty(n, np.int64)
        new_of_old[perm] = np.arange(n)
        xyz, tri = xyz[perm], new_of_old[tri].astype(np.int32)
    cx = xyz[tri][:, :, 0].mean(axis=1)
    t = 0.02 * (1.0 + (ratio - 1.0) * (cx - cx.min()) / (cx.max() - cx.min()))
    sections = np.stack([np.full(len(tri), 0.3), np.full(len(tri), 2.1e5), t], axis=1)
    rng = np.random.default_rng(12)
    dmask = np.zeros(n, np.uint8)
    dmask[rng.choice(n, n // 9, replace=False)] = rng.integers(1, 64, n // 9).astype(np.uint8)
    loads = rng.normal(size=(n, 6))
    return Case(xyz, tri, None, sections, np.arange(len(tri), dtype=np.int32), None, dmask, loads)


# positions swapped between neighbouring slices of a 40 x 30 panel: 143 elements in the fullest slice -- more than the
# pipelined kernel takes with sections (134), fewer than it takes without (150)
BETWEEN_THE_CAPS = dict(nx=40, ny=30, swaps=(3, 9, 15, 21, 27, 30))
