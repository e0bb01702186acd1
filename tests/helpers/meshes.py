"""Mesh fixtures of the tests: the Python mirror of the reference's meshGen and XDA/_f readers lives in the
product package (fem-shell_amd/meshgen.py, also used by bench.py); re-exported here under its old name."""
import importlib as _importlib

_m = _importlib.import_module("fem-shell_amd.meshgen")
globals().update({k: getattr(_m, k) for k in dir(_m) if not k.startswith("__")})


def delaunay_patch(n_pts, seed, strips=True):
    """Random Delaunay triangulation of a curved patch (valences 3..12) whose nodes are numbered strip by strip, so that 32
    consecutive nodes are a compact group: irregular slot widths, chunk counts and element lists per slice, but few enough
    elements per slice for the pipelined assembly kernel (tests of both assembly kernels).  Returns (xyz, tri)."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(seed)
    uv = rng.uniform(0.0, 1.0, size=(n_pts, 2))
    tri = Delaunay(uv).simplices.astype(np.int32)
    p, q, r = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
    area = 0.5 * np.abs((q[:, 0] - p[:, 0]) * (r[:, 1] - p[:, 1]) - (q[:, 1] - p[:, 1]) * (r[:, 0] - p[:, 0]))
    tri = tri[area > 0.02 * area.mean()]  # no slivers on the hull
    used = np.unique(tri)
    width = 4.0 / np.sqrt(n_pts)
    key = np.floor(uv[used, 1] / width) * 4.0 + uv[used, 0] if strips else rng.uniform(size=len(used))
    order = used[np.argsort(key, kind="stable")]
    remap = -np.ones(n_pts, dtype=np.int64)
    remap[order] = np.arange(len(order))
    tri = remap[tri].astype(np.int32)
    uv2 = uv[order]
    xyz = np.stack([3.0 * uv2[:, 0], 2.0 * uv2[:, 1], 0.3 * np.sin(3.0 * uv2[:, 0]) * np.cos(2.0 * uv2[:, 1])], axis=1)
    return xyz, tri


# ------------------------------------------------------------------ meshes at the limits of the plan's encodings
# Deterministic, no random state, every element well shaped (a planar fan of valence 300 would have angles of 1.2 degrees).

def coil(v, hub_last=True):
    """A fan of v near-equilateral triangles wound round its hub many times: ring nodes (cos k, sin k, 0.4 sin 0.61k),
    k = 0..v in radians, the hub at the origin numbered last (or first), triangles (hub, k, k+1).  v + 2 nodes; the
    surface passes through itself, which the finite-element arithmetic does not care about.  Returns (xyz, tri)."""
    k = np.arange(v + 1, dtype=np.float64)
    ring = np.stack([np.cos(k), np.sin(k), 0.4 * np.sin(0.61 * k)], axis=1)
    if hub_last:
        xyz, hub, first = np.concatenate([ring, np.zeros((1, 3))]), v + 1, 0
    else:
        xyz, hub, first = np.concatenate([np.zeros((1, 3)), ring]), 0, 1
    tri = np.array([[hub, first + i, first + i + 1] for i in range(v)], dtype=np.int32)
    return xyz, tri


def _petal_nodes(v):
    k = np.arange(v, dtype=np.float64)
    a = np.stack([np.cos(k), np.sin(k), 0.3 * np.sin(0.61 * k)], axis=1)
    b = np.stack([np.cos(k + 1.1), np.sin(k + 1.1), 0.3 * np.sin(0.61 * k + 0.5)], axis=1)
    xyz = np.concatenate([np.stack([a, a + b, b], axis=1).reshape(-1, 3), np.zeros((1, 3))])  # petal k: 3k, 3k+1, 3k+2; hub last
    return xyz, 3 * v


def quad_petals(v):
    """v planar rhombi (hub, a_k, a_k + b_k, b_k) round a hub at the origin that is numbered last; every petal has three
    nodes of its own: 3v + 1 nodes.  Returns (xyz, quad)."""
    xyz, hub = _petal_nodes(v)
    quad = np.array([[hub, 3 * k, 3 * k + 1, 3 * k + 2] for k in range(v)], dtype=np.int32)
    return xyz, quad


def mixed_petals(v):
    """quad_petals with every odd petal cut into the two triangles of its rhombus.  Returns (xyz, tri, quad)."""
    xyz, hub = _petal_nodes(v)
    quad = np.array([[hub, 3 * k, 3 * k + 1, 3 * k + 2] for k in range(0, v, 2)], dtype=np.int32).reshape(-1, 4)
    tri = np.array([t for k in range(1, v, 2) for t in ([hub, 3 * k, 3 * k + 1], [hub, 3 * k + 1, 3 * k + 2])],
                   dtype=np.int32).reshape(-1, 3)
    return xyz, tri, quad


def _min_angle_deg(p, q, r):
    worst = 180.0
    for a, b, c in ((p, q, r), (q, r, p), (r, p, q)):
        u, w = b - a, c - a
        worst = min(worst, np.degrees(np.arccos(np.clip(u @ w / (np.linalg.norm(u) * np.linalg.norm(w)), -1.0, 1.0))))
    return worst


def clique(m, offset_strips=True):
    """m nodes on a Fibonacci sphere, triangles chosen greedily until every pair of nodes is an edge: the smallest
    uncovered pair (a, b) takes, among the third nodes l that leave all three angles >= 15 degrees, the one that covers
    the most still-uncovered pairs of (a, l), (b, l) -- ties to the lowest l.  Every node is a neighbour of every other:
    with m <= 32 all transposed products of symmetric storage stay inside the slice.
    offset_strips: a structured strip of 32 nodes (30 triangles) is numbered before the clique and another after it, each
    joined to the clique by two triangles, so the clique is slice 1 of three.  Returns (xyz, tri)."""
    i = np.arange(m) + 0.5
    phi, theta = np.arccos(1.0 - 2.0 * i / m), np.pi * (1.0 + np.sqrt(5.0)) * i
    pts = np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)], axis=1)
    ok = np.zeros((m, m, m), dtype=bool)
    for a in range(m):
        for b in range(a + 1, m):
            for l in range(m):
                if l != a and l != b:
                    ok[a, b, l] = _min_angle_deg(pts[a], pts[b], pts[l]) >= 15.0
    covered = np.eye(m, dtype=bool)
    tris = []
    for a in range(m):
        for b in range(a + 1, m):
            if covered[a, b]:
                continue
            best, gain = -1, -1
            for l in range(m):
                if ok[a, b, l]:
                    g = int(not covered[a, l]) + int(not covered[b, l])
                    if g > gain:
                        best, gain = l, g
            assert best >= 0, "no well-shaped triangle on the pair (%d, %d)" % (a, b)
            tris.append([a, b, best])
            for p, q in ((a, b), (a, best), (b, best)):
                covered[p, q] = covered[q, p] = True
    tri = np.array(tris, dtype=np.int32)
    if not offset_strips:
        return pts, tri

    def strip(c0, c1):
        """32 nodes (16 x 2, spacing 0.5) standing off the sphere above the clique nodes c0, c1; node 2i + j; the last two
        are the ones next to the clique"""
        radial = (pts[c0] + pts[c1]) / np.linalg.norm(pts[c0] + pts[c1])
        across = pts[c1] - pts[c0]
        across -= (across @ radial) * radial
        across /= np.linalg.norm(across)
        mid = 0.5 * (pts[c0] + pts[c1])
        xyz = np.array([mid + (0.45 + 0.5 * (15 - ii)) * radial + 0.5 * (jj - 0.5) * across for ii in range(16) for jj in range(2)])
        cells = [t for ii in range(15) for t in ([2 * ii, 2 * ii + 2, 2 * ii + 3], [2 * ii, 2 * ii + 3, 2 * ii + 1])]
        return xyz, np.array(cells, dtype=np.int32)

    xa, ta = strip(0, 1)
    xb, tb = strip(m - 1, m - 2)
    first_b = 32 + m
    joins = np.array([[30, 32 + 0, 31], [31, 32 + 0, 32 + 1],
                      [first_b + 30, 32 + m - 1, first_b + 31], [first_b + 31, 32 + m - 1, 32 + m - 2]], dtype=np.int32)
    xyz = np.concatenate([xa, pts, xb])
    for t in joins:
        assert _min_angle_deg(*xyz[t]) >= 15.0
    return xyz, np.concatenate([ta, tri + 32, tb + first_b, joins]).astype(np.int32)


def many_hubs(n_hubs, v):
    """n_hubs coils of v triangles each, side by side, every ring with nodes of its own and the hubs numbered last: with 32
    hubs the last slice touches 32 v elements.  Returns (xyz, tri)."""
    ring, _ = coil(v)
    ring = ring[:-1]
    xyz = np.concatenate([ring + [3.0 * h, 0.0, 0.0] for h in range(n_hubs)] + [np.array([[3.0 * h, 0.0, 0.0] for h in range(n_hubs)])])
    tri = np.array([[n_hubs * (v + 1) + h, h * (v + 1) + i, h * (v + 1) + i + 1] for h in range(n_hubs) for i in range(v)], dtype=np.int32)
    return xyz, tri
