"""The GPU side of the Krylov-layer tests (tests/test_gpu_krylov_truth.py, tools/krylov_truth_report.py): meshes, contexts, and
the checks that drive the probes femshell_krylov_set / _launch / _get (csrc/api_krylov_probe.cpp) and hold what comes back to
tests/helpers/krylov_truth.py.  Every check returns {label: largest share of its bound used} (0.0 for a bitwise case) and raises
AssertionError where a bound or an equality is missed.

As a program -- python -m tests.helpers.krylov_cases OUT.npz MESH ... -- it runs the vector, product and gating checks and the
chains of those meshes under whatever environment it was started with and writes the shares: FEMSHELL_SLICE_GRID is read once per
process, so the case with more slices than workgroups runs in a child of its own."""
import sys

import numpy as np

from tests.helpers import jacobi_truth as jt
from tests.helpers import krylov_truth as kt
from tests.helpers import residual_truth as rt

MESHES = ("n33", "curved", "panel49", "strip", "mixed")
CHAIN_LENGTHS = (1, 2, 9, 17)


def mesh(name):
    """(xyz, tri, quad, dmask, loads, (nu, E, t)).  n33: one slice and a node, 31 padding rows in the live slice; curved: 475 nodes,
    15 slices -- an odd count, the half-wave of the last pair idles; panel49: 2401 nodes, 76 slices, the last one holds one node;
    strip: clamped all round, a third of its rows Dirichlet; mixed: quadrilaterals and triangles."""
    from tests.helpers import meshes, sections

    if name == "n33":
        m = meshes.structured(10, 2, 0, 0, 5, 1, kind="t", ul_lr=True, bcids=(-1, -1, 0, -1), factor=300.0, loading=2)
        mat = (0.3, 1e7, 0.5)
    elif name == "curved":
        m = sections.curved_patch(24, 18)
        mat = (0.3, 2e5, 0.05)
    elif name == "panel49":
        m = meshes.structured(48, 48, 0, 0, 6, 6, kind="t", ul_lr=True, bcids=(0, 0, 1, -1), factor=300.0, loading=2)
        mat = (0.3, 1e7, 0.5)
    elif name == "strip":
        return jt.spectral_mesh("strip")
    elif name == "mixed":
        c = sections.mixed_patch()
        return c.xyz, c.tri, c.quad, c.dmask, c.loads, tuple(c.sections[0])
    else:
        raise ValueError(name)
    return m.xyz, m.tri if len(m.tri) else None, m.quad if len(m.quad) else None, m.dirichlet_mask(), m.loads, mat


def context(pkg, name, pc="jacobi", **pc_options):
    """an assembled context whose block-Jacobi inverse (and hierarchy, under "amg") is built: what the probes ask for"""
    xyz, tri, quad, dmask, loads, mat = mesh(name)
    fs = pkg.FemShell(*mat, device=0)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.assemble()
    if pc == "amg":
        fs.set_preconditioner("amg", coarsest_nodes=60, **pc_options)
    fs.block_jacobi_export(0)
    fs.free = (1 - ((np.asarray(dmask, dtype=np.uint8)[:, None] >> np.arange(6)) & 1)).astype(np.float64)  # 1 on the free dofs
    return fs


# ------------------------------------------------------------------ the state of the probe

VECTORS = ("x", "r", "z", "p", "q", "sv", "b")


def set_scalars(fs, s):
    st = s.into_struct(fs_scalars_type(fs)())
    fs.krylov_set("scalars", st)


def fs_scalars_type(fs):
    return type(fs.krylov_get("scalars"))


def get_scalars(fs):
    return kt.Scalars.from_struct(fs.krylov_get("scalars"))


def raw_scalars(fs):
    return bytes(fs.krylov_get("scalars"))


def snapshot(fs):
    """every word the probes can reach: the vectors, the 4 G partial sums, the scalars, the history"""
    out = {v: fs.krylov_get(v) for v in VECTORS}
    out["partials"] = fs.krylov_get("partials", 4 * fs.krylov_grid())
    out["scalars"] = np.frombuffer(raw_scalars(fs), dtype=np.uint8).copy()
    cap = fs.krylov_get("history_cap")
    out["history"] = fs.krylov_get("history", cap) if cap > 0 else np.zeros(0)
    return out


def assert_untouched(before, after, label, but=()):
    for k in before:
        if k not in but:
            assert np.array_equal(kt.bits(before[k]) if before[k].dtype == np.float64 else before[k],
                                  kt.bits(after[k]) if after[k].dtype == np.float64 else after[k]), "%s: %s changed" % (label, k)


def fill(fs, rng, integer=False, **scalars):
    """random (or small-integer) vectors in all seven places, NaN in the partial sums, the given scalars; returns the vectors"""
    n = fs.n_nodes
    vec = {}
    for v in VECTORS:
        vec[v] = kt.small_integers(rng, (n, 6)) if integer else rng.standard_normal((n, 6)) * 10.0 ** rng.uniform(-2, 2, size=(n, 6))
        fs.krylov_set(v, vec[v])
    fs.krylov_set("partials", np.full(4 * fs.krylov_grid(), np.nan))
    set_scalars(fs, kt.Scalars(**scalars))
    return vec


def partial_sums(fs, array, count=None):
    """the words array G .. array G + count of the partial sums (count: the grid)"""
    G = fs.krylov_grid()
    count = G if count is None else count
    return fs.krylov_get("partials", 4 * G)[array * G:array * G + count]


def _same(a, b, label):
    assert np.array_equal(kt.bits(a), kt.bits(b)), "%s: not the same bits (first at %s)" % (label, np.argwhere(kt.bits(a) != kt.bits(b))[:1])
    return 0.0


def _minv(fs, B, r, z, label):
    want, budget = jt.apply_truth(B, r)
    return kt.within(z, want, budget)


# ------------------------------------------------------------------ (c) vector kernels and their partial sums

def check_vector_steps(fs, seed=0):
    """every block-Jacobi and flexible vector step on random and on small-integer states"""
    rng = np.random.default_rng(seed)
    B = fs.block_jacobi_export(0)
    b0 = fs.krylov_get("b")
    out = {}

    def dots(tag, integer, *pairs):
        for array, (name, a, b, minv) in enumerate(pairs):
            out["%s %s" % (tag, name)] = kt.assert_dot(partial_sums(fs, array), a, b, "%s %s" % (tag, name), exact=integer and not minv)

    for integer in (False, True):
        kind = "int" if integer else "rnd"
        alpha, beta = (1.0, 1.0) if integer else (0.8125 + rng.uniform() * 1e-3, -0.4375 + rng.uniform() * 1e-3)
        # cg_init, fresh and restart
        for restart in (0, 1):
            tag = "cg_init%d %s" % (restart, kind)
            v = fill(fs, rng, integer, alpha=alpha, beta=beta)
            fs.krylov_launch("cg_init", restart)
            g = {k: fs.krylov_get(k) for k in VECTORS}
            out[tag + " x"] = _same(g["x"], v["x"] if restart else np.zeros_like(v["x"]), tag + " x")
            out[tag + " r"] = _same(g["r"], v["b"] - v["q"] if restart else v["b"], tag + " r")
            out[tag + " z"] = _minv(fs, B, g["r"], g["z"], tag)
            out[tag + " p"] = _same(g["p"], g["z"], tag + " p")
            dots(tag, integer, ("r.z", g["r"], g["z"], True), ("r.r", g["r"], g["r"], False))
        # cgcg_init
        tag = "cgcg_init " + kind
        v = fill(fs, rng, integer)
        fs.krylov_launch("cgcg_init")
        g = {k: fs.krylov_get(k) for k in VECTORS}
        for k in ("x", "p", "sv"):
            out[tag + " " + k] = _same(g[k], np.zeros_like(v[k]), tag + " " + k)
        out[tag + " r"] = _same(g["r"], v["b"], tag + " r")
        out[tag + " z"] = _minv(fs, B, g["r"], g["z"], tag)
        dots(tag, integer, ("r.z", g["r"], g["z"], True), ("r.r", g["r"], g["r"], False))
        # cg_update without the gather (q is whole), cg_direction
        tag = "cg_update " + kind
        v = fill(fs, rng, integer, alpha=alpha, beta=beta)
        fs.krylov_launch("cg_update", 0)
        g = {k: fs.krylov_get(k) for k in VECTORS}
        out[tag + " x"] = kt.within(g["x"], *kt.axpy_truth(v["x"], alpha, v["p"]))
        out[tag + " r"] = kt.within(g["r"], *kt.axpy_truth(v["r"], -alpha, v["q"]))
        if integer:
            _same(g["x"], v["x"] + v["p"], tag + " x")
            _same(g["r"], v["r"] - v["q"], tag + " r")
        out[tag + " z"] = _minv(fs, B, g["r"], g["z"], tag)
        dots(tag, integer, ("r.z", g["r"], g["z"], True), ("r.r", g["r"], g["r"], False))
        for k in ("p", "q", "sv", "b"):
            _same(g[k], v[k], tag + " leaves " + k)
        tag = "cg_direction " + kind
        fs.krylov_launch("cg_direction")
        p = fs.krylov_get("p")
        out[tag + " p"] = kt.within(p, *kt.axpy_truth(g["z"], beta, v["p"]))
        # cgcg_update, the scalars as they are (step -1)
        tag = "cgcg_update " + kind
        v = fill(fs, rng, integer, alpha=alpha, beta=beta)
        fs.krylov_launch("cgcg_update", -1, 0)
        g = {k: fs.krylov_get(k) for k in VECTORS}
        out[tag + " p"] = kt.within(g["p"], *kt.axpy_truth(v["z"], beta, v["p"]))
        out[tag + " sv"] = kt.within(g["sv"], *kt.axpy_truth(v["q"], beta, v["sv"]))
        out[tag + " x"] = kt.within(g["x"], *kt.axpy_truth(v["x"], alpha, g["p"]))
        out[tag + " r"] = kt.within(g["r"], *kt.axpy_truth(v["r"], -alpha, g["sv"]))
        if integer:
            _same(g["p"], v["z"] + v["p"], tag + " p")
            _same(g["r"], v["r"] - (v["q"] + v["sv"]), tag + " r")
        out[tag + " z"] = _minv(fs, B, g["r"], g["z"], tag)
        dots(tag, integer, ("r.z", g["r"], g["z"], True), ("r.r", g["r"], g["r"], False))
        # the flexible recurrence's steps
        tag = "pcg_init " + kind
        v = fill(fs, rng, integer)
        fs.krylov_launch("pcg_init")
        g = {k: fs.krylov_get(k) for k in VECTORS}
        out[tag + " x"] = _same(g["x"], np.zeros_like(v["x"]), tag + " x")
        out[tag + " r"] = _same(g["r"], v["b"], tag + " r")
        dots(tag, integer, ("b.b", v["b"], v["b"], False))
        tag = "pcg_update " + kind
        v = fill(fs, rng, integer, alpha=alpha)
        fs.krylov_launch("pcg_update")
        g = {k: fs.krylov_get(k) for k in VECTORS}
        out[tag + " x"] = kt.within(g["x"], *kt.axpy_truth(v["x"], alpha, v["p"]))
        out[tag + " r"] = kt.within(g["r"], *kt.axpy_truth(v["r"], -alpha, v["q"]))
        dots(tag, integer, ("r.r", g["r"], g["r"], False), ("x.x", g["x"], g["x"], False))
        tag = "pcg_norm " + kind
        fs.krylov_set("partials", np.full(4 * fs.krylov_grid(), np.nan))
        fs.krylov_launch("pcg_norm")
        dots(tag, integer, ("r.r", g["r"], g["r"], False))
        tag = "pcg_dots " + kind
        fs.krylov_launch("pcg_dots")
        dots(tag, integer, ("r.z", g["r"], g["z"], False), ("z.q", g["z"], g["q"], False))
        tag = "minv_apply_norm " + kind
        fs.krylov_launch("minv_apply_norm")
        z = fs.krylov_get("z")
        out[tag + " z"] = _minv(fs, B, g["q"], z, tag)
        dots(tag, integer, ("z.z", z, z, True))
        tag = "copy_z_to_p " + kind
        fs.krylov_launch("copy_z_to_p")
        out[tag + " p"] = _same(fs.krylov_get("p"), z, tag + " p")
        tag = "two_dots " + kind
        sums = fs.krylov_launch("two_dots", 0, 4)[2]
        for name, got, a in (("x.x", sums[0], g["x"]), ("q.q", sums[1], g["q"])):
            out["%s %s" % (tag, name)] = kt.assert_dot([got], a, a, tag + " " + name, exact=integer)
    fs.krylov_set("b", b0)
    return out


def check_gathered_updates(fs, seed=0):
    """Symmetric storage, the update kernels as production runs them: the product leaves the direct part of K p (K z) in q and the
    transposed products beside the slots, and launch_cg_update(gather) / launch_cgcg_update(step, gather) collect them
    themselves (node_gather; the row's own loop over in_width / gat_slots / tbuf).  The whole q comes from a product that gathers
    explicitly -- held row by row to the exact K x in check_product -- and x, r, p, sv are held to the long-double update with
    it, z to the readers' bound, the partial sums to exact_dot of the device's own vectors.  A transposed product lost or
    doubled by a gather is an error of the size of a term of the row.  The folded steps take alpha and beta from folded_step."""
    rng = np.random.default_rng(seed)
    B = fs.block_jacobi_export(0)
    b0 = fs.krylov_get("b")
    out = {}

    def whole_then_direct(source):
        fs.krylov_launch("product", source, 0)
        q = fs.krylov_get("q")
        fs.krylov_launch("product", source, 1)
        assert not np.array_equal(q, fs.krylov_get("q")), "the deferred product left the whole q: nothing to gather"
        fs.krylov_set("partials", np.full(4 * fs.krylov_grid(), np.nan))
        return q

    def dots(tag, g):
        for array, (name, a, b) in enumerate((("r.z", g["r"], g["z"]), ("r.r", g["r"], g["r"]))):
            out["%s %s" % (tag, name)] = kt.assert_dot(partial_sums(fs, array), a, b, "%s %s" % (tag, name))

    for integer in (False, True):
        kind = "int" if integer else "rnd"
        alpha, beta = (1.0, 1.0) if integer else (0.8125 + rng.uniform() * 1e-3, -0.4375 + rng.uniform() * 1e-3)
        tag = "cg_update_gather " + kind
        v = fill(fs, rng, integer, alpha=alpha, beta=beta)
        q = whole_then_direct(0)
        fs.krylov_launch("cg_update", 1)
        g = {k: fs.krylov_get(k) for k in VECTORS}
        out[tag + " x"] = kt.within(g["x"], *kt.axpy_truth(v["x"], alpha, v["p"]))
        out[tag + " r"] = kt.within(g["r"], *kt.axpy_truth(v["r"], -alpha, q))
        out[tag + " z"] = _minv(fs, B, g["r"], g["z"], tag)
        dots(tag, g)
        for step in (-1, 0, 1):
            tag = "cgcg_update_gather step %d %s" % (step, kind)
            scal = dict(alpha=alpha, beta=beta)
            a_, b_ = alpha, beta
            if step >= 0:  # the folded step decides alpha and beta from red[] and its half of the ring
                ring_rz, ring_alpha = [99.0, 99.0], [98.0, 98.0]
                ring_rz[step], ring_alpha[step] = 3.7, 0.61
                scal = dict(rz=3.7, alpha=0.61, beta=0.23, rr=1.9, bb=41.3, tol2=0.77, iters=2, red=[2.3, 0.9, 51.0], ring_rz=ring_rz, ring_alpha=ring_alpha)
                model = kt.Scalars(**scal)
                a_, b_, done = kt.folded_step(model, step)
                assert done == 0
            v = fill(fs, rng, integer, **scal)
            w = whole_then_direct(1)
            fs.krylov_launch("cgcg_update", step, 1)
            g = {k: fs.krylov_get(k) for k in VECTORS}
            if step >= 0:
                kt.assert_scalars_equal(get_scalars(fs), model, tag)
            out[tag + " p"] = kt.within(g["p"], *kt.axpy_truth(v["z"], b_, v["p"]))
            out[tag + " sv"] = kt.within(g["sv"], *kt.axpy_truth(w, b_, v["sv"]))
            out[tag + " x"] = kt.within(g["x"], *kt.axpy_truth(v["x"], a_, g["p"]))
            out[tag + " r"] = kt.within(g["r"], *kt.axpy_truth(v["r"], -a_, g["sv"]))
            out[tag + " z"] = _minv(fs, B, g["r"], g["z"], tag)
            dots(tag, g)
    fs.krylov_set("b", b0)
    return out


def check_pc_apply(fs, seed=0):
    """the cycle as the flexible recurrence issues it (amg_apply on r into z, gated by the scalars) against femshell_pc_apply on the
    same vector: the same launches, the same bits (tests/test_gpu_cycle.py holds that entry point to the restated cycle)"""
    rng = np.random.default_rng(seed)
    b0 = fs.krylov_get("b")
    r = rng.standard_normal((fs.n_nodes, 6)) * fs.free
    fill(fs, rng)
    fs.krylov_set("r", r)
    fs.krylov_launch("pc_apply", 0)
    z = fs.krylov_get("z")
    assert np.array_equal(kt.bits(fs.krylov_get("r")), kt.bits(r))
    out = {"pc_apply z": _same(z, fs.pc_apply(r).reshape(-1, 6), "pc_apply z")}
    fs.krylov_set("b", b0)
    return out


def check_flexible_update_start(fs, symmetric, seed=0):
    """launch_pcg_update_start on a multigrid context: the update and its two sums, and -- symmetric storage -- the whole q it
    stores for the z.q of the next kernel.  (The start of the smoothing it writes to z is the cycle's business: tests/test_gpu_cycle.py,
    and the chain below, which is the solve bit for bit.)"""
    rng = np.random.default_rng(seed)
    b0 = fs.krylov_get("b")
    out = {}
    for integer in (False, True):
        kind = "int" if integer else "rnd"
        alpha = 1.0 if integer else 0.8125
        tag = "pcg_update_start " + kind
        v = fill(fs, rng, integer, alpha=alpha)
        q = v["q"]
        if symmetric:  # q = K p in two phases: the second is the kernel's
            fs.krylov_launch("product", 0, 0)
            q = fs.krylov_get("q")
            fs.krylov_launch("product", 0, 1)
        fs.krylov_launch("pcg_update_start", 1 if symmetric else 0)
        g = {k: fs.krylov_get(k) for k in VECTORS}
        out[tag + " q"] = _same(g["q"], q, tag + " q")
        out[tag + " x"] = kt.within(g["x"], *kt.axpy_truth(v["x"], alpha, v["p"]))
        out[tag + " r"] = kt.within(g["r"], *kt.axpy_truth(v["r"], -alpha, q))
        for array, (name, a) in enumerate((("r.r", g["r"]), ("x.x", g["x"]))):
            out["%s %s" % (tag, name)] = kt.assert_dot(partial_sums(fs, array), a, a, tag + " " + name, exact=integer and not symmetric)
        assert np.isfinite(g["z"]).all()
    fs.krylov_set("b", b0)
    return out


def check_product(fs, symmetric, seed=0):
    """the Krylov product as spmv_with_halo issues it and its fused dot against exact_dot(x, K x): x on every dof and on the free
    dofs only, small integers (where K x is not exact: K is no integer matrix), from p (sums at 0) and from z (sums at 2 G)"""
    rng = np.random.default_rng(seed)
    r, c, v, F = fs.export_bsr()
    K = (r, c, v)
    n = fs.n_nodes
    G = fs.krylov_grid()
    row_gamma = rt.gamma(6.0 * rt.blocks_per_row(K))
    b0 = fs.krylov_get("b")
    out = {}
    for xname, x in (("all", rng.standard_normal((n, 6))), ("free", rng.standard_normal((n, 6)) * fs.free),
                     ("int", kt.small_integers(rng, (n, 6))), ("scaled", rng.standard_normal((n, 6)) * 10.0 ** rng.uniform(-3, 3, size=(n, 6)))):
        truth, extra = kt.fused_dot_truth(K, x)
        Kx = -rt.exact(K, np.zeros(6 * n), x.reshape(-1))
        row_bound = row_gamma * rt.scale(K, np.zeros(6 * n), x.reshape(-1)) + kt.U * np.abs(Kx)
        for source in (0, 1):
            for defer in ((0, 1) if symmetric else (0,)):
                tag = "product %s from %s%s" % (xname, "pz"[source], " deferred" if defer else "")
                fill(fs, rng)
                fs.krylov_set("pz"[source], x)
                count, grid, _ = fs.krylov_launch("product", source, defer)
                assert grid == G and count in (0, G), (count, grid)
                sums = partial_sums(fs, 2 * source)
                assert np.isfinite(sums).all(), tag + ": a partial sum was not written"
                out[tag + " dot"] = kt.assert_dot(sums, x, Kx, tag, truth=truth, bound=extra)
                if defer:  # the direct part is in q: the explicit gather completes it
                    fs.krylov_launch("sym_gather")
                out[tag + " q"] = kt.within(fs.krylov_get("q").reshape(-1), Kx.astype(kt.LD), row_bound)
    fs.krylov_set("b", b0)
    return out


GATED_STEPS = (("cg_update", (0,)), ("cg_direction", ()), ("cgcg_update", (-1, 0)), ("cgcg_update", (0, 0)), ("cgcg_update", (1, 0)),
               ("pcg_update", ()), ("pcg_dots", ()), ("product", (0, 0)), ("product", (1, 0)), ("copy_z_to_p", ()))
UNGATED_STEPS = (("cg_init", (0,)), ("cgcg_init", ()), ("pcg_init", ()), ("pcg_norm", ()), ("minv_apply_norm", ()))


def check_gating(fs, symmetric, amg=False, seed=0):
    """done = 1 and done = -1 in the scalars: every gated step leaves every word as it was; the steps that start a solve run"""
    rng = np.random.default_rng(seed)
    b0 = fs.krylov_get("b")
    steps = list(GATED_STEPS)
    if symmetric:
        steps += [("cg_update", (1,)), ("cgcg_update", (-1, 1)), ("cgcg_update", (1, 1)), ("product", (0, 1)), ("product", (1, 1)), ("sym_gather", ())]
    if amg:
        steps += [("pcg_update_start", (1 if symmetric else 0,)), ("pc_apply", (0,)), ("pc_apply", (1,))]
    fs.krylov_set("history", np.full(4, -7.0))
    out = {}
    for done in (1, -1):
        fill(fs, rng, alpha=0.75, beta=0.5, done=done, red=[3, 2, 5], rz=4, bb=8, tol2=1, iters=2, ring_rz=[4, 4], ring_alpha=[0.75, 0.75])
        before = snapshot(fs)
        for step, args in steps:
            fs.krylov_launch(step, *args)
            assert_untouched(before, snapshot(fs), "%s%s on done = %d" % (step, args, done))
            out["gated %s%s done %d" % (step, args, done)] = 0.0
        for step, args in UNGATED_STEPS:
            fs.krylov_set("partials", np.full(4 * fs.krylov_grid(), np.nan))
            fs.krylov_launch(step, *args)
            assert np.isfinite(partial_sums(fs, 0)).all(), "%s did not run on done = %d" % (step, done)
            assert before["scalars"].tobytes() == raw_scalars(fs), "%s changed the scalars" % step
    fs.krylov_set("b", b0)
    return out


# ------------------------------------------------------------------ (d) the chains

def _start(fs, k):
    set_scalars(fs, kt.Scalars())  # (femshell_solve zeroes the scalars in front of every attempt)
    fs.krylov_set("history", np.full(k + 2, -7.0))
    fs.krylov_set("history_cap", k)


def _finish(fs, k):
    hist = fs.krylov_get("history", k + 2)
    assert (hist[k:] == -7.0).all(), "the history was written beyond its cap"
    return fs.krylov_get("x"), hist[:k], get_scalars(fs)


P = kt.PHASES


def chain_classic(fs, k, symmetric, rtol=0.0):
    """cg_classic's launches, one probe each"""
    _start(fs, k)
    fs.krylov_launch("cg_init", 0)
    fs.krylov_launch("scalar_step", 2, P["init"], 0, 0, -1, rtol=rtol)
    for _ in range(k):
        n = fs.krylov_launch("product", 0, 1)[0]
        fs.krylov_launch("scalar_step", 1, P["alpha"], n, 0, -1, rtol=rtol)
        fs.krylov_launch("cg_update", 1 if symmetric else 0)
        fs.krylov_launch("scalar_step", 2, P["beta"], 0, 0, -1, rtol=rtol)
        fs.krylov_launch("cg_direction")
    return _finish(fs, k)


def chain_single_reduction(fs, k, symmetric, fold, rtol=0.0):
    """cg_single_reduction's launches.  The folded loop closes its last iteration with a FUSED_STEP launch that does not reduce;
    scalar_step always reduces, so the chain's last step adds the same partial sums into the same red[] once more before the same
    phase -- the one place where the chain is not the production launch word for word."""
    G = fs.krylov_grid()
    gather = 1 if (fold and symmetric) else 0
    _start(fs, k)
    fs.krylov_launch("cgcg_init")
    len3 = fs.krylov_launch("product", 1, gather)[0] or G
    fs.krylov_launch("scalar_step", 3, P["fused_init"], G, len3, -1, rtol=rtol)
    for it in range(k):
        fs.krylov_launch("cgcg_update", ((it - 1) & 1) if (fold and it > 0) else -1, gather)
        len3 = fs.krylov_launch("product", 1, gather)[0] or G
        if fold:
            fs.krylov_launch("scalar_step", 3, P["none"], G, len3, P["fused_step"], rtol=rtol)
        else:
            fs.krylov_launch("scalar_step", 3, P["fused_step"], G, len3, -1, rtol=rtol)
    if fold:
        fs.krylov_launch("scalar_step", 3, P["fused_step"], G, len3, -1, rtol=rtol)
    return _finish(fs, k)


def chain_flexible(fs, k, symmetric, fused, rtol=0.0):
    """cg_amg's launches without refinement passes around the cycle (pc_apply); fused: FEMSHELL_AMG_FUSE bit 0 as the process has
    it -- the update kernel finishes the product and starts the cycle's pre-smoothing"""
    _start(fs, k)
    fs.krylov_launch("pcg_init")
    fs.krylov_launch("scalar_step", 1, P["flex_init"], 0, 0, -1, rtol=rtol)
    fs.krylov_launch("pc_apply", 0)
    fs.krylov_launch("pcg_dots")
    fs.krylov_launch("scalar_step", 1, P["flex_rz0"], 0, 0, -1, rtol=rtol)
    fs.krylov_launch("copy_z_to_p")
    defer = 1 if (fused and symmetric) else 0
    for _ in range(k):
        fs.krylov_launch("product", 0, defer)
        fs.krylov_launch("scalar_step", 1, P["alpha"], 0, 0, -1, rtol=rtol)
        fs.krylov_launch("pcg_update_start", defer) if fused else fs.krylov_launch("pcg_update")
        fs.krylov_launch("scalar_step", 2, P["flex_conv"], 0, 0, -1, rtol=rtol)
        fs.krylov_launch("pc_apply", 1 if fused else 0)
        fs.krylov_launch("pcg_dots")
        fs.krylov_launch("scalar_step", 2, P["flex_beta"], 0, 0, -1, rtol=rtol)
        fs.krylov_launch("cg_direction")
    return _finish(fs, k)


def assert_chain_is_the_solve(fs, chain, label, lengths=CHAIN_LENGTHS):
    """chain(k) -> (x, history words r.r / b.b, scalars) against solve(rtol = 0, max_it = k) on the same context, bit for bit"""
    out = {}
    for k in lengths:
        x, hist, s = chain(k)
        u, info = fs.solve(rtol=0.0, max_it=k)
        h = fs.residual_history()
        tag = "%s k=%d" % (label, k)
        assert info["iterations"] == k == s.iters and len(h) == k, (tag, info["iterations"], s.iters, len(h))
        _same(np.sqrt(hist), h, tag + " history")  # (residual_history hands out the roots of the words r.r / b.b in HBM)
        _same(x, u, tag + " x")
        assert h[-1] == info["rel_residual"] == np.sqrt(s.rr / s.bb), tag
        out[tag] = 0.0
    return out


# ------------------------------------------------------------------ as a program: the checks of some meshes under the process's environment

def run_mesh(pkg, name, symmetric):
    out = {}
    fs = context(pkg, name)
    for check in (lambda: check_vector_steps(fs), lambda: check_gathered_updates(fs) if symmetric else {},
                  lambda: check_product(fs, symmetric), lambda: check_gating(fs, symmetric),
                  lambda: assert_chain_is_the_solve(fs, lambda k: chain_classic(fs, k, symmetric), "classic", (2, 9))):
        out.update({"%s: %s" % (name, k): v for k, v in check().items()})
    out["%s: grid" % name] = float(fs.krylov_grid())
    fs.close()
    return out


def main(argv):
    import os

    from tests.helpers.product import ensure_built, pkg

    ensure_built()
    symmetric = os.environ.get("FEMSHELL_SYMMETRIC", "1") != "0"
    out = {}
    for name in argv[2:]:
        out.update(run_mesh(pkg, name, symmetric))
    np.savez(argv[1], **out)
    print("%d checks, largest share of a bound %.3f" % (len(out), max(v for k, v in out.items() if not k.endswith("grid"))))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
