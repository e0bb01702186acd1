"""The multigrid hierarchy a single-rank context built, held level by level to the restatement oracle/amg_oracle.py.

compare() restates the setup from the context's own K, spectral bounds and clusters, and holds aggregates, prolongators and
level operators to it.  It also works out which coarsening steps ran their numerics on the device (csrc/amg_hierarchy.cpp: level 0
whenever it is coarsened above coarsest_nodes or has clusters, the coarser levels by SetupRules::device_step) and checks that
the library accounts for exactly those.  What it returns says what the comparison exercised, so that a case can show that it
reached the kernel path it is there for."""
import os

import numpy as np
import scipy.sparse as sp

from oracle import amg_oracle

DIRECT_NODES = 200        # csrc/amg_device.hpp kDirectNodes
QR_REGISTER_NODES = 42    # csrc/amg_kernels.hip: larger aggregates take k_amg_tentative_qr<true> (rows in memory)
GALERKIN_PASS = 16        # coarse columns per pass of k_amg_galerkin_mfma
QR_DROP = 1e-8            # the tentative QR drops a column at nj <= 1e-8 n0
P_TOL, A_TOL = 1e-11, 1e-10


def bsr(rowptr, cols, vals, nc):
    n = len(rowptr) - 1
    return sp.bsr_matrix((vals, cols, rowptr), shape=(6 * n, 6 * nc))


def _atol(name, default):
    """getenv + atol as the library reads its knobs (unset: default; not a number: 0)."""
    e = os.environ.get(name)
    if e is None:
        return default
    digits = e.strip()
    k = 1 if digits[:1] in "+-" else 0
    while k < len(digits) and digits[k].isdigit():
        k += 1
    return int(digits[:k]) if k > (1 if digits[:1] in "+-" else 0) else 0


def device_steps(sizes, coarsest_nodes, max_levels=12, clusters=False):
    """One flag per coarsening step: were its numerics computed on the device?"""
    if os.environ.get("FEMSHELL_AMG_SETUP") == "host":
        return [False] * (len(sizes) - 1)
    device_min = _atol("FEMSHELL_AMG_DEVICE_MIN", 5000)
    out = []
    for l, n in enumerate(sizes[:-1]):
        if l == 0:
            on = max_levels > 1 and (n > coarsest_nodes or (clusters and n > DIRECT_NODES))
        else:  # (only a level whose operator a device step left in HBM)
            on = out[-1] and n > max(device_min, coarsest_nodes) and l + 2 < max_levels
        out.append(bool(on))
    return out


def coarse_symmetric(n):
    """csrc/amg_hierarchy.cpp coarse_symmetric_storage: a coarse operator stored as diagonal + upper blocks."""
    return 0 < _atol("FEMSHELL_AMG_COARSE_SYM", 100000) <= n and _atol("FEMSHELL_SYMMETRIC", 1) != 0


def stored_widths(A):
    """Blocks per stored row of a coarse operator, as the Galerkin kernels walk it."""
    A = A.tobsr((6, 6))
    A.sort_indices()
    n = A.shape[0] // 6
    if not coarse_symmetric(n):
        return np.diff(A.indptr)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    return np.bincount(rows[A.indices >= rows], minlength=n)


def mfma_flops_issued(P, Ac):
    """What k_amg_galerkin_mfma issues for one step (csrc/amg_device_setup.cpp): per coarse row, tiles of 16 x 16 over its stored
    blocks in passes of 16, two k-steps of 16x16x4 per fine row that reaches it.  P, Ac: the step's prolongator and (full) coarse
    operator, their structural patterns."""
    P = P.tobsr((6, 6))
    reach = np.bincount(P.indices, minlength=P.shape[1] // 6)
    total = 0.0
    for I, cnt in enumerate(stored_widths(Ac)):
        tiles = sum((6 * min(GALERKIN_PASS, cnt - g0) + 15) // 16 for g0 in range(0, cnt, GALERKIN_PASS))
        total += 2048.0 * 2.0 * tiles * reach[I]
    return total


def _per_level(tol, n):
    """a bound, or a list of them whose last entry holds for every deeper level"""
    tol = list(tol) if np.ndim(tol) else [tol]
    return tol + [tol[-1]] * max(0, n - len(tol))


def _rel(X, Y):
    d = abs(X - Y)
    return (d.max() if d.nnz else 0.0) / abs(Y).max()


def compare(fs, xyz, dmask, tri=None, quad=None, coarsest_nodes=1400, max_levels=12, p_tol=P_TOL, a_tol=A_TOL):
    """fs: a single-rank context after a multigrid solve, set up with these coarsest_nodes / max_levels; the mesh it was given.
    p_tol, a_tol: bounds of max|P - P_ref| / max|P_ref| and the same for the level operators (a number, or a list per level whose
    last entry holds for the deeper levels).
    Returns (levels of the restatement, dict of what the comparison exercised)."""
    lv = fs.amg_levels()
    sizes = [l["n_nodes"] for l in lv]
    assert len(lv) >= 2 and sizes[0] == len(xyz), sizes
    rg, cg, vg, _ = fs.export_bsr()
    A = bsr(rg, cg, vg, sizes[0])
    ex = [fs.amg_export(li) for li in range(len(lv))]
    labels = ex[0]["patch_labels"]
    # (FEMSHELL_AMG_PLAIN_RBM=1: the six plain rigid-body modes, no projection onto the tangent planes)
    plain = _atol("FEMSHELL_AMG_PLAIN_RBM", 0) != 0
    levels = amg_oracle.setup(A, xyz, dmask, lams=[l["lambda_max"] for l in lv], coarsest_nodes=coarsest_nodes,
                              max_levels=max_levels, tri=None if plain else tri, quad=None if plain else quad, patch_labels=labels)
    assert [L.n for L in levels] == sizes, ([L.n for L in levels], sizes)
    steps = device_steps(sizes, coarsest_nodes, max_levels, labels is not None)
    tol_p, tol_a = _per_level(p_tol, len(sizes)), _per_level(a_tol, len(sizes))
    got = {"sizes": sizes, "device": steps, "p_err": [], "a_err": [], "zero_columns": [], "stored_width": [],
           "aggregate_nodes": [], "qr_closest": [], "clusters": 0 if labels is None else int(labels.max()) + 1}
    for li, L in enumerate(levels):
        e = ex[li]
        if e["A_vals"] is not None:
            Al = bsr(e["A_rowptr"], e["A_cols"], e["A_vals"], sizes[li])
            got["a_err"].append(_rel(Al, L.A))
        else:  # (only the coarsest level may go without its host copy)
            assert li == len(levels) - 1, "level %d: no host copy of the operator" % li
            got["a_err"].append(None)
        if li == len(levels) - 1:
            break
        np.testing.assert_array_equal(e["agg"], L.agg, err_msg="level %d" % li)
        P = bsr(e["P_rowptr"], e["P_cols"], e["P_vals"], sizes[li + 1])
        got["p_err"].append(_rel(P, L.P))
        # the library's bound is a bound: 1.1 x its power iteration against an independent estimate
        lam = lv[li]["lambda_max"]
        assert 0.9 * lam <= 1.1 * amg_oracle.lambda_max(L.A, L.Dm, 60) <= 1.25 * lam, li
        # no column of the tentative QR may sit near its drop threshold: the case would flip on rounding
        ratios = []
        amg_oracle.tentative(L.agg, sizes[li + 1], L.B, ratios)
        r = np.asarray(ratios)
        near = r[(r > 0.1 * QR_DROP) & (r < 10.0 * QR_DROP)]
        assert len(near) == 0, ("level %d: tentative QR columns within 10x of the drop" % li, near)
        got["qr_closest"].append(float(np.min(np.abs(np.log10(r[r > 0] / QR_DROP)))) if np.any(r > 0) else np.inf)
        # dependent columns: a zero column of P, a unit diagonal entry of the coarse operator
        colmax = abs(L.P.tocsc()).max(axis=0).toarray().ravel()
        zero = np.flatnonzero(colmax == 0.0)
        if len(zero):
            Pcol = abs(P.tocsc()).max(axis=0).toarray().ravel()
            assert np.all(Pcol[zero] == 0.0), li
            if ex[li + 1]["A_vals"] is not None:
                Ac = bsr(ex[li + 1]["A_rowptr"], ex[li + 1]["A_cols"], ex[li + 1]["A_vals"], sizes[li + 1])
                np.testing.assert_array_equal(Ac.diagonal()[zero], 1.0)
        got["zero_columns"].append(len(zero))
        got["aggregate_nodes"].append(np.bincount(L.agg, minlength=sizes[li + 1]))
        got["stored_width"].append(int(stored_widths(levels[li + 1].A).max()))
    print("hierarchy %s device %s: P %s A %s" % (sizes, steps, " ".join("%.1e" % v for v in got["p_err"]),
                                                  " ".join("-" if v is None else "%.1e" % v for v in got["a_err"])))
    for li, v in enumerate(got["p_err"]):
        assert v <= tol_p[li], ("P of level %d" % li, v, tol_p[li])
    for li, v in enumerate(got["a_err"]):
        assert v is None or v <= tol_a[li], ("A of level %d" % li, v, tol_a[li])
    info = fs.amg_symbolic_info()
    assert sum(info.values()) == sum(steps), (info, steps)
    if steps[0]:  # (the statistics describe the step of level 0)
        st = fs.amg_setup_stats()
        mfma = os.environ.get("FEMSHELL_AMG_GALERKIN") == "mfma"
        assert st["galerkin_on_matrix_cores"] == mfma
        if mfma:  # the work the matrix cores were given follows the stored rows of the coarse operator the library chose
            e1 = ex[1]
            A1 = bsr(e1["A_rowptr"], e1["A_cols"], e1["A_vals"], sizes[1])
            P0 = bsr(ex[0]["P_rowptr"], ex[0]["P_cols"], ex[0]["P_vals"], sizes[1])
            got["mfma_flops_issued"] = st["galerkin_mfma_flops_issued"]
            assert got["mfma_flops_issued"] == mfma_flops_issued(P0, A1), (got["mfma_flops_issued"], mfma_flops_issued(P0, A1))
    return levels, got
