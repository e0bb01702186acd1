"""Every per-slice kernel with more slices than workgroups.

The kernels that walk the sliced layout loop with SliceWalk (csrc/device_common.hpp): workgroup b belongs to XCD group b % 8 and
takes the slices b / 8, b / 8 + G / 8, ... of that group's eighth of the rows.  The grid G is 8 ceil(S / 8) up to the cap
FEMSHELL_SLICE_GRID (65536; FEMSHELL_ASM_GRID, 2048, for the two-phase assembly kernel), so below two million node rows no
workgroup ever takes a second slice -- and what the second trip through a loop body depends on (LDS reused behind barriers,
accumulators reset per slice, partial sums carried across slices, the `continue` of the node-pair kernels on an odd slice count,
walks through order[] on spans) never ran under test.  Here the caps are 8, 16 and 24: one, two and three block rows per XCD
group, on matrices of 1 to 79 slices -- uneven last rows, groups with no slice at all, pairs of slices with a dead half.

The caps are read once per process: tests/helpers/grid_worker.py runs the library's paths in a child process per setting and
measures every error against its reference there; its docstring lists what the npz holds.  Asserted here:
  * ratio:*  every error is within its bound -- the bounds the project already holds the default grid to;
  * bits:*   results formed row by row by one lane, whichever workgroup holds the slice, have the bits of the default grid;
  * close:*  results behind partial sums over workgroups (CG, the K cycle, Gram matrices), grouped differently now, agree with
             the default grid's to 1e-10 relative (the solver-term bound of tests/test_gpu_parity.py), iteration counts to +-3
             (block-Jacobi), +-5 (multigrid);
  * same:*   two runs in one process give the same bits, M(2r) = 2 M(r);
  * S:*      ceil(S / 8) > G / 8 for the cases meant to walk: a second step happened.
No setting here is below 8 or off a multiple of 8: what the library makes of such values is shown on the CPU alone
(tests/test_plan_cpu.py)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests.helpers.product import ROOT

pytestmark = pytest.mark.gpu

GRIDS = ("default", "8", "16", "24")
CHILD_TIMEOUT = 600


def run_worker(tmp_path_factory, name, env, which):
    out = str(tmp_path_factory.mktemp("grid_" + name) / "out.npz")
    e = dict(os.environ)
    for k in ("FEMSHELL_SLICE_GRID", "FEMSHELL_ASM_GRID", "FEMSHELL_ASM_PIPE_GRID", "FEMSHELL_ASM_PIPE", "FEMSHELL_SYMMETRIC"):
        e.pop(k, None)
    e.update(env)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "tests.helpers.grid_worker", out, which], cwd=ROOT, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout[-20000:])
    assert r.returncode == 0, "grid worker %s ended with %d:\n%s" % (name, r.returncode, r.stdout[-3000:])
    got = dict(np.load(out))
    ratios = {k: float(v) for k, v in got.items() if k.startswith("ratio:")}
    worst = max(ratios, key=ratios.get)
    print("[grid] setting %s: %.1f s, largest ratio to a bound %.3e (%s)" % (name, time.time() - t0, ratios[worst], worst))
    for letter in "abcde":
        part = {k: v for k, v in ratios.items() if k.startswith("ratio:%s:" % letter)}
        if part:
            k = max(part, key=part.get)
            print("[grid] setting %s section %s: largest ratio %.3e (%s)" % (name, letter, part[k], k))
    return got


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One child per setting, one after another; the first child that does not exit 0 ends the module (nothing more is started on
    the GPU behind a child that failed)."""
    got = {}
    for grid in GRIDS:
        env = {} if grid == "default" else {"FEMSHELL_SLICE_GRID": grid, "FEMSHELL_ASM_GRID": grid}
        got[grid] = run_worker(tmp_path_factory, grid, env, "abcde")
    got["two_phase_8"] = run_worker(tmp_path_factory, "two_phase_8", {"FEMSHELL_ASM_PIPE": "0", "FEMSHELL_ASM_GRID": "8"}, "b")
    return got


def keys(run, prefix):
    return sorted(k for k in run if k.startswith(prefix))


def walks(slices, grid):
    """the proof that a workgroup took a second slice: more slices in an XCD group's eighth than block rows in the grid"""
    return (int(slices) + 7) // 8 > int(grid) // 8


def test_the_worker_ran_every_case_under_every_setting(runs):
    base = set(runs["default"])
    # 14 contexts of section a with ten row-by-row results each, two of section b with K and F
    assert len(keys(runs["default"], "ratio:")) >= 120 and len(keys(runs["default"], "bits:")) == 144
    for grid in GRIDS[1:]:
        assert set(runs[grid]) == base, grid
    assert set(runs["two_phase_8"]) == {k for k in base if k.split(":")[1] == "b"}


@pytest.mark.parametrize("grid", GRIDS + ("two_phase_8",))
def test_every_error_is_within_the_bound_the_default_grid_is_held_to(runs, grid):
    run = runs[grid]
    for k in keys(run, "ratio:"):
        assert float(run[k]) <= 1.0, (grid, k, float(run[k]))
    for k in keys(run, "same:"):
        assert int(run[k]) == 1, (grid, k)
    for k in keys(run, "text:b:"):
        assert str(run[k]) == "k_assemble", (grid, k, str(run[k]))


@pytest.mark.parametrize("grid", GRIDS[1:])
def test_row_by_row_results_have_the_bits_of_the_default_grid(runs, grid):
    """spmv, spmm (1, 3, 4, 5 columns), residual, element_product, reactions, K and F: every row is summed by the same lane in
    the same order, whichever workgroup holds its slice."""
    for k in keys(runs["default"], "bits:"):
        np.testing.assert_array_equal(runs[grid][k], runs["default"][k], err_msg="%s under grid %s" % (k, grid))


def test_two_phase_assembly_with_eight_workgroups_has_the_bits_of_the_default_grid(runs):
    run = runs["two_phase_8"]
    assert len(keys(run, "bits:b:")) == 4
    for k in keys(run, "bits:b:"):
        np.testing.assert_array_equal(run[k], runs["default"][k], err_msg=k)
    for k in keys(run, "S:b:"):
        assert walks(run[k], 8), (k, int(run[k]))


@pytest.mark.parametrize("grid", GRIDS[1:])
def test_results_behind_partial_sums_agree_with_the_default_grid(runs, grid):
    """The solutions of block-Jacobi CG (both recurrences) and of the multigrid solve, Gram matrices: the partial sums of the
    workgroups are grouped differently, so the bits may differ -- by rounding: 1e-10 relative, the solver-term bound of
    tests/test_gpu_parity.py -- and the solves by a few iterations."""
    run, base = runs[grid], runs["default"]
    assert len(keys(base, "close:")) == 2 + 1 + 6
    for k in keys(base, "close:"):
        a, b = np.asarray(run[k], dtype=np.float64), np.asarray(base[k], dtype=np.float64)
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("[grid] %s under grid %s: %.2e from the default grid" % (k, grid, err))
        assert err <= 1e-10, (grid, k, err)
    for k in keys(base, "its:"):
        a, b = int(run[k]), int(base[k])
        if k.endswith("levels") or k.endswith("widest_restriction_row"):
            assert a == b, (grid, k, a, b)
        else:
            assert abs(a - b) <= (3 if k.startswith("its:c:") else 5), (grid, k, a, b)


def test_the_cases_meant_to_walk_did(runs):
    walking = {"8": (9, 15, 17, 76), "16": (17, 76), "24": (76,)}
    for grid in GRIDS[1:]:
        run = runs[grid]
        for slices in (1, 7, 8, 9, 15, 17, 76):
            for sym in "10":
                s = int(run["S:a:S%d:sym%s" % (slices, sym)])
                assert s == slices
                assert walks(s, grid) == (slices in walking[grid]), (grid, slices)
        for k in ("S:b:panel76", "S:b:mixed", "S:c:panel76", "S:e:gram", "S:e:newmark"):
            assert walks(run[k], grid), (grid, k, int(run[k]))
        for k in keys(run, "S:d:"):
            levels = [int(s) for s in run[k]]
            assert len(levels) >= 3 and walks(levels[0], grid), (grid, k, levels)
            if grid == "8" and "delaunay" not in k:  # level 1 of the 48 x 48 panel has about ten slices: its kernels walk too
                assert walks(levels[1], grid), (grid, k, levels)
        # the restriction-wider-than-the-LDS-panel case: k_spmv's panel loop inside a slice loop
        assert int(run["its:d:delaunay-morton-K:widest_restriction_row"]) > 64
    # modes: the small patch of the issue has 5 slices and cannot walk; the 24 x 18 patch does with one block row
    assert not walks(runs["8"]["S:e:modes-small-jacobi"], 8) and walks(runs["8"]["S:e:modes-curved-amg"], 8)


# ---- the row partition: interior and boundary spans, each capped at 8 workgroups, walking order[] ---------------------------------

def test_two_ranks_block_jacobi_under_a_grid_of_eight(tmp_path):
    """The single-reduction recurrence over interior and boundary spans.  Held to what tests/test_multirank_gpu.py holds the default
    grid to: every rank's rows of K and F against the oracle's assembly (1e-12, exact), iteration count and solution against the
    single-rank run of the default grid (+-3, 1e-8), the solution against the oracle's refined solve (1e-8); and the iteration
    count against the oracle's block-Jacobi CG within 5 -- the 2 that tests/test_gpu_parity.py allows between a single-rank solve
    and the oracle's, and the 3 between that solve and the ranks'."""
    from tests.helpers import oracle
    from tests.helpers.multirank_worker import build_problem
    from tests.test_multirank_gpu import run_ranks

    (tmp_path / "one").mkdir()
    single = run_ranks(1, "panel", tmp_path / "one")[0]
    ranks = run_ranks(2, "panel", tmp_path, extra_env={"FEMSHELL_SLICE_GRID": "8", "FEMSHELL_TEST_EXPORT": "1"})
    assert int(single["converged"]) == 1 and abs(int(ranks[0]["iterations"]) - int(single["iterations"])) <= 3
    assert np.linalg.norm(ranks[0]["u"] - single["u"]) < 1e-8 * np.linalg.norm(single["u"])
    m, mat = build_problem("panel")
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, oracle.material(*mat), m.dirichlet_mask(), m.loads)
    scale = np.abs(v0).max()
    covered = 0
    for r in sorted(ranks, key=lambda q: int(q["begin"])):
        b, e = int(r["begin"]), int(r["end"])
        assert b == covered and walks((e - b + 31) // 32, 8)
        covered = e
        lo, hi = int(r0[b]), int(r0[e])
        np.testing.assert_array_equal(r["k_cols"][:hi - lo], c0[lo:hi])
        assert np.abs(r["k_vals"][:hi - lo] - v0[lo:hi]).max() <= 1e-12 * scale
        np.testing.assert_array_equal(r["k_F"], F0[6 * b:6 * e])
        assert int(r["converged"]) == 1 and int(r["converged2"]) == 1
        assert int(r["iterations"]) == int(ranks[0]["iterations"])
        np.testing.assert_array_equal(r["u"], ranks[0]["u"])
        assert np.linalg.norm(r["u2"] - 2.0 * r["u"]) <= 1e-8 * np.linalg.norm(r["u2"])
        assert float(r["true_res"]) == float(ranks[0]["true_res"])
    assert covered == m.n_nodes
    _, info0 = oracle.pcg(r0, c0, v0, F0, rtol=1e-11, max_it=100000)
    assert info0["converged"] == 1 and abs(int(ranks[0]["iterations"]) - info0["iterations"]) <= 5, (int(ranks[0]["iterations"]), info0)
    u0 = oracle.refined_solve(r0, c0, v0, F0)
    err = np.linalg.norm(ranks[0]["u"].ravel() - u0) / np.linalg.norm(u0)
    print("[grid] two ranks, block-Jacobi, grid 8: %d iterations (oracle %d), %.2e from the refined solve"
          % (int(ranks[0]["iterations"]), info0["iterations"], err))
    assert err < 1e-8, err


def test_two_ranks_multigrid_with_split_levels_under_a_grid_of_eight(tmp_path):
    """FEMSHELL_AMG_DIST_MIN=100: levels 0 and 1 are split over the ranks.  The assertions of
    test_row_partitioned_hierarchy_follows_the_restatement, which holds the default grid to them."""
    from tests.test_multirank_gpu import check_hierarchy_against_the_restatement

    check_hierarchy_against_the_restatement(2, "panel", 100, tmp_path, extra_env={"FEMSHELL_SLICE_GRID": "8"})
