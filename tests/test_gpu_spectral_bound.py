"""The spectral bound lambda of every smoothed multigrid level -- a power iteration of 30 steps from a hash vector, times 1.1
(csrc/amg_hierarchy.cpp power_iteration_start / _finish, on one rank and on a row-partitioned level) -- against lambda_max(D^-1 A) itself.
It sets the Chebyshev interval and the damping 4 / (3 lambda) of every prolongator; every restatement test takes the device's
value as an input and cannot see a wrong one.

lambda_true: the largest eigenvalue of the pencil (A, D), A from export_bsr / amg_export, D its diagonal blocks, by dense LAPACK
(tests/helpers/jacobi_truth.py true_lambda; proven on the CPU in tests/test_jacobi_truth_cpu.py).

(1) lambda_true <= lambda_device <= 1.1 lambda_true: a condition.  Below lambda_true the smoother amplifies the top of the
    spectrum; above 1.1 lambda_true the estimate would have overshot, which a power iteration -- it approaches from below -- cannot.
(2) lambda_device = 1.1 x the same iteration restated in numpy from the same hash vector with the exported inverse, to
    max(1e-12, 100 x |restated in double - restated in long double| / lambda): two evaluations that differ in summation order.
(3) FEMSHELL_AMG_LAMBDA_SAFETY and FEMSHELL_AMG_POWER_ITS do what they say.

First run on an MI355X (profiles/block_jacobi_and_spectral_bound.txt): no bug.  lambda_device / lambda_true lies between 1.0541
(20 x 20 cylinder) and 1.0996 (the Delaunay patch, whose level 0 smooths with 157 clusters of rigidly coupled nodes: the pencil
is taken over the clusters there); the distance to the restated iteration is at most 2.1e-16; both ranks of the row partition
report the same bits, 1.0788 and 1.0684 of the truth on the two partitioned levels."""
import numpy as np
import pytest

from tests.helpers import jacobi_truth as jt
from tests.helpers.product import ensure_built, pkg

pytestmark = pytest.mark.gpu

KNOBS = ("FEMSHELL_AMG_LAMBDA_SAFETY", "FEMSHELL_AMG_POWER_ITS", "FEMSHELL_AMG_SYMBOLIC", "FEMSHELL_AMG_DEVICE_MIN")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _context(name):
    ensure_built()
    ctx = jt.spectral_context(pkg, name)
    ctx.block_jacobi_export(0)  # (builds the hierarchy)
    return ctx


def smoothed_levels(ctx):
    """[(level, lambda_device)] of the levels that have a smoother: all but the coarsest"""
    lv = ctx.amg_levels()
    assert len(lv) >= 2
    return [(l, lv[l]["lambda_max"]) for l in range(len(lv) - 1)]


def check_condition(tag, lam_device, lam_true, safety=1.1):
    ratio = lam_device / lam_true
    print("%s: lambda_device %.12f lambda_true %.12f ratio %.4f" % (tag, lam_device, lam_true, ratio))
    # (a converged estimate gives safety x (1 +- a few eps): four eps of room on the upper side, as for the safety factor below)
    assert 1.0 <= ratio <= safety * (1.0 + 4.0 * jt.EPS), (tag, lam_device, lam_true, ratio)
    return ratio


def check_restated(ctx, tag, level, lam_device, safety=1.1, iterations=30):
    r, c, v = jt.level_operator(ctx, level)
    B = ctx.block_jacobi_export(level)
    e64 = float(jt.restated_lambda(r, c, v, B, iterations, np.float64))
    eld = float(jt.restated_lambda(r, c, v, B, iterations, jt.LD))
    tol = max(1e-12, 100.0 * abs(e64 - eld) / eld)
    dist = abs(lam_device / safety - eld) / eld
    print("%s: device / %.1f = %.15f restated %.15f distance %.1e (double against long double %.1e, tolerance %.1e)"
          % (tag, safety, lam_device / safety, eld, dist, abs(e64 - eld) / eld, tol))
    assert dist <= tol, (tag, dist, tol)
    return dist


@pytest.mark.parametrize("name", jt.SPECTRAL_MESHES)
def test_lambda_of_every_level_against_the_pencil(name):
    ctx = _context(name)
    patches = ctx.amg_patch_info()
    print("%s: levels %s, clusters on level 0: %d" % (name, [l["n_nodes"] for l in ctx.amg_levels()], patches["clusters"]))
    # The Delaunay patch has nodes close enough for clusters of rigidly coupled nodes (49 of its 1783 pairs above sigma 0.98): its
    # level 0 smooths with one block per cluster (csrc/amg_patch.hpp) and iterates on THAT operator, so D of the pencil is the
    # diagonal of K over the clusters.  The cluster blocks' inverses are not exported and agree with numpy's to about 1e-8
    # (tests/test_gpu_cycle.py), so (2), a statement to 1e-12 about the exported inverse, has no counterpart on that level.
    assert (patches["clusters"] > 0) == (name == "delaunay") and patches["not_positive_definite"] == 0
    for level, lam in smoothed_levels(ctx):
        tag = "%s level %d" % (name, level)
        clustered = level == 0 and patches["clusters"] > 0
        labels = ctx.amg_export(0)["patch_labels"] if clustered else None
        check_condition(tag + (" (clusters)" if clustered else ""), lam, jt.true_lambda(*jt.level_operator(ctx, level), labels=labels))
        # (every context here keeps the caller's numbering: the rows of level 0 lie in HBM in the order export_bsr hands out)
        if not clustered:
            check_restated(ctx, tag, level, lam)
    ctx.close()


def test_lambda_with_the_patterns_built_on_the_host(monkeypatch):
    """FEMSHELL_AMG_SYMBOLIC=host (the default builds the patterns in HBM), with every coarsening step on the device
    (FEMSHELL_AMG_DEVICE_MIN=100: level 0's power iteration then runs on the second stream beside the step's host work): the same
    conditions, and the same bits of lambda -- the two settings produce the same operators bit for bit (tests/test_gpu_amg.py)."""
    name = "curved"
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    ctx = _context(name)
    default = smoothed_levels(ctx)
    ctx.close()
    monkeypatch.setenv("FEMSHELL_AMG_SYMBOLIC", "host")
    ctx = _context(name)
    host = smoothed_levels(ctx)
    for level, lam in host:
        tag = "%s (host patterns) level %d" % (name, level)
        check_condition(tag, lam, jt.true_lambda(*jt.level_operator(ctx, level)))
        check_restated(ctx, tag, level, lam)
    ctx.close()
    assert host == default


def test_safety_factor_and_iteration_count_do_what_they_say(monkeypatch):
    name = "strip"
    ctx = _context(name)
    default = smoothed_levels(ctx)
    true0 = jt.true_lambda(*jt.level_operator(ctx, 0))
    ctx.close()
    # the reported value is the safety factor times the estimate: level 0's estimate does not depend on the factor (the coarse
    # operators do, through the damping of the prolongator: their estimates are held to the restated iteration instead)
    monkeypatch.setenv("FEMSHELL_AMG_LAMBDA_SAFETY", "1.3")
    ctx = _context(name)
    wide = smoothed_levels(ctx)
    assert abs(wide[0][1] / (default[0][1] * (1.3 / 1.1)) - 1.0) <= 4.0 * jt.EPS, (wide[0][1], default[0][1])
    for level, lam in wide:
        check_restated(ctx, "%s safety 1.3 level %d" % (name, level), level, lam, safety=1.3)
        check_condition("%s safety 1.3 level %d" % (name, level), lam, jt.true_lambda(*jt.level_operator(ctx, level)), safety=1.3)
    ctx.close()
    monkeypatch.delenv("FEMSHELL_AMG_LAMBDA_SAFETY")
    monkeypatch.setenv("FEMSHELL_AMG_POWER_ITS", "60")
    ctx = _context(name)
    for level, lam in smoothed_levels(ctx):
        tag = "%s 60 steps level %d" % (name, level)
        check_condition(tag, lam, true0 if level == 0 else jt.true_lambda(*jt.level_operator(ctx, level)))
        check_restated(ctx, tag, level, lam, iterations=60)
    ctx.close()


def test_row_partitioned_levels_report_one_lambda_that_meets_the_condition(tmp_path):
    """Two ranks, the panel of tests/helpers/multirank_worker.py (2337 nodes), FEMSHELL_AMG_DIST_MIN=100: levels 0 and 1 are
    row-partitioned and their bound comes from the same power iteration, halo exchanges and all-reduce included.  Every rank reports the same bits; condition (1) against
    the ranks' rows stacked.  Level 0 has 14,022 dofs, beyond a dense eigh in a test: true_lambda_sparse (the same reduced
    pencil, Lanczos to convergence; equal to the dense value to 1e-13 where both can run, tests/test_jacobi_truth_cpu.py)."""
    from tests.test_multirank_gpu import run_ranks, stacked_k_rows, stacked_level_rows

    env = {"FEMSHELL_AMG_DIST_MIN": "100", "FEMSHELL_TEST_AMG_EXPORT": "1", "FEMSHELL_TEST_EXPORT": "1"}
    ranks = sorted(run_ranks(2, "panel", tmp_path, pc="amg", extra_env=env), key=lambda q: int(q["begin"]))
    lam = np.asarray(ranks[0]["amg_lambda"])
    for r in ranks[1:]:
        assert np.asarray(r["amg_lambda"]).tobytes() == lam.tobytes()
    d = int(ranks[0]["amg_partitioned_levels"])
    assert d == 2
    for level in range(d):
        rp, ci, va = stacked_k_rows(ranks) if level == 0 else stacked_level_rows(ranks, level, "A")
        n = len(rp) - 1
        assert n == int(ranks[0]["amg_n_nodes"][level])
        true = jt.true_lambda(rp, ci, va) if 6 * n <= 3600 else jt.true_lambda_sparse(rp, ci, va)
        check_condition("two ranks, panel, level %d (%d nodes)" % (level, n), float(lam[level]), true)
