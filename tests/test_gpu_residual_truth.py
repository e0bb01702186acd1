"""The double-double residual (femshell_residual: k_residual_dd_sym, k_residual_dd) against an exact truth, row by row, and the two
numbers the solver derives from it.

The kernels are the measuring instrument of the project: the refinement passes and the solve from an initial guess take their
right-hand sides from them, femshell_solve_info::true_rel_residual and the error estimate behind the solver term of DESIGN
section 2 are their output, and tests/helpers/manufactured.py builds its right-hand sides with them.  Every older assertion on
them is ||r_dd - r_ext|| <= 1e-11 ||F|| against a long-double evaluation, mostly on inputs where nothing cancels: plain FP64 row
sums pass that (tests/test_residual_truth_cpu.py shows it), and so would a kernel that lost the error terms of one row, of the
transposed products, of the diagonal block or of the tail of a chunk.

Here every scalar row is held to

    |r_i - r*_i|  <=  u |r*_i| + gamma_m^2 (|F_i| + (|K||x|)_i),     m = 6 (blocks in row i) + 2,  u = 2^-53

r* the correctly rounded residual of the exported K and F (tests/helpers/residual_truth.py: error-free products, math.fsum), the
budget the bound of Dot2, the algorithm the kernels implement; derived, not measured.  States: "cancel" -- F set to the FP64
product K x, so that the exact residual is the rounding noise of that product, sixteen digits below the terms: the state that
tells double-double from double; "zero" -- F = 0; "free" -- K x of the size of F, the input of the older tests; and on a roof the
converged iterate of a solve without refinement, which is what a refinement pass sees.  tests/helpers/residual_cases.py lists
the shapes and the path each is there for.

Measured on an MI355X (profiles/residual_truth_vs_exact.txt, tools/residual_truth_report.py): the worst row uses 0.016 of its
budget in k_residual_dd_sym (the roof's iterate; 0.013 on coil300, 0.012 on the curved patch) and 0.008 in k_residual_dd (the
walking panel); rows without cancellation come out correctly rounded.  The numpy restatement of the arithmetic uses 0.004 to
0.07.  A build with the product error dropped in the in-list alone, or in the last block of a chunk of four alone, was 5e11 to
5e12 budgets out in the cancelling state of every case here.  true_rel_residual: 4e-16 from the exact value on one rank and
3e-16 on two, where 2.9e-12 and 6.2e-12 are allowed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import residual_cases as rc
from tests.helpers import residual_truth as rt
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu
pkg = ensure_built()

CHILD_TIMEOUT = 300


def held_to_the_budget(name, got):
    for state, g in got.items():
        print(rc.line(name, state, g))
    for state, g in got.items():
        over = np.flatnonzero(rt.ratios(g["r"], g["truth"], g["budget"]) > 1.0)
        assert len(over) == 0, "%s, state %s: %d rows over the budget, the first %s, the worst at %.3g" % (
            name, state, len(over), over[:8], g["ratio"])
    # the states are what they are meant to be: the residual of "cancel" is the rounding error of an FP64 product of at most
    # 1812 terms a row, gamma_1812 = 2e-13 of the terms at the very most; in the other two nothing cancels
    assert got["cancel"]["cancel"] < 1e-12 and got["zero"]["cancel"] > 0.1 and got["free"]["cancel"] > 0.1


@pytest.mark.parametrize("name", rc.SYMMETRIC_CASES)
def test_symmetric_storage_residual_within_the_budget_on_every_row(name):
    got, _ = rc.run_case(pkg, name)
    held_to_the_budget(name, got)


@pytest.mark.parametrize("name", rc.FULL_CASES)
def test_full_storage_residual_within_the_budget_on_every_row(name):
    got, _ = rc.run_case(pkg, name)
    held_to_the_budget(name, got)


def test_residual_within_the_budget_when_workgroups_walk_over_slices(tmp_path):
    """FEMSHELL_SLICE_GRID=8 on a matrix of 76 slices, both kernels, in a child process as tests/test_gpu_slice_walk.py runs its
    cases (the cap is read once per process): a workgroup takes ten slices, one after the other.  That test asks the later trips
    for the bits of the default grid; here every row of every trip is held to the budget in the cancelling state, where an
    accumulator or a staged x left over from the slice before is an error of the size of a term."""
    out = str(tmp_path / "walk.npz")
    env = dict(os.environ, FEMSHELL_SLICE_GRID="8")
    r = subprocess.run([sys.executable, "-m", "tests.helpers.residual_cases", out] + list(rc.WALK_CASES), cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:]
    got = dict(np.load(out))
    for name in rc.WALK_CASES:
        assert (int(got["S:" + name]) + 7) // 8 > 1  # more slices in an XCD group's eighth than block rows in the grid
        for state in rt.STATES:
            assert float(got["ratio:%s:%s" % (name, state)]) <= 1.0, (name, state, float(got["ratio:%s:%s" % (name, state)]))
        assert float(got["cancel:%s:cancel" % name]) < 1e-12


# ------------------------------------------------------------------ the converged iterate, and true_rel_residual

def roof():
    from tests.test_gpu_amg import _context, _make

    m, mat = _make("roof", 32)
    return _context(m, mat), m


def test_residual_of_a_converged_iterate_within_the_budget_on_every_row():
    """The thin roof, solved with the multigrid preconditioner and no refinement pass: ||K|| ||u|| is seven orders above ||F||,
    the residual of the iterate is what a refinement pass would take as its right-hand side."""
    fs, m = roof()
    fs.set_preconditioner("amg", refine_passes=0)
    u, info = fs.solve(rtol=1e-12, max_it=500)
    assert info["converged"] == 1
    r, c, v, F = fs.export_bsr()
    res = fs.residual(u)
    fs.close()
    K = (r, c, v)
    truth = rt.exact(K, F, u.ravel())
    budget = rt.bound(K, F, u.ravel(), truth)
    ratio = rt.ratios(res, truth, budget)
    cancel = rt.cancellation(truth, rt.scale(K, F, u.ravel()))
    print("roof32 iterate: ||r*|| / ||S|| %.1e, ||r*|| / ||F|| %.2e, worst error / budget %.4f"
          % (cancel, np.linalg.norm(truth) / np.linalg.norm(F), ratio.max()))
    assert ratio.max() <= 1.0, (np.flatnonzero(ratio > 1.0)[:8], ratio.max())


def test_true_rel_residual_is_the_exact_residual_of_the_returned_iterate():
    """One refinement pass, rtol 1e-12: the solve ends on the double-double residual of the accumulated iterate, and that norm is
    what femshell_solve_info reports (cg_amg: *true_rr_out).  Held to the exact residual of the returned u on the exported K and F."""
    fs, m = roof()
    fs.set_preconditioner("amg", refine_passes=1)
    u, info = fs.solve(rtol=1e-12, max_it=500)
    assert info["converged"] == 1
    r, c, v, F = fs.export_bsr()
    fs.close()
    want = np.linalg.norm(rt.exact((r, c, v), F, u.ravel())) / np.linalg.norm(F)
    rel = abs(info["true_rel_residual"] - want) / want
    print("roof32: true_rel_residual %.17e, exact %.17e, relative difference %.2e (allowed %.2e)"
          % (info["true_rel_residual"], want, rel, rt.norm_tolerance(len(F))))
    assert info["true_rel_residual"] > 0.0
    assert rel <= rt.norm_tolerance(len(F))
