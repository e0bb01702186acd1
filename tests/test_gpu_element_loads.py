"""Element loads on the device (femshell_set_element_loads, femshell_element_load_vector, FemShell.set_element_loads) against
tests/helpers/element_loads.py, the longdouble reference tests/test_element_loads_cpu.py pins, and the invariant the library keeps:
the loads in force are nodal + S in every consumer (F, the right-hand side of prescribed values, reactions, Newmark)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import element_loads as el, oracle, prescribed as pr, resultants as rs
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

TINY = 1e-12
RHO = 7.8e-3


def _counts(tri, quad):
    return (0 if tri is None else len(tri)), (0 if quad is None else len(quad))


def _context(xyz, tri, quad, sec=None):
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    fs.set_mesh(xyz, tri, quad)
    if sec is not None:
        fs.set_sections(sec[0], sec[1], sec[2])
    return fs


def _mask(n):
    mask = np.zeros(n, np.uint8)
    mask[::3] = 0x15
    mask[0] = 0x3F
    return mask


def _expected_F(mask, loads):
    return np.where(pr.fixed_dofs(mask), 0.0, np.asarray(loads, dtype=np.float64).ravel())


# ------------------------------------------------------------------ 1. device against reference

@pytest.mark.parametrize("name", list(rs.device_meshes()))
def test_load_vector_matches_the_reference(name, monkeypatch):
    """Seeded random (p, q) per element: |S - S_ref| <= 1e-12 T_a per row and component, T_a = sum over the row's elements of
    (|p| + ||q||_1) |d1| |d2|.  The cross products and the list-order sum of at most 765 terms cost at most about (n_e + 8) eps T_a,
    under 1e-13 T_a.  The rotational columns are exactly zero, two calls give the same bits, one kind alone leaves the other
    unloaded, a Dirichlet set does not show, clearing returns zeros."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nt, nq = _counts(tri, quad)
    fs = _context(xyz, tri, quad, sec)
    assert not fs.element_load_vector().any()  # none set yet
    tl, ql = el.random_loads(nt, nq)
    fs.set_element_loads(tl, ql)
    S = fs.element_load_vector()
    assert S.shape == (len(xyz), 6)
    S_ref, T = el.load_vector(xyz, tri, quad, tl, ql)
    ratio = el.bound_ratio(S, S_ref, T)
    print("element_loads_vs_reference %-28s elements %5d  max |S - S_ref| / (1e-12 T_a) = %.3e" % (name, nt + nq, ratio))
    assert ratio <= 1.0
    assert np.abs(S[:, :3]).max() > 0.0 and not S[:, 3:].any()
    assert np.array_equal(S, fs.element_load_vector())
    fs.set_dirichlet(_mask(len(xyz)))
    assert np.array_equal(S, fs.element_load_vector())
    if nt and nq:  # one kind alone
        fs.set_element_loads(tl, None)
        assert el.bound_ratio(fs.element_load_vector(), el.load_vector(xyz, tri, quad, tl, None)[0], T) <= 1.0
        fs.set_element_loads(None, ql)
        assert el.bound_ratio(fs.element_load_vector(), el.load_vector(xyz, tri, quad, None, ql)[0], T) <= 1.0
    fs.set_element_loads(None, None)
    assert not fs.element_load_vector().any()
    fs.set_element_loads(tl, ql)
    assert np.array_equal(S, fs.element_load_vector())
    fs.close()


def test_wrong_lengths_are_refused_by_the_binding():
    xyz, tri, quad = rs.device_meshes()["mixed_petals24"]()[:3]
    fs = _context(xyz, tri, quad)
    with pytest.raises(ValueError):
        fs.set_element_loads(np.zeros((len(tri) + 1, 4)), None)
    with pytest.raises(ValueError):
        fs.set_element_loads(None, np.zeros((len(quad) - 1, 4)))
    fs.close()


# ------------------------------------------------------------------ 2. the invariant: loads in force = nodal + S

@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24", "coil300", "delaunay600_rcm", "panel_three_sections"])
def test_right_hand_side_is_nodal_plus_element_loads(name, monkeypatch):
    """With nodal loads L and element loads set, in either order, F at the free dofs is fl(L + S) with S as element_load_vector
    returns it, zero at the fixed ones; a second set of element loads replaces the first, a second set of nodal loads keeps the
    element loads, clearing leaves L."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = len(xyz)
    nt, nq = _counts(tri, quad)
    mask = _mask(n)
    rng = np.random.default_rng(23)
    L1, L2 = rng.uniform(-50.0, 50.0, (n, 6)), rng.uniform(-50.0, 50.0, (n, 6))
    a, b = el.random_loads(nt, nq, seed=3), el.random_loads(nt, nq, seed=4)

    def F_of(fs):
        return fs.export_bsr()[3]

    for order in ("nodal_first", "element_first"):
        fs = _context(xyz, tri, quad, sec)
        fs.set_dirichlet(mask)
        if order == "nodal_first":
            fs.set_loads(L1)
            fs.set_element_loads(*a)
        else:
            fs.set_element_loads(*a)
            fs.set_loads(L1)
        fs.assemble()  # F by the assembly kernel
        Sa = fs.element_load_vector()
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L1 + Sa), err_msg=order)
        fs.set_element_loads(*b)  # F by k_rhs alone from here on
        Sb = fs.element_load_vector()
        assert not np.array_equal(Sa, Sb)
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L1 + Sb), err_msg=order)
        fs.set_loads(L2)
        np.testing.assert_array_equal(fs.element_load_vector(), Sb)
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L2 + Sb), err_msg=order)
        fs.set_element_loads(None, None)
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L2), err_msg=order)
        fs.set_element_loads(*a)
        np.testing.assert_array_equal(fs.element_load_vector(), Sa)
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L2 + Sa), err_msg=order)
        fs.close()


# ------------------------------------------------------------------ 3. end to end

def _clamped_panel():
    xyz, tri = pr.panel(lift=True)
    mask = np.zeros(len(xyz), np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    tl, _ = el.random_loads(len(tri), 0, seed=9)
    tl[:, 0] += 300.0  # a pressure with a mean
    return xyz, tri, mask, tl


def _pair(mask, prepare=None):
    """two contexts of the lifted panel under the same Dirichlet set (block-Jacobi), `prepare` applied to each"""
    xyz, tri = pr.panel(lift=True)
    out = []
    for _ in range(2):
        fs = _context(xyz, tri, None)
        fs.set_dirichlet(mask)
        fs.set_preconditioner("jacobi")
        if prepare:
            prepare(fs)
        out.append(fs)
    return out


def test_static_solve_equals_the_solve_under_the_load_vector():
    """set_element_loads against set_loads(element_load_vector()): F and the block-Jacobi solution are equal as numbers, and the
    reactions' force columns sum to minus the total applied force to the bound of tests/test_gpu_prescribed.py"""
    xyz, tri, mask, tl = _clamped_panel()
    fa, fb = _pair(mask)
    fa.set_element_loads(tl)
    S = fa.element_load_vector()
    fb.set_loads(S)
    ua, ia = fa.solve(rtol=1e-12, max_it=50000)
    ub, ib = fb.solve(rtol=1e-12, max_it=50000)
    assert ia["converged"] == 1 and ia["iterations"] == ib["iterations"]
    np.testing.assert_array_equal(fa.export_bsr()[3], fb.export_bsr()[3])
    np.testing.assert_array_equal(fa.export_bsr()[3], _expected_F(mask, S))
    np.testing.assert_array_equal(ua, ub)
    assert np.abs(ua).max() > 0.0
    r = fa.reactions()
    np.testing.assert_array_equal(r, fb.reactions())
    K_unc, _ = pr.matrices(xyz, tri, None, oracle.material(rs.NU, rs.E, rs.T), mask)
    scale = pr.row_scale(K_unc, ua)
    balance = np.abs(r[:, :3].sum(axis=0) + S[:, :3].sum(axis=0)).max()
    print("reactions under element loads: force balance / (1e-12 sum S_a) = %.2e, total applied force %s" % (balance / (TINY * scale.sum()), S[:, :3].sum(axis=0)))
    assert balance <= TINY * scale.sum()
    assert np.abs(S[:, :3].sum(axis=0)).max() > 1.0
    fa.close()
    fb.close()


def test_newmark_step_with_element_loads_set_while_dynamics_is_active():
    """F of the next step: one Newmark step from rest, the loads set after dynamics_begin, gives the state of set_loads(S)"""
    xyz, tri, mask, tl = _clamped_panel()
    fa, fb = _pair(mask, prepare=lambda fs: fs.set_density(RHO))
    for fs in (fa, fb):
        fs.dynamics_begin(1e-3)
    fa.set_element_loads(tl)
    S = fa.element_load_vector()
    fb.set_loads(S)
    for fs in (fa, fb):
        assert fs.dynamics_step(rtol=1e-12, max_it=50000)["converged"] == 1
    sa, sb = fa.dynamics_state(candidate=True), fb.dynamics_state(candidate=True)
    assert np.abs(sa[0]).max() > 0.0
    for x, y in zip(sa, sb):
        np.testing.assert_array_equal(x, y)
    # a second set while active, the step recomputed from the same committed state
    fa.set_element_loads(2.0 * tl)
    fb.set_loads(fa.element_load_vector())
    for fs in (fa, fb):
        assert fs.dynamics_step(rtol=1e-12, max_it=50000)["converged"] == 1
    for x, y in zip(fa.dynamics_state(candidate=True), fb.dynamics_state(candidate=True)):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(fa.dynamics_state(candidate=True)[0], sa[0])
    for fs in (fa, fb):
        fs.dynamics_end()
        fs.close()


def test_prescribed_values_with_element_loads():
    """F = mask(nodal + S - K_unc u_bar): the right-hand side and the solution of set_loads(S)"""
    xyz, tri, mask, tl = _clamped_panel()
    tip = pr.edge_nodes(xyz, 0, pr.LX)
    mask = mask.copy()
    mask[tip] = 0x04
    ubar = np.zeros((len(xyz), 6))
    ubar[tip, 2] = 0.01
    fa, fb = _pair(mask, prepare=lambda fs: fs.set_prescribed(ubar))
    fa.set_element_loads(tl)
    S = fa.element_load_vector()
    fb.set_loads(S)
    ua, ia = fa.solve(rtol=1e-12, max_it=50000)
    ub, ib = fb.solve(rtol=1e-12, max_it=50000)
    assert ia["converged"] == 1 and ia["iterations"] == ib["iterations"]
    Fa = fa.export_bsr()[3]
    np.testing.assert_array_equal(Fa, fb.export_bsr()[3])
    assert not np.array_equal(Fa, _expected_F(mask, S))  # u_bar shows
    np.testing.assert_array_equal(ua, ub)
    assert np.array_equal(ua[tip, 2], np.full(len(tip), 0.01))
    np.testing.assert_array_equal(fa.reactions(), fb.reactions())
    fa.close()
    fb.close()


# ------------------------------------------------------------------ 4. refusals

def test_refusals_leave_the_context_usable_and_the_loads_in_force():
    xyz, tri, mask, tl = _clamped_panel()
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    # no mesh: through the binding (clearing needs no arrays) and with arrays, straight at the C entry point
    with pytest.raises(pkg.FemShellError) as info:
        fs.set_element_loads(None, None)
    assert info.value.code == -1
    rc = fs._L.femshell_set_element_loads(fs._h, tl.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None)
    assert rc == -1 and b"femshell_set_mesh first" in fs._L.femshell_last_error()
    with pytest.raises(pkg.FemShellError):
        fs.element_load_vector()
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(mask)
    L = np.random.default_rng(2).uniform(-1.0, 1.0, (len(xyz), 6))
    fs.set_loads(L)
    fs.set_element_loads(tl)
    S = fs.element_load_vector()
    fs.assemble()
    F = fs.export_bsr()[3]
    for bad_value in (np.nan, np.inf):
        bad = tl.copy()
        bad[len(bad) // 2, 2] = bad_value
        with pytest.raises(pkg.FemShellError) as info:
            fs.set_element_loads(bad)
        assert info.value.code == -1
        np.testing.assert_array_equal(fs.element_load_vector(), S)
        np.testing.assert_array_equal(fs.export_bsr()[3], F)
    # set_sections and set_density do not touch them
    fs.set_sections([[0.3, 2e5, 0.05], [0.25, 7e4, 0.1]], np.arange(len(tri)) % 2, None)
    fs.set_density(RHO)
    np.testing.assert_array_equal(fs.element_load_vector(), S)
    fs.assemble()
    np.testing.assert_array_equal(fs.export_bsr()[3], F)
    # set_mesh forgets them (and the nodal loads)
    fs.set_mesh(xyz, tri)
    assert not fs.element_load_vector().any()
    fs.set_dirichlet(mask)
    fs.set_loads(L)
    fs.assemble()
    np.testing.assert_array_equal(fs.export_bsr()[3], _expected_F(mask, L))
    fs.close()


# ------------------------------------------------------------------ 5. the timing hook

@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24", "coil300"])
def test_time_kernel_reports_the_bytes_of_the_model(name):
    """per listed element 16 + 4 + 32 bytes, 24 per node, 96 per owned row; the loads in force are not disturbed"""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    assert not env
    nt, nq = _counts(tri, quad)
    fs = _context(xyz, tri, quad)
    ms, by = fs.time_kernel(pkg.KERNEL_ELEMENT_LOADS, reps=3)  # a mesh is all it needs
    assert ms > 0.0
    n = len(xyz)
    assert by == el.model_bytes(el.listed_elements(n, tri, quad), n, n)
    mask = _mask(n)
    fs.set_dirichlet(mask)
    L = np.random.default_rng(2).uniform(-1.0, 1.0, (n, 6))
    fs.set_loads(L)
    fs.set_element_loads(*el.random_loads(nt, nq))
    S = fs.element_load_vector()
    fs.assemble()
    F = fs.export_bsr()[3]
    ms, by2 = fs.time_kernel(pkg.KERNEL_ELEMENT_LOADS, reps=3)
    assert ms > 0.0 and by2 == by
    np.testing.assert_array_equal(fs.element_load_vector(), S)
    np.testing.assert_array_equal(fs.export_bsr()[3], F)
    np.testing.assert_array_equal(F, _expected_F(mask, L + S))
    fs.close()


# ------------------------------------------------------------------ 6. slice walk and ranks (child processes)

WORKER = os.path.join(ROOT, "tests", "helpers", "element_loads_worker.py")
FAKE_DIR = os.path.join(ROOT, "tests", "helpers", "fake_rccl")
CHILD_TIMEOUT = 240


def run_ranks(world, tmp_path, tag, extra_env=None):
    """the launch pattern of tests/test_gpu_dynamics.py on the element-loads worker"""
    subprocess.check_call(["make", "-C", FAKE_DIR, "-s"])
    env = dict(os.environ, FEMSHELL_RCCL_LIB=os.path.join(FAKE_DIR, "libfake_rccl.so"))
    env.pop("FEMSHELL_SLICE_GRID", None)
    env.update(extra_env or {})
    uid = str(tmp_path / ("uid_%s.npy" % tag))
    outs = [str(tmp_path / ("out_%s_%d.npz" % (tag, r))) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), uid, outs[r]], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(out.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, "\n".join("--- rank %d\n%s" % (q, logs[q][-1500:]) for q in range(world)))
    return [dict(np.load(o)) for o in outs]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One child per grid setting, then the two ranks, one after another; the first child that does not exit 0 ends the module
    (nothing more is started on the GPU behind a child that failed)."""
    tmp = tmp_path_factory.mktemp("element_loads")
    got = {}
    for grid in ("default", "8", "24"):
        got[grid] = run_ranks(1, tmp, "grid" + grid, {} if grid == "default" else {"FEMSHELL_SLICE_GRID": grid})[0]
    got["ranks"] = run_ranks(2, tmp, "ranks")
    return got


def _reference_of_the_worker():
    from tests.helpers.element_loads_worker import problem
    xyz, tri, tl, mask, nodal = problem()
    S_ref, T = el.load_vector(xyz, tri, None, tl, None)
    return mask, nodal, S_ref, T


def test_more_slices_than_workgroups_give_the_bits_of_the_default_grid(runs):
    mask, nodal, S_ref, T = _reference_of_the_worker()
    base = runs["default"]
    assert int(base["slices"]) == 40 and len(base["S"]) == 1271 and int(base["same"]) == 1
    assert el.bound_ratio(base["S"], S_ref, T) <= 1.0
    np.testing.assert_array_equal(base["F"], _expected_F(mask, nodal + base["S"]))
    for grid in ("8", "24"):
        run = runs[grid]
        assert (int(run["slices"]) + 7) // 8 > int(grid) // 8  # a workgroup took a second slice
        assert int(run["same"]) == 1
        np.testing.assert_array_equal(run["S"], base["S"], err_msg="grid " + grid)
        np.testing.assert_array_equal(run["F"], base["F"], err_msg="grid " + grid)


def test_two_ranks_on_one_gpu_gather_the_load_vector_of_the_single_rank_run(runs):
    """both ranks return the same gathered S; it agrees with the single-rank S to 1e-13 T_a (a rank sums a row over its own list,
    whose order may differ from the single rank's); every rank's rows of F are fl(nodal + S) of its own S"""
    mask, nodal, S_ref, T = _reference_of_the_worker()
    single, ranks = runs["default"], runs["ranks"]
    ranks = sorted(ranks, key=lambda q: int(q["begin"]))
    assert int(ranks[0]["begin"]) == 0 and int(ranks[0]["end"]) == int(ranks[1]["begin"]) and int(ranks[1]["end"]) == len(single["S"])
    assert 0 < int(ranks[0]["end"]) < len(single["S"])
    np.testing.assert_array_equal(ranks[0]["S"], ranks[1]["S"])
    ratio = el.bound_ratio(ranks[0]["S"], single["S"], T, tol=1e-13)
    print("two ranks: max |S - S_single| / (1e-13 T_a) = %.3e" % ratio)
    assert ratio <= 1.0
    assert el.bound_ratio(ranks[0]["S"], S_ref, T) <= 1.0
    want = _expected_F(mask, nodal + ranks[0]["S"])
    for r in ranks:
        assert int(r["same"]) == 1
        np.testing.assert_array_equal(r["F"], want[6 * int(r["begin"]):6 * int(r["end"])])
