"""Linear buckling on the device (femshell_buckling, FemShell.buckling, FEM-shell -buckling) against the dense pencil of
tests/helpers/buckling.py, the reference tests/test_buckling_cpu.py pins.

The bounds.  With rho_j <= tol some eigenvalue mu lies within rho_j |mu_j| of mu_j, so |lambda_j - lambda| <= rho / (1 - rho) |lambda_j|:
a factor of 2 covers that, another factor of 2 the inner solves at tol / 100: 4 tol |lambda_j|.  The K-sine between x_j and the
span of the reference cluster is at most (residual in the K^-1 norm) / gap = rho_j |mu_j| / gap_j, with the same factor 4."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import buckling as bk, prescribed as pr, resultants as rs
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

TOL = 1e-8
N_MODES, GUARD = 3, 3
INVALID, UNSUPPORTED, BREAKDOWN = -1, -7, -5

_cases = {}


def case(name):
    """the problem and its dense reference: computed once, shared by the tests, left unchanged"""
    if name not in _cases:
        _cases[name] = bk.CASES[name]()
        _cases[name].reference(TOL)
    return _cases[name]


def context(c, pc):
    fs = pkg.FemShell(*c.material)
    fs.set_mesh(c.xyz, c.tri, c.quad)
    if c.sec is not None:
        fs.set_sections(*c.sec)
    fs.set_dirichlet(c.mask)
    if c.loads is not None:
        fs.set_loads(c.loads)
    if pc == "amg":
        fs.set_preconditioner("amg", coarsest_nodes=20)  # more than one level on meshes of 48 and 81 nodes
    else:
        fs.set_preconditioner("jacobi")
    return fs


def run(c, fs):
    """the call the tests look at: the prestress of the context's own solve where the case has loads (the NULL form), else the
    given field"""
    if c.loads is not None:
        u, info = fs.solve(rtol=1e-12, max_it=50000)
        assert info["converged"] == 1
        return fs.buckling(n_modes=N_MODES, guard=GUARD, tol=TOL), u
    return fs.buckling(n_modes=N_MODES, guard=GUARD, tol=TOL, u=c.u), None


@pytest.mark.parametrize("pc", ["jacobi", "amg"])
@pytest.mark.parametrize("name", list(bk.CASES))
def test_factors_and_shapes_against_the_dense_pencil(name, pc):
    c = case(name)
    mu, V, free, Kf = c.reference(TOL)
    lam_ref = bk.factors(mu, N_MODES)
    fs = context(c, pc)
    (lam, modes, info), u = run(c, fs)
    print("buckling %-15s %-6s lambda %s  iterations %d, inner %d, rho_max %.2e, %.2f s (solves %.2f)"
          % (name, pc, lam, info["iterations"], info["inner_iterations"], info["rho_max"], info["seconds_total"], info["seconds_solves"]))
    assert info["converged"] == N_MODES and info["block"] == N_MODES + GUARD and info["rho_max"] <= TOL
    assert (info["rho"] <= TOL).all() and info["rho_max"] == info["rho"].max()
    # eigenvalues, signed and in the order of the definition
    for j in range(N_MODES):
        assert abs(lam[j] - lam_ref[j]) <= 4.0 * TOL * abs(lam[j]), (j, lam, lam_ref)
    assert (np.diff(np.abs(lam)) >= -4.0 * TOL * np.abs(lam[1:])).all()
    if name == "shear_plate":  # +- pairs: the positive member first
        assert lam[0] > 0.0 > lam[1] and lam[2] > 0.0 and abs(lam[0] + lam[1]) <= 4.0 * TOL * lam[0]
    if name == "sections_panel":
        assert (lam_ref < 0.0).any() and (lam_ref > 0.0).any()  # a mixed-sign spectrum
    # shapes
    groups = bk.clusters(mu)
    for j in range(N_MODES):
        group = bk.cluster_of(j, groups)
        gap = bk.cluster_gap(mu, group)
        x = modes[j].ravel()
        assert not x[pr.fixed_dofs(c.mask)].any()
        sine = bk.subspace_distance(x[free], V[:, group], Kf)
        print("    mode %d: K-sine to the reference cluster %s = %.2e, bound %.2e" % (j, group, sine, 4.0 * TOL * abs(mu[j]) / gap))
        assert sine <= 4.0 * TOL * abs(mu[j]) / gap
        # scaling and sign: the translational entry of largest magnitude is +1, the lowest index on ties
        tr = modes[j][:, :3].ravel()
        big = int(np.argmax(np.abs(tr)))
        assert tr[big] == 1.0 and np.abs(tr).max() == 1.0
    # two calls give the same bits
    (lam2, modes2, info2), _ = run(c, fs)
    np.testing.assert_array_equal(lam, lam2)
    np.testing.assert_array_equal(modes, modes2)
    np.testing.assert_array_equal(info["rho"], info2["rho"])
    assert info["iterations"] == info2["iterations"] and info["inner_iterations"] == info2["inner_iterations"]
    if u is not None:  # the NULL form is the explicit one
        lam3, modes3, _ = fs.buckling(n_modes=N_MODES, guard=GUARD, tol=TOL, u=u)
        np.testing.assert_array_equal(lam, lam3)
        np.testing.assert_array_equal(modes, modes3)
    fs.close()


@pytest.mark.parametrize("pc", ["jacobi", "amg"])
def test_the_context_is_as_it_was(pc):
    """get_solution before and after are bitwise equal; a solve after buckling gives the bits of a fresh context's solve; a pending
    initial guess stays pending"""
    c = case("flat_panel")
    fs, fresh = context(c, pc), context(c, pc)
    u, _ = fs.solve(rtol=1e-12, max_it=50000)
    F = fs.export_bsr()
    hist = fs.residual_history()
    lam, _, info = fs.buckling(n_modes=N_MODES, guard=GUARD, tol=TOL)
    assert info["converged"] == N_MODES
    np.testing.assert_array_equal(fs.get_solution(), u)
    np.testing.assert_array_equal(fs.residual_history(), hist)
    for x, y in zip(fs.export_bsr(), F):
        np.testing.assert_array_equal(x, y)
    u1, i1 = fs.solve(rtol=1e-12, max_it=50000)
    u2, i2 = fresh.solve(rtol=1e-12, max_it=50000)
    assert i1["converged"] == 1 and i1["iterations"] == i2["iterations"]
    np.testing.assert_array_equal(u1, u2)
    np.testing.assert_array_equal(u1, u)
    for key in ("refine_passes_done", "refine_correction_rel", "refine_residual_reduction"):
        assert i1[key] == i2[key], key
    # a warm start that was pending stays pending: the next solve is the warm one
    fs.set_initial_guess(None)
    fresh.set_initial_guess(None)
    fs.buckling(n_modes=N_MODES, guard=GUARD, tol=TOL)
    u1, i1 = fs.solve(rtol=1e-12, max_it=50000)
    u2, i2 = fresh.solve(rtol=1e-12, max_it=50000)
    assert i1["iterations"] == i2["iterations"]
    np.testing.assert_array_equal(u1, u2)
    fs.close()
    fresh.close()


def test_buckling_before_any_assembly_builds_what_it_needs():
    """a mesh, a Dirichlet set and an explicit u are enough"""
    c = case("shear_plate")
    fs = context(c, "jacobi")
    lam, _, info = fs.buckling(n_modes=2, guard=2, tol=1e-6, u=c.u, want_modes=False)
    ref = bk.factors(c.reference(TOL)[0], 2)
    assert info["converged"] == 2 and (np.abs(lam - ref) <= 4e-6 * np.abs(lam)).all()
    fs.close()


def test_refusals_leave_a_usable_context():
    c = case("flat_panel")
    fs = pkg.FemShell(*c.material)
    with pytest.raises(pkg.FemShellError) as e:  # no mesh
        fs.buckling()
    assert e.value.code == INVALID and "no mesh" in str(e.value)
    fs.close()
    fs = context(c, "jacobi")
    with pytest.raises(pkg.FemShellError) as e:  # the NULL form before any solve
        fs.buckling(n_modes=N_MODES, guard=GUARD)
    assert e.value.code == INVALID and "no solve" in str(e.value)
    bad = c.u.copy()
    bad[5, 0] = np.inf
    with pytest.raises(pkg.FemShellError) as e:
        fs.buckling(n_modes=N_MODES, guard=GUARD, u=bad)
    assert e.value.code == INVALID and "non-finite" in str(e.value)
    for kw, word in (({"n_modes": 0}, "n_modes"), ({"guard": -1}, "guard"), ({"n_modes": 20, "guard": 13}, "32"),
                     ({"tol": 0.0}, "tol"), ({"tol": -1e-8}, "tol"), ({"max_it": 0}, "max_it"), ({"inner_rtol": -1.0}, "inner_rtol")):
        args = dict(n_modes=N_MODES, guard=GUARD, tol=TOL, u=c.u)
        args.update(kw)
        with pytest.raises(pkg.FemShellError) as e:
            fs.buckling(**args)
        assert e.value.code == INVALID and word in str(e.value), kw
    # fewer than 2 (n_modes + guard) free translational dofs
    tight = np.full(c.n, 0x07, np.uint8)
    tight[:3] = 0x00
    fs.set_dirichlet(tight)  # 9 free translational dofs
    with pytest.raises(pkg.FemShellError) as e:
        fs.buckling(n_modes=3, guard=2, u=c.u)
    assert e.value.code == INVALID and "free translational" in str(e.value)
    fs.set_dirichlet(c.mask)
    # dynamics active
    fs.set_density(7.8e-3)
    fs.dynamics_begin(1e-3)
    with pytest.raises(pkg.FemShellError) as e:
        fs.buckling(n_modes=N_MODES, guard=GUARD, u=c.u)
    assert e.value.code == INVALID and "dynamics" in str(e.value)
    fs.dynamics_end()
    # no prestress at all
    with pytest.raises(pkg.FemShellError) as e:
        fs.buckling(n_modes=N_MODES, guard=GUARD, u=np.zeros((c.n, 6)))
    assert e.value.code == BREAKDOWN and "no prestress" in str(e.value)
    # the context is usable: the factors of the reference
    lam, _, info = fs.buckling(n_modes=N_MODES, guard=GUARD, tol=TOL, u=c.u)
    ref = bk.factors(c.reference(TOL)[0], N_MODES)
    assert info["converged"] == N_MODES and (np.abs(lam - ref) <= 4.0 * TOL * np.abs(lam)).all()
    fs.close()
    # a row-partitioned context
    part = pkg.FemShell(*c.material, rank=0, world_size=2)
    with pytest.raises(pkg.FemShellError) as e:
        part.buckling(u=np.zeros(0))
    assert e.value.code == UNSUPPORTED and "single-rank" in str(e.value)


def test_reaching_max_it_returns_the_best_pairs():
    c = case("flat_panel")
    fs = context(c, "jacobi")
    lam, _, info = fs.buckling(n_modes=N_MODES, guard=GUARD, tol=TOL, max_it=2, u=c.u)
    assert info["iterations"] == 2 and info["converged"] < N_MODES and info["rho_max"] > TOL
    assert np.isfinite(lam).all() and (np.diff(np.abs(lam)) >= 0.0).all() and info["rho_max"] == info["rho"].max()
    # (a Ritz value of the pencil never lies below the lowest factor in magnitude)
    assert abs(lam[0]) >= abs(bk.factors(c.reference(TOL)[0], 1)[0]) * (1.0 - 1e-6)
    fs.close()


# ------------------------------------------------------------------ the host program

HOST = os.path.join(ROOT, "fem-shell_amd", "host")


def _cantilever_panel():
    """the flat jittered 7 x 5 panel, clamped on x = 0 (boundary id 1: all six), a uniaxial edge load on x = LX"""
    c = case("flat_panel")
    mask = np.zeros(c.n, np.uint8)
    clamped = pr.edge_nodes(c.xyz, 0, 0.0)
    mask[clamped] = 0x3F
    return c.xyz, c.tri, clamped, mask, c.loads


def _write_panel(tmp_path):
    xyz, tri, clamped, _, loads = _cantilever_panel()
    lines = ["$MeshFormat", "2.2 0 8", "$EndMeshFormat", "$Nodes", str(len(xyz))]
    lines += ["%d %r %r %r" % (n + 1, float(x), float(y), float(z)) for n, (x, y, z) in enumerate(xyz)]
    lines += ["$EndNodes", "$Elements", str(len(tri) + len(clamped))]
    k = 1
    for t in tri:
        lines.append("%d 2 2 5 5 %d %d %d" % (k, t[0] + 1, t[1] + 1, t[2] + 1))
        k += 1
    for n in clamped:  # point elements: a boundary id on the node
        lines.append("%d 15 2 1 0 %d" % (k, n + 1))
        k += 1
    lines += ["$EndElements", ""]
    msh = tmp_path / "panel.msh"
    msh.write_text("\n".join(lines))
    with open(str(tmp_path / "panel_f"), "w") as f:
        f.write("%d 1.0\n" % len(xyz))
        for row in loads:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    return str(msh)


def _point_vectors(vtk_path, name, n_nodes):
    lines = open(vtk_path).read().splitlines()
    at = lines.index("VECTORS %s double" % name)
    return np.array([[float(t) for t in l.split()] for l in lines[at + 1:at + 1 + n_nodes]])


def test_fem_shell_writes_the_factors_the_binding_gives(tmp_path):
    """FEM-shell -buckling 2 after its static solve: the same library, the same calls (multigrid by default, guard 4, tol 1e-8)"""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    msh = _write_panel(tmp_path)
    xyz, tri, _, mask, loads = _cantilever_panel()
    out = str(tmp_path / "P")
    r = subprocess.run([os.path.join(HOST, "FEM-shell"), "-nu", repr(rs.NU), "-e", repr(rs.E), "-t", repr(rs.T), "-mesh", msh, "-out", out,
                        "-buckling", "2", "-reactions"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "Linear buckling: 2 of 2 pairs converged" in r.stdout
    text = open(out + "_buckling.txt").read().splitlines()
    assert text[0].startswith("#") and not text[-1].startswith("#")
    got = np.loadtxt(out + "_buckling.txt")
    assert got.shape == (2, 3) and list(got[:, 0]) == [1, 2]
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.set_preconditioner("amg")
    _, sinfo = fs.solve(rtol=1e-12, max_it=5000)
    lam, modes, info = fs.buckling(n_modes=2)
    fs.close()
    assert sinfo["converged"] == 1 and info["converged"] == 2 and lam[0] > 0.0
    # '%.15e': sixteen significant digits
    assert (np.abs(got[:, 1] - lam) <= 1e-15 * np.abs(lam)).all()
    assert (np.abs(got[:, 2] - info["rho"]) <= 1e-15 * np.abs(info["rho"])).all()
    for k in range(2):
        np.testing.assert_array_equal(_point_vectors(out + ".vtk", "buckling_%d_u" % (k + 1), len(xyz)), modes[k][:, :3])
        np.testing.assert_array_equal(_point_vectors(out + ".vtk", "buckling_%d_r" % (k + 1), len(xyz)), modes[k][:, 3:])
    assert len(_point_vectors(out + ".vtk", "reaction_f", len(xyz))) == len(xyz)  # the reactions' arrays are still there
