"""Structural dynamics without a GPU: the pins of the tests' own reference (tests/helpers/dynamics.py) against closed-form
results, the declaration of the new entry points, and the command lines of the host programs.

The pins run on sections.curved_patch(12, 10) with the oracle's K, nu 0.3, E 2.1e5, t 0.04, rho 7.8e-3."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import dynamics, oracle, sections
from tests.helpers.product import ROOT, ensure_built

NU, E, T, RHO = 0.3, 2.1e5, 0.04, 7.8e-3
N = 20

NEW_NAMES = ["femshell_set_density", "femshell_lumped_mass", "femshell_dynamics_defaults", "femshell_dynamics_begin",
             "femshell_dynamics_step", "femshell_dynamics_accept", "femshell_dynamics_state", "femshell_dynamics_energy",
             "femshell_dynamics_end"]


@pytest.fixture(scope="module")
def patch():
    m = sections.curved_patch(12, 10)
    mat = oracle.material(NU, E, T)
    mass = dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T)
    return m, mat, mass


def test_translational_mass_adds_up_to_rho_t_area(patch):
    m, _, mass = patch
    at, aq = dynamics.element_areas(m.xyz, m.tri, m.quad)
    total = RHO * T * (at.sum() + aq.sum())
    for d in range(3):
        assert abs(mass[:, d].sum() - total) <= 1e-14 * total
    np.testing.assert_array_equal(mass[:, 0], mass[:, 1])
    np.testing.assert_array_equal(mass[:, 3], mass[:, 5])
    assert abs(mass[:, 3].sum() - total * T * T / 12.0) <= 1e-14 * total * T * T / 12.0
    assert (mass > 0.0).all()


def test_quadrilateral_area_is_half_the_cross_product_of_the_diagonals():
    xyz = np.array([[0.0, 0, 0], [2, 0, 0], [2, 1, 0], [0, 1, 0]])
    mass = dynamics.lumped_mass(xyz, None, np.array([[0, 1, 2, 3]]), 3.0, 0.5)
    np.testing.assert_allclose(mass[:, 0], 3.0 * 0.5 * 2.0 / 4.0, rtol=1e-15)
    np.testing.assert_allclose(mass[:, 4], 3.0 * 0.5 ** 3 / 12.0 * 2.0 / 4.0, rtol=1e-15)


def test_free_fall_is_half_g_t_squared(patch):
    """unconstrained mesh, F = m g on the translations: u = g t^2 / 2 on every node, rotations 0 (average acceleration is exact
    for a constant acceleration; K u = 0 for a rigid translation)"""
    m, mat, mass = patch
    K = dynamics.to_matrix(oracle.assemble(m.xyz, m.tri, m.quad, mat, None, None))
    g = np.array([0.3, -0.2, 9.81])
    F = np.zeros((m.n_nodes, 6))
    F[:, :3] = mass[:, :3] * g
    dt = 1e-3
    nm = dynamics.Newmark(K, mass, None, dt)
    nm.begin(F.ravel())
    worst = 0.0
    scale = np.abs(0.5 * g * (N * dt) ** 2).max()  # max |g t^2 / 2| over the history, as the GPU test measures it
    for n in range(1, N + 1):
        u, v, a = nm.step(F.ravel())
        want = np.zeros((m.n_nodes, 6))
        want[:, :3] = 0.5 * g * (n * dt) ** 2
        worst = max(worst, np.abs(u.reshape(-1, 6) - want).max() / scale)
    print("free fall: worst deviation %.2e of max |g t^2 / 2|" % worst)
    assert worst <= 1e-11


def test_undamped_free_vibration_conserves_energy(patch):
    """from the static deflection with the load removed, dt = T1 / 20: the average-acceleration scheme conserves v.Mv/2 + u.Ku/2"""
    m, mat, mass = patch
    dmask = m.dirichlet_mask()
    r, c, v, F = oracle.assemble(m.xyz, m.tri, m.quad, mat, dmask, m.loads)
    K = dynamics.to_matrix((r, c, v))
    u0 = oracle.direct_solve(r, c, v, F)
    T1 = dynamics.first_period(K, mass, dmask)
    nm = dynamics.Newmark(K, mass, dmask, T1 / 20.0)
    zero = np.zeros(6 * m.n_nodes)
    nm.begin(zero, u0=u0)
    E0 = sum(dynamics.energy(K, mass, nm.u, nm.v))
    drift = 0.0
    for _ in range(N):
        u, vel, _ = nm.step(zero)
        drift = max(drift, abs(sum(dynamics.energy(K, mass, u, vel)) - E0) / E0)
    print("free vibration: T1 %.4e, energy drift %.2e" % (T1, drift))
    assert E0 > 0.0 and drift <= 1e-11


# ------------------------------------------------------------------ the feature, as far as it shows without a GPU

def test_new_entry_points_are_declared_exported_and_bound():
    pkg = ensure_built()
    with open(os.path.join(ROOT, "include", "femshell.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(pkg.library_path())
    from importlib import import_module

    binding = import_module("fem-shell_amd.binding")
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/femshell.h"
        assert hasattr(lib, name), name + " is not exported by libfemshell.so"
        assert name in binding.SYMBOLS, name + " is missing from binding.SYMBOLS"
    assert re.search(r"typedef struct femshell_dynamics_options\s*\{\s*double dt, beta, gamma, alpha;\s*\}", header)
    assert "#define FEMSHELL_VERSION 2" in header
    for method in ("set_density", "lumped_mass", "dynamics_begin", "dynamics_step", "dynamics_accept", "dynamics_state",
                   "dynamics_energy", "dynamics_end"):
        assert callable(getattr(pkg.FemShell, method, None)), method


HOST = os.path.join(ROOT, "fem-shell_amd", "host")


@pytest.fixture(scope="module")
def twins():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")


@pytest.mark.parametrize("program", [0, 1])
@pytest.mark.parametrize("args,option", [(["-rho", "-1"], "-rho"), (["-steps", "5"], "-dt"), (["-rho", "1", "-dt", "0", "-steps", "5"], "-dt")])
def test_twins_refuse_bad_dynamics_options_before_any_device_is_touched(twins, tmp_path, program, args, option):
    """-rho <= 0, -steps without -dt, -dt <= 0: refused in read_parameters with a message that names the option, exit
    status non-zero, on a machine without a GPU (no device is hidden here: the refusal comes before the first HIP call, and
    HIP_VISIBLE_DEVICES=-1 makes sure a machine with one behaves alike)"""
    base = ["-nu", "0.3", "-e", "1e4", "-t", "0.25", "-mesh", os.path.join(ROOT, "tests", "golden", "meshes", "test_E_uvw_t.xda"),
            "-out", str(tmp_path / "out")]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([twins[program]] + base + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=env, cwd=str(tmp_path), timeout=60)
    text = r.stdout + r.stderr
    assert r.returncode != 0, text
    assert option in text, text
    assert "HIP" not in text and "device" not in text.lower(), text
