"""Linear buckling as far as it shows without a GPU: the declaration of the new entry points and the command line of FEM-shell --
-buckling and -buckling_tol are read, and refused, with the command line, before a device is touched."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.helpers.product import ROOT, ensure_built

HOST = os.path.join(ROOT, "fem-shell_amd", "host")
NEW_NAMES = ["femshell_geometric_product", "femshell_buckling_defaults", "femshell_buckling"]


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
    assert re.search(r"FEMSHELL_KERNEL_GEOMETRIC_PRODUCT\s*=\s*14\b", header) and pkg.KERNEL_GEOMETRIC_PRODUCT == 14
    for method in ("geometric_product", "buckling"):
        assert callable(getattr(pkg.FemShell, method, None)), method
    # the structures the binding mirrors have the C layout: 4 int32 + 2 doubles; 4 int32, an int64 and 6 doubles
    assert ctypes.sizeof(binding.BucklingOptions) == 32 and ctypes.sizeof(binding.BucklingInfo) == 72
    assert re.search(r"typedef struct femshell_buckling_options\s*\{\s*int32_t n_modes, guard, max_it, reserved;\s*double tol, inner_rtol;\s*\}", header)
    L = pkg.load_library()
    for name in NEW_NAMES:
        assert getattr(L, name).argtypes is not None, name
    o = binding.BucklingOptions()
    assert L.femshell_buckling_defaults(ctypes.byref(o)) == 0
    assert (o.n_modes, o.guard, o.max_it, o.tol, o.inner_rtol) == (4, 4, 100, 1e-8, 0.0)
    assert L.femshell_buckling_defaults(None) == -1
    # the header comment begins, as its neighbours do, with what it extends
    at = header.index("linear buckling: load factors")
    assert "extends: the reference has no stability analysis" in header[at:at + 400]


@pytest.fixture(scope="module")
def fem_shell():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell")


BASE = ["-nu", "0.3", "-e", "1e4", "-t", "0.25", "-mesh", os.path.join(ROOT, "tests", "golden", "meshes", "test_E_uvw_t.xda")]
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.mark.parametrize("args,option", [
    (["-buckling", "0"], "-buckling"),                                        # N outside 1 .. 28 (guard 4, block <= 32)
    (["-buckling", "29"], "-buckling"),
    (["-buckling"], "-buckling"),                                             # no number at all
    (["-buckling", "3", "-rho", "1", "-modes", "4"], "-modes"),               # instead of the solve it follows
    (["-buckling", "3", "-rho", "1", "-dt", "0.1", "-steps", "5"], "-dt"),    # the time stepping options
    (["-buckling", "3", "-rho", "1", "-steps", "5"], "-steps"),
    (["-buckling", "3", "-buckling_tol", "0"], "-buckling_tol"),
    (["-buckling", "3", "-buckling_tol", "-1e-8"], "-buckling_tol"),
    (["-buckling_tol", "1e-8"], "-buckling"),                                 # the tolerance without -buckling
])
def test_fem_shell_refuses_bad_buckling_options_before_any_device_is_touched(fem_shell, tmp_path, args, option):
    """refused in read_parameters with a message that names the option, exit status non-zero, before the first HIP call"""
    r = subprocess.run([fem_shell] + BASE + ["-out", str(tmp_path / "out")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=dict(os.environ, **NO_DEVICE), cwd=str(tmp_path), timeout=60)
    text = r.stdout + r.stderr
    assert r.returncode != 0, text
    assert option in r.stderr and "FAILED" in r.stdout, text
    assert "n_elem()" not in r.stdout  # while the command line is read
    assert "HIP" not in text and "device" not in text.lower(), text


@pytest.mark.parametrize("extra", [[], ["-reactions", "-stress"], ["-pressure", "2.5"], ["-rho", "7.8e-9", "-gravity", "0", "0", "-9810"],
                                   ["-buckling_tol", "1e-6"]])
def test_fem_shell_accepts_buckling_with_the_options_of_the_static_solve(fem_shell, tmp_path, extra):
    """good flags are accepted up to the point where the program needs a GPU"""
    r = subprocess.run([fem_shell] + BASE + ["-out", str(tmp_path / "out"), "-buckling", "2"] + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, env=dict(os.environ, **NO_DEVICE), cwd=str(tmp_path), timeout=60)
    assert "Read command-line arguments.......OK" in r.stdout and "n_elem()=" in r.stdout, r.stdout + r.stderr
    assert "-buckling" not in r.stderr, r.stderr


def test_usage_names_the_option_and_the_precice_twin_does_not_take_it(fem_shell, tmp_path):
    r = subprocess.run([fem_shell, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, cwd=str(tmp_path),
                       timeout=60, env=dict(os.environ, **NO_DEVICE))
    assert "-buckling:" in r.stdout + r.stderr and "-buckling_tol:" in r.stdout + r.stderr
    twin = os.path.join(HOST, "FEM-shell-precice")
    r = subprocess.run([twin, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, cwd=str(tmp_path),
                       timeout=60, env=dict(os.environ, **NO_DEVICE))
    assert "-buckling" not in r.stdout + r.stderr
    r = subprocess.run([twin] + BASE + ["-config", str(tmp_path / "no-config.xml"), "-dt", "0.01", "-buckling", "2"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, cwd=str(tmp_path), timeout=60, env=dict(os.environ, **NO_DEVICE))
    assert r.returncode != 0 and "FAILED" in r.stdout
    assert "-buckling" in r.stderr
