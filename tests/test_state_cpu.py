"""CPU tests of the table that says which derived products of a context every kind of change makes stale (csrc/derived.hpp,
DESIGN section 8e): femshell_stale_after gives the table restated below, the closure rules hold for every row, and no source
file beside csrc/api_state.cpp writes the flags behind it or drops the multigrid hierarchy.  No GPU call is made."""
import glob
import os
import re

import pytest

from tests.helpers.product import ROOT, ensure_built

pkg = ensure_built()

CSRC = os.path.join(ROOT, "fem-shell_amd", "csrc")
WITH_K = {"K", "F", "Jacobi", "Hierarchy"}
TABLE = {
    "mesh": {"K", "F", "Jacobi", "Hierarchy", "Mass", "Ubar", "Solution", "WarmStart", "Fp64Only"},
    "dirichlet": {"K", "F", "Jacobi", "Hierarchy", "Ubar"},
    "sections": {"K", "F", "Jacobi", "Hierarchy", "Mass"},
    "sections_cleared_none_set": {"Mass"},
    "loads": {"F"},
    "prescribed": {"F", "Ubar"},
    "density": {"Mass"},
    "pc_options": {"Hierarchy", "Fp64Only"},
    "assembled": {"Jacobi", "Hierarchy"},
    "matrix_shifted": {"Jacobi", "Hierarchy"},
    "dynamics_begin": {"Jacobi", "Hierarchy", "WarmStart"},
    "matrix_spoiled": {"K", "F", "Jacobi", "Hierarchy"},
    "dynamics_end": {"K", "F", "Jacobi", "Hierarchy", "WarmStart"},
    "fp64_fallback": {"Hierarchy"},
    "krylov_probe": {"Solution"},
}
# the flags only api_state.cpp may assign to (have_solution: but for the one place where a solve produces it, below)
FLAGS = ["matrix_valid", "rhs_valid", "jacobi_valid", "mass_valid", "ubar_valid", "have_solution", "amg_fp64_only"]


def csrc_files():
    files = sorted(f for ext in ("cpp", "hip", "hpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) >= 40 and os.path.join(CSRC, "api_state.cpp") in files
    return files


def code_of(path):
    """The file without its // comments (a comment may speak of a flag being set)."""
    return "\n".join(line.split("//")[0] for line in open(path))


def test_the_names_are_those_of_the_table():
    assert pkg.STATE_CHANGES == list(TABLE)
    assert set(pkg.DERIVED_PRODUCTS) == TABLE["mesh"] and len(pkg.DERIVED_PRODUCTS) == 9


@pytest.mark.parametrize("change", list(TABLE))
def test_stale_after_is_the_restated_table(change):
    assert pkg.stale_after(change) == TABLE[change]
    assert pkg.stale_after(pkg.STATE_CHANGES.index(change)) == TABLE[change]


@pytest.mark.parametrize("change", list(TABLE))
def test_whatever_is_computed_from_k_is_stale_when_k_is(change):
    stale = pkg.stale_after(change)
    if "K" in stale:
        assert WITH_K <= stale
    if change == "mesh":
        assert stale == frozenset(pkg.DERIVED_PRODUCTS)


def test_there_is_no_change_beyond_the_table():
    for number in (-1, len(TABLE), len(TABLE) + 1, 1 << 20):
        with pytest.raises(pkg.FemShellError):
            pkg.stale_after(number)


def test_only_api_state_writes_the_flags():
    """An assignment is the flag's name followed by a single `=` (so `a = b = false` counts for both, `==` does not).  The one
    exception: solve_system (api.cpp) says that a solution exists, where it has produced one."""
    pattern = re.compile(r"\b(%s)\s*=(?!=)" % "|".join(FLAGS))
    seen_in_api_state = set()
    produced = []
    for f in csrc_files():
        name = os.path.basename(f)
        for lineno, line in enumerate(code_of(f).split("\n"), 1):
            for flag in pattern.findall(line):
                if name == "api_state.cpp":
                    seen_in_api_state.add(flag)
                elif name == "context.hpp" and re.search(r"\bbool\b", line):
                    pass  # the declarations with their initial values
                elif name == "api.cpp" and line.strip() == "c->have_solution = true;":
                    produced.append(lineno)
                else:
                    raise AssertionError("%s:%d assigns to %s" % (os.path.relpath(f, ROOT), lineno, flag))
    assert seen_in_api_state == set(FLAGS), "the scan no longer finds the writers in api_state.cpp?"
    assert len(produced) == 1


def test_only_api_state_drops_the_hierarchy():
    pattern = re.compile(r"\bamg\s*\.\s*reset\s*\(\s*\)")
    for f in csrc_files():
        found = pattern.search(code_of(f))
        if os.path.basename(f) == "api_state.cpp":
            assert found, "the scan no longer finds amg.reset() in api_state.cpp?"
        else:
            assert not found, os.path.relpath(f, ROOT)


def test_prepare_system_is_gone():
    for f in csrc_files():
        assert "prepare_system" not in open(f).read(), os.path.relpath(f, ROOT)
