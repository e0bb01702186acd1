"""The derived element kernels and the quadrilateral assembly give the bits of a recorded parent commit.

tests/golden/derived_bits/parent_digests.json holds, per case, sha256 of `array + 0.0` (signed zeros folded) of what the
calls below return, computed on an MI355X at the commit the file names -- the last one before the element geometry
(QUAD4 frame, Gauss-point Jacobian, bilinear gradients, DKQ sides and shape derivatives, Specht's sums and mu, the
coordinate gather) and the slice row sum (row bits, ballots, position word, list-order walk) were folded into shared
functions.  The arithmetic of the following did not move, so every digest must be the parent's:

  panel  the warped 70 x 45 triangle panel of test_gpu_assembly_bits: full and partial slices, a last slice of fewer than
         32 nodes.  element_load_vector, geometric_product (1 and 3 columns), thermal_load_vector, element_resultants cold
         and with temperatures in force
  hub    the fan of 40 triangles on top of the 20 x 20 grid: the hub's row has 40 entries in a slice list of 87, which
         takes two 64-entry words.  The same calls as the panel
  hub96  the tiling case.  The 40-triangle fan leaves the densest slice list at 102 entries, short of the smallest tile
         (kGpTile = 128 of k_geometric_product), and a ring of 80 reaches 127; with the ring refined to 96 triangles the
         hub's slice list has 143 entries -- asserted from the plan on the CPU -- so a kernel with a tile of 128 walks it in
         two tiles and three 64-entry words.  The same calls.  (The panel's densest list, 130 entries, also passes 128.)
  quads  a warped 24 x 18 quadrilateral mesh with one row of triangles mixed in (kHasQuads kernels meet both kinds in one
         slice list): export_bsr values and F (the assembly digests of test_gpu_assembly_bits cover triangles only) and
         element_load_vector.  The resultants, thermal loads and geometric coefficients of quadrilaterals are NOT pinned:
         their frame and Jacobian take the floating-point mode of quad4_record now and may round differently in the last
         place; the truth tests hold them.

Inputs are random element loads, temperatures, displacements and columns from fixed seeds.
    python tests/test_gpu_derived_bits.py     prints the digests of this tree as JSON.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import meshes  # noqa: E402
from tests.helpers.product import ensure_built  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "derived_bits", "parent_digests.json")
TRI_CALLS = ("element_loads", "geometric_product_1", "geometric_product_3", "thermal_loads", "resultants", "resultants_thermal")
QUAD_CALLS = ("bsr_vals", "bsr_F", "element_loads")
CASES = ["%s-%s" % (mesh, call) for mesh, calls in (("panel", TRI_CALLS), ("hub", TRI_CALLS), ("hub96", TRI_CALLS), ("quads", QUAD_CALLS)) for call in calls]
SMALLEST_TILE = 128  # kGpTile of k_geometric_product


def _mesh(name):
    """(xyz, tri, quad)"""
    none = np.zeros((0, 4), np.int32)
    if name == "panel":
        m = meshes.structured(70, 45, 0, 0, 7, 4.5, kind="t", ul_lr=True)
        xyz = m.xyz.copy()
        xyz[:, 2] = 0.3 * np.sin(0.9 * xyz[:, 0]) * np.cos(0.7 * xyz[:, 1])
        return xyz, m.tri, none
    if name in ("hub", "hub96"):  # the fan of test_gpu_assembly_bits; "hub96": its ring refined to 96 triangles
        v = 40 if name == "hub" else 96
        m = meshes.structured(20, 20, 0, 0, 2, 2, kind="t", ul_lr=True)
        ang = np.linspace(0.0, 2.0 * np.pi, v + 1)[:-1]
        hub = len(m.xyz)
        ring = np.stack([3.0 + 0.5 * np.cos(ang), 1.0 + 0.5 * np.sin(ang), np.zeros(v)], axis=1)
        xyz = np.concatenate([m.xyz, [[3.0, 1.0, 0.2]], ring])
        fan = np.array([[hub, hub + 1 + k, hub + 1 + (k + 1) % v] for k in range(v)], dtype=np.int32)
        return xyz, np.concatenate([m.tri, fan]).astype(np.int32), none
    m = meshes.structured(24, 18, 0, 0, 2.4, 1.8, kind="q")  # "quads": row 9 of the 18 rows cut into triangles
    xyz = m.xyz.copy()
    xyz[:, 2] = 0.2 * np.sin(1.3 * xyz[:, 0]) * np.cos(1.1 * xyz[:, 1])
    pick = np.arange(len(m.quad)) // 24 == 9
    q = m.quad[pick]
    tri = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]]).astype(np.int32)
    return xyz, tri, m.quad[~pick].copy()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64) + 0.0).tobytes()).hexdigest()


def densest_slice_entries(pkg, name):
    xyz, tri, quad = _mesh(name)
    return int(np.diff(pkg.build_plan(xyz, tri, quad)["slice_elem_ptr"]).max())


def digests_of_this_tree():
    pkg = ensure_built()
    out = {}
    for name in ("panel", "hub", "hub96", "quads"):
        xyz, tri, quad = _mesh(name)
        n, nt, nq = len(xyz), len(tri), len(quad)
        rng = np.random.default_rng(41)
        tl, ql = rng.normal(size=(nt, 4)), rng.normal(size=(nq, 4))
        temps = rng.uniform(-50.0, 50.0, (nt, 2))
        u = 1e-3 * rng.normal(size=(n, 6))
        X = rng.uniform(-1.0, 1.0, (3, n, 6))
        fs = pkg.FemShell(0.3, 2.1e5, 0.04)
        fs.set_mesh(xyz, tri, quad)
        got = {}
        fs.set_element_loads(tl, ql if nq else None)
        got["element_loads"] = fs.element_load_vector()
        if name == "quads":
            dmask = np.zeros(n, np.uint8)
            dmask[rng.choice(n, n // 9, replace=False)] = rng.integers(1, 64, n // 9).astype(np.uint8)
            fs.set_dirichlet(dmask)
            fs.set_loads(rng.normal(size=(n, 6)))
            fs.assemble()
            _, _, got["bsr_vals"], got["bsr_F"] = fs.export_bsr()
        else:
            got["geometric_product_1"] = fs.geometric_product(u, X[0])
            got["geometric_product_3"] = fs.geometric_product(u, X)
            got["resultants"] = fs.element_resultants(u)
            fs.set_expansion(1.2e-5)
            fs.set_thermal(temps)
            got["thermal_loads"] = fs.thermal_load_vector()
            got["resultants_thermal"] = fs.element_resultants(u)
        fs.close()
        for call, a in got.items():
            assert np.all(np.isfinite(a)) and np.abs(a).max() > 0.0, (name, call)
            out["%s-%s" % (name, call)] = {"sha256": _sha(a), "size": int(np.asarray(a).size)}
    return out


@pytest.fixture(scope="module")
def digests():
    return digests_of_this_tree()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_names_its_commit_and_every_case(golden):
    assert len(golden["parent_commit"]) == 40
    assert sorted(golden["cases"]) == sorted(CASES)


def test_the_refined_hub_slice_list_is_longer_than_the_smallest_tile(golden):
    got = densest_slice_entries(ensure_built(), "hub96")
    print("hub96: densest slice list", got, "entries")
    assert got > SMALLEST_TILE and got == golden["hub96_densest_slice_entries"]


@pytest.mark.parametrize("case", CASES)
def test_derived_kernels_give_the_bits_of_the_parent_commit(case, digests, golden):
    want, got = golden["cases"][case], digests[case]
    print(case, got["sha256"])
    assert got["size"] == want["size"]
    assert got["sha256"] == want["sha256"]


if __name__ == "__main__":
    pkg_ = ensure_built()
    print(json.dumps({"hub96_densest_slice_entries": densest_slice_entries(pkg_, "hub96"), "cases": digests_of_this_tree()}))
