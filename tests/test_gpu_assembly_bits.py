"""The assembly kernels give the bits of a recorded parent commit.

tests/golden/assembly_bits/parent_digests.json holds, per case, sha256 of `vals + 0.0` (signed zeros folded) and of `F`
as export_bsr returns them, computed on an MI355X at the commit the file names -- the last one before the consumer waves
of k_assemble_pipe lost their bookkeeping instructions (lane shifts without the `old` operand, no accumulator zero-fill,
node-pair index arithmetic from packed constants).  Those changes are moves and integer work only, so every case must
give the same digests:

  panel  the warped 70 x 45 triangle panel of test_pipelined_and_two_phase_assembly_kernels_agree: full and partial
         slices, boundary slices with fewer than 192 items, a last slice of fewer than 32 nodes
  patch  meshes.delaunay_patch(3000, 7): slots of one to four chunks, mixed waves, diagonal slots through the general routine
  hub    a fan of 40 triangles around one node: a slot of 14 chunks, the generic lane-shift loops

each with random Dirichlet masks and loads, through k_assemble_pipe with the default grid and with FEMSHELL_ASM_PIPE_GRID=8
(a workgroup walks many slices, the producer's held records cross them), and the panel once more through k_assemble
(FEMSHELL_ASM_PIPE=0), which shares the block functions.  The grid knob is read once per process, so each grid is one
child process that assembles all its cases:  python tests/test_gpu_assembly_bits.py  prints its digests as JSON.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import meshes  # noqa: E402
from tests.helpers.product import ensure_built  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "assembly_bits", "parent_digests.json")
GRIDS = ("default", "8")
# (mesh, FEMSHELL_ASM_PIPE, kernel, grids): 2 = the pipelined layout wherever the kernel can run
RUNS = (("panel", "2", "k_assemble_pipe", GRIDS), ("patch", "2", "k_assemble_pipe", GRIDS), ("hub", "2", "k_assemble_pipe", GRIDS),
        ("panel", "0", "k_assemble", ("default",)))
CASES = ["%s-pipe%s-grid_%s" % (mesh, pipe, grid) for mesh, pipe, _, grids in RUNS for grid in grids]


def _mesh(name):
    if name == "panel":
        m = meshes.structured(70, 45, 0, 0, 7, 4.5, kind="t", ul_lr=True)
        xyz, tri = m.xyz.copy(), m.tri
        xyz[:, 2] = 0.3 * np.sin(0.9 * xyz[:, 0]) * np.cos(0.7 * xyz[:, 1])
        return xyz, tri
    if name == "patch":
        return meshes.delaunay_patch(3000, 7)
    m = meshes.structured(20, 20, 0, 0, 2, 2, kind="t", ul_lr=True)  # "hub": the fan of test_gpu_parity._fan_mesh
    ang = np.linspace(0.0, 2.0 * np.pi, 41)[:-1]
    hub = len(m.xyz)
    ring = np.stack([3.0 + 0.5 * np.cos(ang), 1.0 + 0.5 * np.sin(ang), np.zeros(40)], axis=1)
    xyz = np.concatenate([m.xyz, [[3.0, 1.0, 0.2]], ring])
    fan = np.array([[hub, hub + 1 + k, hub + 1 + (k + 1) % 40] for k in range(40)], dtype=np.int32)
    return xyz, np.concatenate([m.tri, fan]).astype(np.int32)


def digests_of_this_process(grid):
    """Assembles every case of one grid setting (the process's: FEMSHELL_ASM_PIPE_GRID is read once) and returns its digests."""
    pkg = ensure_built()
    out = {}
    for mesh, pipe, kernel, grids in RUNS:
        if grid not in grids:
            continue
        xyz, tri = _mesh(mesh)
        n = len(xyz)
        rng = np.random.default_rng(12)
        dmask = np.zeros(n, np.uint8)
        dmask[rng.choice(n, n // 9, replace=False)] = rng.integers(1, 64, n // 9).astype(np.uint8)
        loads = rng.normal(size=(n, 6))
        os.environ["FEMSHELL_ASM_PIPE"] = pipe  # (read per femshell_set_mesh)
        fs = pkg.FemShell(0.3, 2.1e5, 0.04)
        fs.set_mesh(xyz, tri)
        assert fs.assembly_kernel() == kernel, (mesh, pipe, fs.assembly_kernel())
        fs.set_dirichlet(dmask)
        fs.set_loads(loads)
        fs.assemble()
        _, _, vals, F = fs.export_bsr()
        fs.close()
        assert np.all(np.isfinite(vals)) and np.abs(vals).max() > 0.0
        out["%s-pipe%s-grid_%s" % (mesh, pipe, grid)] = {
            "vals": hashlib.sha256(np.ascontiguousarray(vals + 0.0).tobytes()).hexdigest(),
            "F": hashlib.sha256(np.ascontiguousarray(F).tobytes()).hexdigest(),
            "vals_size": int(vals.size)}
    return out


def digests_by_child_processes():
    got = {}
    for grid in GRIDS:
        env = dict(os.environ)
        env.pop("FEMSHELL_ASM_PIPE_GRID", None)
        env.pop("FEMSHELL_SYMMETRIC", None)
        if grid != "default":
            env["FEMSHELL_ASM_PIPE_GRID"] = grid
        r = subprocess.run([sys.executable, os.path.abspath(__file__), grid], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got.update(json.loads(r.stdout.strip().splitlines()[-1]))
    return got


@pytest.fixture(scope="module")
def digests():
    return digests_by_child_processes()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_names_its_commit_and_every_case(golden):
    assert len(golden["parent_commit"]) == 40
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_assembly_gives_the_bits_of_the_parent_commit(case, digests, golden):
    want, got = golden["cases"][case], digests[case]
    print(case, "vals", got["vals"], "F", got["F"])
    assert got["vals_size"] == want["vals_size"]
    assert got["F"] == want["F"]
    assert got["vals"] == want["vals"]


if __name__ == "__main__":
    print(json.dumps(digests_of_this_process(sys.argv[1])))
