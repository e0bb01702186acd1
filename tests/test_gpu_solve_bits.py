"""The kernels of the solve give the bits of a recorded parent commit.

tests/golden/solve_bits/parent_digests.json holds, per case, sha256 of `array + 0.0` (signed zeros folded) of the float64
arrays a case produces, and its iteration counts, computed on an MI355X at the commit the file names -- the last one before the
launchers of the products were folded into one entry point with one epilogue description, the lane-per-scalar-row twins of the
node kernels were retired and kernels.hip was split by subject.  Those changes move launch code only: the same kernels with the
same grids, LDS sizes and arguments, so every case must give the same digests.

Single-rank cases, all on the 48 x 48 triangle panel of cycle_worker.panel_context (2401 nodes, a last slice of one node, three
or more levels), one child process per environment (several knobs are read once per process).  The "amg" cases digest pc_apply
on a random vector and on the load vector, then solution and residual_history of solve(rtol=1e-10); the "jacobi" cases solution
and history of the classic CG:

  default     float copies, k_pcg_update_start_node, fused starts, the kept product of the prolongation, the node product for P
  sym         FP64 levels, symmetric coarse levels: first phase + gather, k_sym_gather_start_node
  start       FP64, full-storage coarse levels, every fusion: the `start` epilogue of k_spmv
  cheb_step   the same without the fused Chebyshev step: plain product + k_cheb_step_node
  residual    FP64, no residual increments: Cycle::residual through the base_vec epilogue
  width0      FEMSHELL_SPMV_NODE_WIDTH=0: every full-storage product through k_spmv
  jacobi      k_spmv_sym + k_cg_update_node<true>
  jacobi_full FEMSHELL_SYMMETRIC=0: full storage, k_spmv with partials

  ranks2      two ranks on one GPU over tests/helpers/fake_rccl (as tests/test_multirank_gpu.py drives its workers), an 8 x 96
              strip cut across, default halo overlap: each rank's owned rows of the block-Jacobi solve (single-reduction
              recurrence: the product over interior / boundary spans, k_cgcg_update) and of the "amg" solve (the epilogues over
              the spans), with both histories.  Its digests repeated over two runs of the parent commit before they were
              recorded.

python tests/test_gpu_solve_bits.py  prints the digests of all cases as JSON (CASE: of one case, in this process).
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "solve_bits", "parent_digests.json")
PARENT_COMMIT = "cf197fe01d21aa2b557cc2d9f41e9938b1c435f6"  # the commit the digests were recorded at
FAKE_DIR = os.path.join(ROOT, "tests", "helpers", "fake_rccl")
FP64 = {"FEMSHELL_AMG_SMOOTH_F32": "0"}
FULL = dict(FP64, FEMSHELL_AMG_COARSE_SYM="100000", FEMSHELL_AMG_FUSE="-1")
# case: (preconditioner, environment)
SINGLE = {"default": ("amg", {}),
          "sym": ("amg", dict(FP64, FEMSHELL_AMG_COARSE_SYM="1")),
          "start": ("amg", FULL),
          "cheb_step": ("amg", dict(FULL, FEMSHELL_AMG_FUSED_CHEB="0")),
          "residual": ("amg", dict(FP64, FEMSHELL_AMG_RESIDUAL_INCREMENT="0")),
          "width0": ("amg", {"FEMSHELL_SPMV_NODE_WIDTH": "0"}),
          "jacobi": ("jacobi", {}),
          "jacobi_full": ("jacobi", {"FEMSHELL_SYMMETRIC": "0"})}
CASES = list(SINGLE) + ["ranks2"]


def _sha(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert np.all(np.isfinite(a)) and np.abs(a).max() > 0.0
    return hashlib.sha256((a + 0.0).tobytes()).hexdigest()


def _solve_digest(fs, out, tag=""):
    u, info = fs.solve(rtol=1e-10, max_it=100000)
    assert info["converged"] == 1, info
    out[tag + "u"], out[tag + "history"], out[tag + "iterations"] = _sha(u), _sha(fs.residual_history()), int(info["iterations"])
    return u


def digests_of_this_process(case):
    """One single-rank case in this process's environment."""
    from tests.helpers import cycle_ref
    from tests.helpers.cycle_worker import panel_context

    fs, m = panel_context()
    out = {}
    if SINGLE[case][0] == "amg":
        fs.assemble()
        r = np.random.default_rng(7).standard_normal(6 * m.n_nodes) * cycle_ref.free_dofs(fs)
        out["z"] = _sha(fs.pc_apply(r))
        out["zF"] = _sha(fs.pc_apply(fs.export_bsr()[3]))
        assert len(fs.amg_levels()) >= 3
    else:
        fs.set_preconditioner("jacobi")
    _solve_digest(fs, out)
    fs.close()
    return out


def digests_of_this_rank(rank, uid_file):
    """Rank `rank` of the two of case ranks2."""
    from tests.helpers import meshes
    from tests.helpers.product import ensure_built

    pkg = ensure_built()
    m = meshes.structured(8, 96, 0, 0, 1, 12, kind="t", ul_lr=True, bcids=(0, 0, 1, -1), factor=3.0, loading=2)
    fs = pkg.FemShell(0.3, 2.0e5, 0.05, device=0, rank=rank, world_size=2)
    if rank == 0:
        np.save(uid_file + ".tmp.npy", pkg.comm_unique_id())
        os.replace(uid_file + ".tmp.npy", uid_file)
    else:
        t0 = time.time()
        while not os.path.exists(uid_file):
            if time.time() - t0 > 60:
                raise SystemExit("timeout waiting for the unique id")
            time.sleep(0.01)
    fs.comm_init(np.load(uid_file))
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    b, e = fs.row_range()
    assert 0 < e - b < m.n_nodes
    out = {}
    u = _solve_digest(fs, out, "jacobi_")
    out["jacobi_u"] = _sha(u[b:e])  # (the owned rows: the others arrive by the final gather)
    fs.set_preconditioner("amg", coarsest_nodes=60)
    u = _solve_digest(fs, out, "amg_")
    out["amg_u"] = _sha(u[b:e])
    assert len(fs.amg_levels()) >= 2
    fs.close()
    return {"rank%d_%s" % (rank, k): v for k, v in out.items()}


def _clean_env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FEMSHELL_")}
    env.update(extra)
    return env


def _last_json(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def digests_by_child_processes(cases=CASES):
    from tests.helpers.product import ensure_built

    ensure_built()
    got = {}
    for case in cases:
        if case != "ranks2":
            got[case] = _last_json(subprocess.run([sys.executable, os.path.abspath(__file__), case], env=_clean_env(SINGLE[case][1]),
                                                  capture_output=True, text=True, timeout=300))
            continue
        subprocess.check_call(["make", "-C", FAKE_DIR, "-s"])
        env = _clean_env({"FEMSHELL_RCCL_LIB": os.path.join(FAKE_DIR, "libfake_rccl.so")})
        with tempfile.TemporaryDirectory() as tmp:
            uid = os.path.join(tmp, "uid.npy")
            procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "rank", str(r), uid], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True) for r in range(2)]
            got[case] = {}
            try:
                for p in procs:
                    out, err = p.communicate(timeout=240)
                    assert p.returncode == 0, out[-2000:] + err[-2000:]
                    got[case].update(json.loads(out.strip().splitlines()[-1]))
            finally:
                for p in procs:
                    if p.poll() is None:
                        p.kill()
    return got


@pytest.fixture(scope="module")
def digests():
    return digests_by_child_processes()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_names_its_commit_and_every_case(golden):
    assert golden["parent_commit"] == PARENT_COMMIT
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_the_solve_gives_the_bits_of_the_parent_commit(case, digests, golden):
    want, got = golden["cases"][case], digests[case]
    print(case, json.dumps(got))
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (case, key)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rank":
        print(json.dumps(digests_of_this_rank(int(sys.argv[2]), sys.argv[3])))
    elif len(sys.argv) > 1:
        print(json.dumps(digests_of_this_process(sys.argv[1])))
    else:
        print(json.dumps(digests_by_child_processes(), indent=1, sort_keys=True))
