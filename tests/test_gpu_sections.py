"""Shell sections on the GPU (femshell_set_sections): thickness and material per element, through the C ABI, against the
CPU oracle.  The reference of every assembled matrix is the oracle's assembly section by section, summed
(tests/helpers/sections.py; pinned on the CPU by tests/test_sections_cpu.py).  Tolerances are those of
tests/test_gpu_parity.py: element matrices and K 1e-12, two kernels / two instantiations of one kernel 1e-13,
displacements 1e-9 of the direct solve."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import oracle, sections
from tests.helpers.product import ROOT, ensure_built
from tests.test_gpu_parity import random_quads, random_tris

pytestmark = pytest.mark.gpu
pkg = ensure_built()


def rel_max(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------ 1. element matrices

@pytest.mark.parametrize("flags", [3, 0])
def test_element_matrices_take_the_elements_own_section(flags):
    sec = sections.wide_sections(7, 40 + flags)
    mats = [oracle.material(nu, E, t, flags) for nu, E, t in sec]
    rng = np.random.default_rng(flags)
    xyz, tri = random_tris(257, seed=21 + flags)
    ts = rng.integers(0, 7, len(tri)).astype(np.int32)
    fs = pkg.FemShell(0.3, 2.1e5, 0.37, flags=flags)
    fs.set_mesh(xyz, tri)
    fs.set_sections(sec, ts)
    Ke = fs.element_matrices(0, len(tri))
    worst = 0.0
    for e in range(len(tri)):
        ref = oracle.element_tri3(xyz[tri[e]], mats[ts[e]])
        worst = max(worst, np.linalg.norm(Ke[e] - ref) / np.linalg.norm(ref))
    print("triangles, flags %d: worst element %.2e" % (flags, worst))
    assert worst <= 1e-12, worst
    xyz, quad = random_quads(129, seed=15 + flags)
    qs = rng.integers(0, 7, len(quad)).astype(np.int32)
    fs.set_mesh(xyz, None, quad)
    fs.set_sections(sec, None, qs)
    Ke = fs.element_matrices(0, len(quad))
    worst = 0.0
    for e in range(len(quad)):
        ref = oracle.element_quad4(xyz[quad[e]], mats[qs[e]])
        worst = max(worst, np.linalg.norm(Ke[e] - ref) / np.linalg.norm(ref))
    print("quadrilaterals, flags %d: worst element %.2e" % (flags, worst))
    assert worst <= 1e-12, worst
    fs.close()


# ------------------------------------------------------------------ 2. assembled K

CASES = {"ibeam": sections.ibeam, "mixed": sections.mixed_patch, "delaunay": sections.delaunay_random,
         "taper": sections.tapered_panel}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("symmetric", ["1", "0"])
@pytest.mark.parametrize("pipe", ["default", "0"])
def test_assembled_matrix_equals_the_split_sum(monkeypatch, case, symmetric, pipe):
    """I-beam (web / flanges), mixed triangle + quadrilateral patch in three strips, Delaunay shell with a random section
    out of seven per element, structured panel with ONE SECTION PER ELEMENT (tapered thickness, 4:1); symmetric and full
    storage; the kernel the plan chooses and the two-phase kernel forced."""
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", symmetric)
    if pipe == "0":
        monkeypatch.setenv("FEMSHELL_ASM_PIPE", "0")
    else:
        monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    cs = CASES[case]()
    fs = pkg.FemShell(0.3, 2.1e5, 0.04)
    fs.set_mesh(cs.xyz, cs.tri, cs.quad)
    before = fs.assembly_kernel()
    cs.apply(fs)
    kernel = fs.assembly_kernel()
    plan = pkg.build_plan(cs.xyz, cs.tri, cs.quad)
    most = int(np.diff(plan["slice_elem_ptr"]).max())
    # what must run: the two-phase kernel where it is forced or the plan chose it, else the pipelined one where its sectioned
    # records fit (all of these meshes)
    if pipe == "0":
        assert before == kernel == "k_assemble"
    else:
        fits = len(cs.quad) > 0 or most <= 134
        assert kernel == (before if fits else "k_assemble")
        if case in ("taper", "mixed") and symmetric == "1":
            # the pipelined kernel with sections, in both of its instantiations: triangles with one section per element, and
            # the mixed patch (the only case that runs the one for meshes with quadrilaterals)
            assert kernel == "k_assemble_pipe"
    fs.assemble()
    rowptr, colidx, vals, F = fs.export_bsr()
    r0, c0, v0, F0 = sections.reference(cs)
    np.testing.assert_array_equal(rowptr, r0)
    np.testing.assert_array_equal(colidx, c0)
    np.testing.assert_array_equal(F, F0)
    print("%s sym %s pipe %s: %s, max %.2e, Frobenius %.2e" % (case, symmetric, pipe, kernel, rel_max(vals, v0),
                                                          np.linalg.norm(vals - v0) / np.linalg.norm(v0)))
    assert np.linalg.norm(vals - v0) <= 1e-12 * np.linalg.norm(v0)
    assert np.abs(vals - v0).max() <= 1e-12 * np.abs(v0).max()
    fs.close()


def test_both_kernels_ran_with_sections_and_agree(monkeypatch):
    """the tapered panel through the pipelined and through the two-phase kernel, both with sections: 1e-13"""
    cs = sections.tapered_panel()
    out = {}
    for pipe in ("1", "0"):
        if pipe == "0":
            monkeypatch.setenv("FEMSHELL_ASM_PIPE", "0")
        else:
            monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
        fs = cs.apply(pkg.FemShell(0.3, 2.1e5, 0.04))
        assert fs.assembly_kernel() == ("k_assemble_pipe" if pipe == "1" else "k_assemble")
        fs.assemble()
        out[pipe] = fs.export_bsr()[2]
        fs.close()
    assert rel_max(out["1"], out["0"]) <= 1e-13


def test_a_mesh_between_the_caps_changes_kernel_and_comes_back_bitwise(monkeypatch):
    """143 elements in the fullest slice: the pipelined kernel without sections, the two-phase kernel with them (its
    sectioned records would not fit twice into a CU), correct, and after set_sections(None) pipelined again with the bits
    of the first K."""
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    cs = sections.tapered_panel(**sections.BETWEEN_THE_CAPS)
    plan = pkg.build_plan(cs.xyz, cs.tri)
    assert plan["pipe"] == 1 and 134 < int(np.diff(plan["slice_elem_ptr"]).max()) <= 150
    fs = pkg.FemShell(0.3, 2.1e5, 0.04)
    fs.set_mesh(cs.xyz, cs.tri)
    fs.set_dirichlet(cs.dmask)
    fs.set_loads(cs.loads)
    assert fs.assembly_kernel() == "k_assemble_pipe"
    fs.assemble()
    first = fs.export_bsr()
    fs.set_sections(cs.sections, cs.tri_section)
    assert fs.assembly_kernel() == "k_assemble"
    fs.assemble()
    r, c, v, F = fs.export_bsr()
    r0, c0, v0, F0 = sections.reference(cs)
    np.testing.assert_array_equal(r, r0)
    np.testing.assert_array_equal(c, c0)
    np.testing.assert_array_equal(F, F0)
    assert rel_max(v, v0) <= 1e-12
    fs.set_sections(None)
    assert fs.assembly_kernel() == "k_assemble_pipe"
    fs.assemble()
    again = fs.export_bsr()
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    # the two kernels on this mesh, both with sections of one material: 1e-13
    fs.set_sections([[0.3, 2.1e5, 0.04]], np.zeros(len(cs.tri), np.int32))
    fs.assemble()
    assert rel_max(fs.export_bsr()[2], first[2]) <= 1e-13
    fs.close()


# ------------------------------------------------------------------ 3. the neutral element

@pytest.mark.parametrize("case", ["strips", "mixed", "panel"])
def test_sections_equal_to_the_config_change_nothing(case):
    cs = {"strips": sections.three_strips, "mixed": sections.mixed_patch, "panel": sections.tapered_panel}[case]()
    cfg = (0.3, 7.0e4, 0.05)
    fs = pkg.FemShell(*cfg)
    fs.set_mesh(cs.xyz, cs.tri, cs.quad)
    fs.set_dirichlet(cs.dmask)
    fs.set_loads(cs.loads)
    fs.assemble()
    plain = fs.export_bsr()
    tri_arg = (lambda a: a if len(cs.tri) else None)
    quad_arg = (lambda a: a if len(cs.quad) else None)
    rng = np.random.default_rng(1)
    for n in (1, 7):
        ts = rng.integers(0, n, len(cs.tri)).astype(np.int32)
        qs = rng.integers(0, n, len(cs.quad)).astype(np.int32)
        fs.set_sections([cfg] * n, tri_arg(ts), quad_arg(qs))
        fs.assemble()
        v = fs.export_bsr()[2].copy()
        print("%s, %d sections equal to the config: %.2e" % (case, n, rel_max(v, plain[2])))
        assert rel_max(v, plain[2]) <= 1e-13
        fs.assemble()  # run to run: the same bits
        np.testing.assert_array_equal(fs.export_bsr()[2], v)
    fs.set_sections(None)
    fs.assemble()
    for a, b in zip(plain, fs.export_bsr()):
        np.testing.assert_array_equal(a, b)
    fs.close()


# ------------------------------------------------------------------ 4. solve

@pytest.mark.parametrize("case", ["ibeam", "strips"])
@pytest.mark.parametrize("pc", ["block_jacobi", "amg"])
def test_solve_with_sections(case, pc):
    """I-beam with flanges twice as thick as the web, three strips of three materials: converged, the solution within 1e-9
    of the direct solve of the reference matrix; block-Jacobi CG follows the oracle's PCG on that matrix iteration by
    iteration.  (Multigrid iteration counts are printed, not bounded.)"""
    cs = sections.ibeam() if case == "ibeam" else sections.three_strips()
    fs = cs.apply(pkg.FemShell(0.3, 1e4, 0.25))
    if pc == "amg":
        fs.set_preconditioner("amg", coarsest_nodes=40)
    u, info = fs.solve(rtol=1e-13, max_it=100000 if pc == "block_jacobi" else 500)
    r0, c0, v0, F0 = sections.reference(cs)
    u0 = oracle.direct_solve(r0, c0, v0, F0)
    err = np.linalg.norm(u.ravel() - u0) / np.linalg.norm(u0)
    print("%s, %s: %d iterations, %d levels, error against the direct solve %.2e" % (case, pc, info["iterations"], info["amg_levels"], err))
    assert info["converged"] == 1
    assert err <= 1e-9, err
    if pc == "block_jacobi":
        _, info1 = fs.solve(rtol=1e-10, max_it=100000)
        h = fs.residual_history()
        u1, info0 = oracle.pcg(r0, c0, v0, F0, rtol=1e-10, max_it=100000, history=True)
        assert info1["converged"] == 1 and info0["converged"] == 1
        assert abs(info1["iterations"] - info0["iterations"]) <= 2
        k = min(len(h), len(info0["history"]), 60)
        np.testing.assert_allclose(h[:k], info0["history"][:k], rtol=1e-6)
    fs.close()


@pytest.mark.parametrize("pc", ["block_jacobi", "amg"])
def test_changing_the_sections_between_two_solves_rebuilds_everything(pc):
    cs = sections.three_strips()
    other = sections.three_strips(sections=sections.THREE[[2, 0, 1]])
    fs = cs.apply(pkg.FemShell(0.3, 1e5, 0.05))
    if pc == "amg":
        fs.set_preconditioner("amg", coarsest_nodes=40)
    fs.solve(rtol=1e-12, max_it=100000)
    fs.set_sections(other.sections, other.tri_section)
    u, info = fs.solve(rtol=1e-12, max_it=100000)
    assert info["converged"] == 1 and info["assemble_seconds"] > 0.0
    assert (info["pc_setup_seconds"] if pc == "amg" else info["setup_seconds"]) > 0.0
    fresh = other.apply(pkg.FemShell(0.3, 1e5, 0.05))
    if pc == "amg":
        fresh.set_preconditioner("amg", coarsest_nodes=40)
    u1, info1 = fresh.solve(rtol=1e-12, max_it=100000)
    np.testing.assert_array_equal(u, u1)
    assert info["iterations"] == info1["iterations"]
    fs.close()
    fresh.close()


def test_multigrid_iteration_count_of_the_neutral_case():
    """one section equal to the config: the count of the uniform context within one iteration (K differs in the last bits)"""
    cs = sections.three_strips()
    cfg = (0.3, 1e5, 0.05)
    fs = pkg.FemShell(*cfg)
    fs.set_mesh(cs.xyz, cs.tri)
    fs.set_dirichlet(cs.dmask)
    fs.set_loads(cs.loads)
    fs.set_preconditioner("amg", coarsest_nodes=40)
    _, plain = fs.solve(rtol=1e-12, max_it=500)
    fs.set_sections([cfg], np.zeros(len(cs.tri), np.int32))
    _, neutral = fs.solve(rtol=1e-12, max_it=500)
    print("multigrid iterations: uniform %d, one section equal to the config %d" % (plain["iterations"], neutral["iterations"]))
    assert plain["converged"] == 1 and neutral["converged"] == 1
    assert abs(plain["iterations"] - neutral["iterations"]) <= 1
    fs.close()


# ------------------------------------------------------------------ 5. row partition, renumbering

WORKER = os.path.join(ROOT, "tests", "helpers", "sections_worker.py")
FAKE_DIR = os.path.join(ROOT, "tests", "helpers", "fake_rccl")


def run_ranks(world, tmp_path):
    subprocess.check_call(["make", "-C", FAKE_DIR, "-s"])
    env = dict(os.environ, FEMSHELL_RCCL_LIB=os.path.join(FAKE_DIR, "libfake_rccl.so"))
    uid = str(tmp_path / ("uid_%d.npy" % world))
    outs = [str(tmp_path / ("out_%d_%d.npz" % (world, r))) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), uid, outs[r]], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(out.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, "\n".join("--- rank %d\n%s" % (q, logs[q][-1500:]) for q in range(world)))
    return [np.load(o) for o in outs]


@pytest.mark.parametrize("world", [2, 3])
def test_row_partitioned_contexts_with_sections(world, tmp_path):
    """three strips along x over 2 and 3 ranks (bands in y: every section boundary crosses every rank cut): each rank's rows
    of K against the same rows of the reference, the solution against the single-rank one"""
    cs = sections.three_strips(24, 40)
    r0, c0, v0, F0 = sections.reference(cs)
    scale = np.abs(v0).max()
    single = run_ranks(1, tmp_path)[0]
    ranks = run_ranks(world, tmp_path)
    covered = 0
    for r in sorted(ranks, key=lambda q: int(q["begin"])):
        b, e = int(r["begin"]), int(r["end"])
        assert b == covered
        covered = e
        assert 0 < b or e < cs.n_nodes  # a real partition
        # a rank's rows see more than one section
        touched = np.unique(cs.tri_section[np.any((cs.tri >= b) & (cs.tri < e), axis=1)])
        assert len(touched) == 3
        lo, hi = int(r0[b]), int(r0[e])
        np.testing.assert_array_equal(r["k_cols"][:hi - lo], c0[lo:hi])
        assert np.abs(r["k_vals"][:hi - lo] - v0[lo:hi]).max() <= 1e-12 * scale
        np.testing.assert_array_equal(r["k_F"], F0[6 * b:6 * e])
        assert int(r["converged"]) == 1
    assert covered == cs.n_nodes
    err = np.linalg.norm(ranks[0]["u"] - single["u"]) / np.linalg.norm(single["u"])
    print("%d ranks against one: %.2e" % (world, err))
    assert err <= 1e-9, err


def test_sections_under_internal_renumbering():
    """FEMSHELL_REORDER_MORTON on the Delaunay shell: the element arrays stay in the caller's element order"""
    cs = sections.delaunay_random()
    fs = cs.apply(pkg.FemShell(0.3, 7.0e4, 0.03, flags=pkg.REF_DEFAULT | pkg.REORDER_MORTON))
    fs.assemble()
    r, c, v, F = fs.export_bsr()
    r0, c0, v0, F0 = sections.reference(cs)
    np.testing.assert_array_equal(r, r0)
    np.testing.assert_array_equal(c, c0)
    np.testing.assert_array_equal(F, F0)
    assert rel_max(v, v0) <= 1e-12
    fs.close()


# ------------------------------------------------------------------ 6. errors

def test_invalid_calls_are_refused_and_change_nothing():
    cs = sections.mixed_patch()
    empty = pkg.FemShell(0.3, 1e5, 0.05)
    with pytest.raises(pkg.FemShellError) as ei:
        empty.set_sections([[0.3, 1e5, 0.05]])  # (no mesh: no element arrays to give; the library refuses the call itself)
    assert ei.value.code == -1 and "set_mesh" in str(ei.value)
    empty.close()
    fs = cs.apply(pkg.FemShell(0.3, 1e5, 0.05))
    fs.assemble()
    good = fs.export_bsr()
    L, h = fs._L, fs._h
    sec = np.ascontiguousarray(cs.sections)
    ts, qs = cs.tri_section.copy(), cs.quad_section.copy()
    binding = __import__("importlib").import_module("fem-shell_amd.binding")
    dp, ip = binding._d, binding._i
    bad_t, bad_q, neg = ts.copy(), qs.copy(), ts.copy()
    bad_t[5] = 3
    bad_q[2] = 17
    neg[0] = -1

    def with_section(row):
        s = sec.copy()
        s[1] = row
        return s
    calls = {
        "sections is null": (3, None, ts, qs),
        "tri_section is null": (3, sec, None, qs),
        "quad_section is null": (3, sec, ts, None),
        "triangle 5": (3, sec, bad_t, qs),
        "quadrilateral 2": (3, sec, ts, bad_q),
        "triangle 0": (3, sec, neg, qs),
        "n_sections < 0": (-1, sec, ts, qs),
        "section 1": (3, with_section([0.6, 1e5, 0.05]), ts, qs),
    }
    for text, (n, s, t_, q_) in calls.items():
        rc = L.femshell_set_sections(h, n, dp(s), ip(t_), ip(q_))
        assert rc == -1, text
        assert text in L.femshell_last_error().decode(), (text, L.femshell_last_error().decode())
    for row in ([-1.0, 1e5, 0.05], [0.3, 0.0, 0.05], [0.3, 1e5, -0.1], [0.3, float("nan"), 0.05]):
        rc = L.femshell_set_sections(h, 3, dp(with_section(row)), ip(ts), ip(qs))
        assert rc == -1 and "section 1" in L.femshell_last_error().decode(), row
    # the sections that were in force still are
    fs.assemble()
    for a, b in zip(good, fs.export_bsr()):
        np.testing.assert_array_equal(a, b)
    # a new mesh forgets them
    fs.set_mesh(cs.xyz, cs.tri, cs.quad)
    fs.set_dirichlet(cs.dmask)
    fs.set_loads(cs.loads)
    fs.assemble()
    v = fs.export_bsr()[2]
    v0 = oracle.assemble(cs.xyz, cs.tri, cs.quad, oracle.material(0.3, 1e5, 0.05), cs.dmask, cs.loads)[2]
    assert rel_max(v, v0) <= 1e-12
    fs.close()
