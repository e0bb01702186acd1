"""The derived state of a context on the GPU (csrc/api_state.cpp): after every kind of change a long-lived
context solves to the bits of a fresh context that was handed the final inputs only, and rebuilds exactly what
femshell_stale_after says the change made stale.

The project holds solves to bits across contexts and processes (tests/test_gpu_solve_bits.py), so every comparison here is
np.testing.assert_array_equal, not a tolerance.  What a solve rebuilt is read off femshell_solve_info: assemble_seconds,
setup_seconds and pc_setup_seconds are 0 exactly when K, the block-Jacobi inverse and the multigrid hierarchy were reused.

Static cases run on the 48 x 48 triangle panel of cycle_worker.panel_context (2401 nodes, a last slice of one node, three or more
levels), dynamics on the 44 x 40 curved patch tests/test_gpu_dynamics.py steps on; each with both preconditioners."""
import functools

import numpy as np
import pytest

from tests.helpers import meshes, sections
from tests.helpers.cycle_worker import panel_context
from tests.helpers.product import ensure_built
from tests.test_gpu_dynamics import MAX_IT, RHO, RTOL, context as patch_context

pytestmark = pytest.mark.gpu
pkg = ensure_built()

INVALID = -1
PCS = ["jacobi", "amg"]
DT = 1e-3
REBUILDS = {"K": "assemble_seconds", "Jacobi": "setup_seconds", "Hierarchy": "pc_setup_seconds"}


def needed(pc):
    return {"K", "Jacobi"} | ({"Hierarchy"} if pc == "amg" else set())


def rebuilt(info):
    return {product for product, seconds in REBUILDS.items() if info[seconds] > 0.0}


def solve(fs):
    """(u, residual history, iterations, what the solve rebuilt)"""
    u, info = fs.solve(rtol=1e-10, max_it=100000)
    assert info["converged"] == 1, info
    return u, fs.residual_history(), int(info["iterations"]), rebuilt(info)


def same_bits(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2] == want[2]


# ------------------------------------------------------------------ the inputs of the panel, by name

@functools.lru_cache(maxsize=None)
def panel():
    fs, m = panel_context()
    fs.close()
    return m


def value(name):
    m = panel()
    if name == "mask":
        return m.dirichlet_mask()
    if name == "mask2":  # the node nearest the middle of the panel clamped as well
        mask = m.dirichlet_mask().copy()
        mask[np.argmin(((m.xyz[:, :2] - 5.0) ** 2).sum(axis=1))] = 0x3F
        assert (mask != m.dirichlet_mask()).sum() == 1
        return mask
    if name == "loads":
        return m.loads
    if name == "loads2":
        return 1.25 * m.loads[::-1]
    if name == "prescribed":  # counts where the Dirichlet set fixes a dof: the clamped boundary moves and tilts
        u = np.zeros((m.n_nodes, 6))
        u[:, 2] = 1e-3 * np.sin(0.7 * m.xyz[:, 0]) * np.cos(0.4 * m.xyz[:, 1])
        u[:, 3] = 2e-4 * m.xyz[:, 1]
        assert np.abs(u[m.dirichlet_mask() != 0]).max() > 0.0
        return u
    if name == "sections":  # two materials, split along x = 4 (no multiple of the slice or the mesh width)
        tri_section = (m.xyz[m.tri].mean(axis=1)[:, 0] > 4.0).astype(np.int32)
        assert 0 < tri_section.sum() < len(tri_section)
        return np.array([[0.3, 1e7, 0.5], [0.25, 2.5e7, 0.3]]), tri_section
    raise KeyError(name)


BASE = {"mask": "mask", "loads": "loads", "prescribed": None, "sections": None, "density": None, "pc_options": ()}


def apply_inputs(fs, pc, inputs):
    fs.set_dirichlet(value(inputs["mask"]))
    fs.set_loads(value(inputs["loads"]))
    if inputs["sections"]:
        fs.set_sections(*value(inputs["sections"]))
    if inputs["density"]:
        fs.set_density(inputs["density"])
    if inputs["prescribed"]:
        fs.set_prescribed(value(inputs["prescribed"]))
    set_pc(fs, pc, inputs["pc_options"])


def set_pc(fs, pc, options):
    if pc == "amg":
        fs.set_preconditioner("amg", **dict((("cycle", "K"), ("coarsest_nodes", 60)) + tuple(options)))
    else:
        fs.set_preconditioner("jacobi", **dict(options))


def panel_with(pc, inputs):
    m = panel()
    fs = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    apply_inputs(fs, pc, inputs)
    return fs


@functools.lru_cache(maxsize=None)
def fresh(pc, items):
    """The solve of a fresh context with these inputs: computed once per (preconditioner, inputs), read by every case."""
    fs = panel_with(pc, dict(items))
    got = solve(fs)
    levels = len(fs.amg_levels())
    fs.close()
    assert got[3] == needed(pc) and (levels >= 3 if pc == "amg" else levels == 0)
    for a in got[:2]:
        a.setflags(write=False)
    return got


# ------------------------------------------------------------------ 1. every row of the table against a fresh context

# case: (row of the table or None where nothing is stale, inputs before (changes of BASE), the call, inputs after)
ROWS = {
    "dirichlet": ("dirichlet", {}, lambda fs, pc: fs.set_dirichlet(value("mask2")), {"mask": "mask2"}),
    "loads": ("loads", {}, lambda fs, pc: fs.set_loads(value("loads2")), {"loads": "loads2"}),
    "prescribed_set": ("prescribed", {}, lambda fs, pc: fs.set_prescribed(value("prescribed")), {"prescribed": "prescribed"}),
    "prescribed_cleared": ("prescribed", {"prescribed": "prescribed"}, lambda fs, pc: fs.set_prescribed(None), {}),
    "sections_set": ("sections", {}, lambda fs, pc: fs.set_sections(*value("sections")), {"sections": "sections"}),
    "sections_cleared": ("sections", {"sections": "sections"}, lambda fs, pc: fs.set_sections(None), {}),
    "sections_cleared_none_set": ("sections_cleared_none_set", {}, lambda fs, pc: fs.set_sections(None), {}),
    "density": ("density", {"density": RHO}, lambda fs, pc: fs.set_density(2.7e-3), {"density": 2.7e-3}),
    "pc_options": ("pc_options", {}, lambda fs, pc: set_pc(fs, pc, (("smoother_degree", 2),)), {"pc_options": (("smoother_degree", 2),)}),
    "pc_options_same_hierarchy": (None, {}, lambda fs, pc: set_pc(fs, pc, (("refine_passes", 2),)), {"pc_options": (("refine_passes", 2),)}),
    "assembled": ("assembled", {}, lambda fs, pc: fs.assemble(), {}),
    "timed_assembly": ("assembled", {}, lambda fs, pc: fs.time_kernel(pkg.KERNEL_ASSEMBLE, 1), {}),
    "modes_with_a_shift": ("matrix_spoiled", {"density": RHO}, lambda fs, pc: fs.modes(2, tol=1e-3, shift=50.0, max_it=40, want_modes=False),
                           {"density": RHO}),
    "mesh": ("mesh", {}, lambda fs, pc: (fs.set_mesh(panel().xyz, panel().tri, panel().quad), apply_inputs(fs, pc, BASE)), {}),
}


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", list(ROWS))
def test_after_a_change_the_context_solves_like_a_fresh_one_and_rebuilds_what_the_table_says(case, pc):
    change, before, call, after = ROWS[case]
    before, after = dict(BASE, **before), dict(BASE, **after)
    fs = panel_with(pc, before)
    same_bits(solve(fs), fresh(pc, tuple(sorted(before.items()))))
    call(fs, pc)
    got = solve(fs)
    fs.close()
    stale = pkg.stale_after(change) if change else frozenset()
    print(case, pc, "stale:", sorted(stale), "rebuilt:", sorted(got[3]))
    assert got[3] == set(stale) & needed(pc)
    same_bits(got, fresh(pc, tuple(sorted(after.items()))))


@functools.lru_cache(maxsize=None)
def patch():
    return sections.curved_patch(44, 40)


@pytest.mark.parametrize("pc", PCS)
def test_dynamics_begin_to_end_leaves_a_context_that_solves_like_a_fresh_one(pc):
    m = patch()
    fs = patch_context(m, pc=pc, loads=m.loads)
    want = solve(fs)
    assert want[3] == needed(pc) and (pc != "amg" or len(fs.amg_levels()) >= 2)
    fs.dynamics_begin(DT)
    info = fs.dynamics_step(rtol=RTOL, max_it=MAX_IT)
    assert info["converged"] == 1 and rebuilt(info) == set(pkg.stale_after("dynamics_begin")) & needed(pc)
    fs.dynamics_accept()
    fs.dynamics_end()
    assert fs.amg_levels() == []
    got = solve(fs)
    fs.close()
    assert got[3] == set(pkg.stale_after("dynamics_end")) & needed(pc)
    same_bits(got, want)


# ------------------------------------------------------------------ 3. defect B, and the timed mass shift: twins in dynamics

@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("which", ["timed_assembly", "timed_mass_shift"])
def test_a_timed_kernel_between_two_steps_leaves_the_steps_of_a_twin(which, pc):
    """One of two twins times the assembly kernel once (the matrix in HBM must be K_eff again afterwards, and what was derived
    from the previous matrix gone), or the mass shift three times (K_eff is spoiled and built again), between two accepted steps:
    its second step gives the state and the iteration count of the twin that did not."""
    m = patch()
    kernel, reps, change = {"timed_assembly": (pkg.KERNEL_ASSEMBLE, 1, "assembled"),
                            "timed_mass_shift": (pkg.binding.KERNEL_MASS_SHIFT, 3, "matrix_spoiled")}[which]
    states, iterations = [], []
    for timed in (True, False):
        fs = patch_context(m, pc=pc, loads=m.loads)
        fs.dynamics_begin(DT)
        assert fs.dynamics_step(rtol=RTOL, max_it=MAX_IT)["converged"] == 1
        fs.dynamics_accept()
        if timed:
            fs.time_kernel(kernel, reps)
        info = fs.dynamics_step(rtol=RTOL, max_it=MAX_IT)
        assert info["converged"] == 1, info
        assert rebuilt(info) == (set(pkg.stale_after(change)) & needed(pc) if timed else set())
        states.append(fs.dynamics_state(candidate=True))
        iterations.append(info["iterations"])
        fs.dynamics_end()
        fs.close()
    assert np.abs(states[1][0]).max() > 0.0
    for a, b in zip(*states):
        np.testing.assert_array_equal(a, b)
    assert iterations[0] == iterations[1]


# ------------------------------------------------------------------ 2. defect A: a refused mesh over an assembled context

@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("v", [766, 765])
def test_a_refused_mesh_leaves_nothing_of_the_previous_one_valid(monkeypatch, v, pc):
    """coil(766) is refused inside build_plan, which has overwritten the plan by then; coil(765) after the device view points
    at the new, zero-filled buffers.  Every call that needs a mesh or K then refuses on the host, before its first launch, and
    the panel set again gives the bits of a fresh context."""
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    m = panel()
    fs = panel_with(pc, BASE)
    fs.assemble()
    same_bits(solve(fs), fresh(pc, tuple(sorted(BASE.items()))))
    with pytest.raises(pkg.FemShellError):
        fs.set_mesh(*meshes.coil(v))
    x, z = np.ones(6 * m.n_nodes), np.zeros(6 * m.n_nodes)
    first = "call femshell_assemble first"
    calls = [(lambda: fs.spmv(x), first), (lambda: fs.residual(x), first), (fs.export_bsr, first), (lambda: fs.spmm(x.reshape(1, -1)), first),
             (fs.assemble, "no mesh set"), (fs.solve, "no mesh set"),
             # (FemShell.pc_apply sizes its arrays by the owned rows, of which there are none: the C entry point itself)
             (lambda: pkg.binding._check(fs._L.femshell_pc_apply(fs._h, pkg.binding._d(x), pkg.binding._d(z))), "no mesh set")]
    for call, message in calls:
        with pytest.raises(pkg.FemShellError) as ei:
            call()
        assert ei.value.code == INVALID and message in str(ei.value), str(ei.value)
    assert fs.amg_levels() == []
    fs.set_mesh(m.xyz, m.tri, m.quad)
    apply_inputs(fs, pc, BASE)
    got = solve(fs)
    fs.close()
    assert got[3] == needed(pc)
    same_bits(got, fresh(pc, tuple(sorted(BASE.items()))))


# ------------------------------------------------------------------ 4. defect C: a new mesh drops the hierarchy at once

def test_a_new_mesh_drops_the_hierarchy_of_the_previous_one():
    m = panel()
    fs = panel_with("amg", BASE)
    solve(fs)
    assert len(fs.amg_levels()) >= 3 and fs.amg_setup_stats()["galerkin_ms"] >= 0.0
    fs.set_mesh(m.xyz, m.tri, m.quad)
    assert fs.amg_levels() == []
    with pytest.raises(pkg.FemShellError) as ei:
        fs.amg_setup_stats()
    assert ei.value.code == INVALID and "no multigrid hierarchy" in str(ei.value)
    fs.close()
