"""ctypes mirror of include/femshell.h (no arithmetic here; see __init__.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")

REF_Y21 = 0x1
REF_DRILL_MAX = 0x2
REASSEMBLE_EACH_SOLVE = 0x4
REF_DEFAULT = REF_Y21 | REF_DRILL_MAX
REORDER_MORTON = 0x10
REORDER_RCM = 0x20

KERNEL_ASSEMBLE, KERNEL_SPMV, KERNEL_CG_UPDATE, KERNEL_CG_DIRECTION = 0, 1, 2, 3
KERNEL_LUMPED_MASS, KERNEL_MASS_SHIFT, KERNEL_NEWMARK_RHS, KERNEL_NEWMARK_UPDATE = 4, 5, 6, 7
KERNEL_SPMM, KERNEL_GRAM, KERNEL_BLOCK_COMBINE = 8, 9, 10
KERNEL_ELEMENT_PRODUCT = 11
KERNEL_ELEMENT_RESULTANTS = 12
KERNEL_ELEMENT_LOADS = 13
KERNEL_GEOMETRIC_PRODUCT = 14
KERNEL_ELEMENT_THERMAL = 15
KERNEL_NODAL_RECOVERY = 16
KERNEL_RECOVERY_ERROR = 17
KERNEL_ELASTIC_SUPPORT = 18

SYMBOLS = [
    "femshell_create", "femshell_destroy", "femshell_last_error", "femshell_set_mesh",
    "femshell_set_dirichlet", "femshell_set_loads", "femshell_assemble", "femshell_assemble_async", "femshell_solve",
    "femshell_get_solution", "femshell_residual_history", "femshell_element_matrices",
    "femshell_nnz_blocks", "femshell_export_bsr", "femshell_spmv", "femshell_row_begin",
    "femshell_row_end", "femshell_comm_unique_id", "femshell_comm_init", "femshell_time_kernel",
    "femshell_sync", "femshell_pc_defaults", "femshell_set_preconditioner", "femshell_amg_levels", "femshell_amg_level",
    "femshell_amg_export", "femshell_residual", "femshell_comm_ranks", "femshell_amg_setup_stats", "femshell_amg_dense_stats", "femshell_amg_partition_info", "femshell_assembly_kernel",
    "femshell_amg_cycle_bytes", "femshell_comm_selftest", "femshell_comm_counters", "femshell_owned_nodes", "femshell_comm_bytes", "femshell_set_initial_guess",
    "femshell_amg_patch_info", "femshell_amg_symbolic_info", "femshell_pc_apply", "femshell_set_sections",
    "femshell_set_density", "femshell_lumped_mass", "femshell_dynamics_defaults", "femshell_dynamics_begin", "femshell_dynamics_step",
    "femshell_dynamics_accept", "femshell_dynamics_state", "femshell_dynamics_energy", "femshell_dynamics_end",
    "femshell_modal_defaults", "femshell_modes", "femshell_spmm", "femshell_modal_gram",
    "femshell_set_prescribed", "femshell_reactions", "femshell_element_product", "femshell_element_resultants",
    "femshell_nodal_resultants",
    "femshell_set_element_loads", "femshell_element_load_vector",
    "femshell_set_expansion", "femshell_set_thermal", "femshell_thermal_load_vector",
    "femshell_set_foundation", "femshell_set_springs", "femshell_support_stiffness", "femshell_support_forces",
    "femshell_geometric_product", "femshell_buckling_defaults", "femshell_buckling",
    "femshell_solve_cases", "femshell_combination_envelope",
    "femshell_pool_stats", "femshell_amg_device_dense_inverse", "femshell_amg_dense_apply",
    "femshell_amg_device_block_jacobi", "femshell_block_jacobi_export", "femshell_block_jacobi_apply",
    "femshell_krylov_grid", "femshell_krylov_set", "femshell_krylov_get", "femshell_krylov_launch", "femshell_cg_reduce",
    "femshell_modal_combine", "femshell_modal_residual", "femshell_modal_block_jacobi", "femshell_modal_mask", "femshell_modal_start",
]


def relative_error(elems):
    """sqrt(sum eta^2 / (sum e2 + sum eta^2)) of the element rows FemShell.nodal_resultants returns, summed in their order (0 for
    a mesh that carries nothing)"""
    elems = np.asarray(elems, dtype=np.float64).reshape(-1, 2)
    e2 = eta2 = 0.0
    for a, b in elems:
        e2 += a
        eta2 += b
    return float(np.sqrt(eta2 / (e2 + eta2))) if e2 + eta2 > 0.0 else 0.0


class FemShellError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("femshell error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("nu", C.c_double), ("E", C.c_double), ("thickness", C.c_double), ("flags", C.c_uint32),
                ("device", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32)]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("rel_residual", C.c_double),
                ("true_rel_residual", C.c_double), ("assemble_seconds", C.c_double), ("setup_seconds", C.c_double), ("solve_seconds", C.c_double),
                ("bytes_per_iteration", C.c_double), ("pc_type", C.c_int32), ("amg_levels", C.c_int32),
                ("pc_setup_seconds", C.c_double), ("operator_complexity", C.c_double),
                ("refine_passes_done", C.c_int32), ("pc_fp64_fallback", C.c_int32), ("refine_correction_rel", C.c_double),
                ("refine_residual_reduction", C.c_double), ("error_estimate", C.c_double)]


class PcOptions(C.Structure):
    _fields_ = [("type", C.c_int32), ("cycle", C.c_int32), ("smoother_degree", C.c_int32), ("coarse_degree", C.c_int32),
                ("coarsest_nodes", C.c_int32), ("max_levels", C.c_int32), ("refine_passes", C.c_int32), ("reserved", C.c_int32),
                ("eig_ratio", C.c_double)]


class AmgLevelInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_coarse", C.c_int32), ("nnz_blocks", C.c_int64), ("p_blocks", C.c_int64),
                ("lambda_max", C.c_double)]


class DynamicsOptions(C.Structure):
    _fields_ = [("dt", C.c_double), ("beta", C.c_double), ("gamma", C.c_double), ("alpha", C.c_double)]


class ModalOptions(C.Structure):
    _fields_ = [("n_modes", C.c_int32), ("guard", C.c_int32), ("max_it", C.c_int32), ("reserved", C.c_int32),
                ("tol", C.c_double), ("shift", C.c_double)]


class ModalInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("block", C.c_int32), ("restarts", C.c_int32),
                ("fused_product", C.c_int32), ("pc_type", C.c_int32), ("residual_max", C.c_double),
                ("seconds_total", C.c_double), ("seconds_product", C.c_double), ("seconds_precond", C.c_double),
                ("seconds_gram", C.c_double), ("seconds_update", C.c_double), ("pc_setup_seconds", C.c_double)]


class BucklingOptions(C.Structure):
    _fields_ = [("n_modes", C.c_int32), ("guard", C.c_int32), ("max_it", C.c_int32), ("reserved", C.c_int32),
                ("tol", C.c_double), ("inner_rtol", C.c_double)]


class BucklingInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("block", C.c_int32), ("pc_type", C.c_int32),
                ("inner_iterations", C.c_int64), ("rho_max", C.c_double),
                ("seconds_total", C.c_double), ("seconds_solves", C.c_double), ("seconds_products", C.c_double),
                ("seconds_gram", C.c_double), ("seconds_update", C.c_double)]


class CaseInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("rel_residual", C.c_double)]


class CasesInfo(C.Structure):
    _fields_ = [("passes", C.c_int32), ("fused_product", C.c_int32), ("pc_type", C.c_int32), ("reserved", C.c_int32),
                ("solve_seconds", C.c_double), ("bytes_per_iteration", C.c_double)]


class EnvelopeInfo(C.Structure):
    _fields_ = [("seconds_cases", C.c_double), ("seconds_envelope", C.c_double), ("bytes_cases", C.c_double), ("bytes_envelope", C.c_double)]


class KrylovScalars(C.Structure):
    """femshell_krylov_scalars of include/femshell.h: the scalars of the recurrence as they lie in HBM (csrc/kernels.hpp CgScalars)"""
    _fields_ = [("rz", C.c_double), ("alpha", C.c_double), ("beta", C.c_double), ("rr", C.c_double), ("bb", C.c_double),
                ("tol2", C.c_double), ("red", C.c_double * 3), ("done", C.c_int32), ("iters", C.c_int32), ("ticket", C.c_uint32),
                ("pad", C.c_uint32), ("stage", (C.c_double * 64) * 3), ("ring_rz", C.c_double * 2), ("ring_alpha", C.c_double * 2),
                ("pass_xx", C.c_double), ("pass_rhs_rr", C.c_double), ("pass_rtol", C.c_double)]


# femshell_krylov_set / _get: the arrays, and femshell_krylov_launch: the steps (include/femshell.h)
KRYLOV_ARRAYS = {"x": 0, "r": 1, "z": 2, "p": 3, "q": 4, "sv": 5, "b": 6, "partials": 7, "scalars": 8, "history": 9, "history_cap": 10}
KRYLOV_STEPS = {"cg_init": 0, "cg_update": 1, "cg_direction": 2, "cgcg_init": 3, "cgcg_update": 4, "pcg_init": 5, "pcg_update": 6,
                "pcg_update_start": 7, "pcg_norm": 8, "pcg_dots": 9, "minv_apply_norm": 10, "product": 11, "sym_gather": 12,
                "two_dots": 13, "scalar_step": 14, "pc_apply": 15, "copy_z_to_p": 16}
CG_PHASES = {"none": 0, "init": 1, "alpha": 2, "beta": 3, "restart": 4, "fused_init": 5, "fused_step": 6, "flex_init": 7,
             "flex_rz0": 8, "flex_conv": 9, "flex_beta": 10, "flex_restart": 11, "flex_warm": 12}

PC_BLOCK_JACOBI, PC_AMG = 0, 1
CYCLE_V, CYCLE_K = 0, 1


def library_path():
    return os.path.join(_HERE, "libfemshell.so")


def build_library(force=False):
    """Compile csrc/ for gfx950 with hipcc (in-tree, so the .so travels with the repo)."""
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", _CSRC, "-s"])
    return library_path()


_lib = None


def load_library():
    """Loads libfemshell.so; raises if it has not been built (there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    host_only = os.environ.get("FEMSHELL_HOST_LIBRARY")
    if host_only:
        # sanitizer builds of the host-side code only (`make -C fem-shell_amd/csrc san`, tools/run_sanitizers.sh): they
        # export include/femshell_plan.h and femshell_last_error, nothing that touches a GPU
        L = C.CDLL(host_only)
        L.femshell_last_error.restype = C.c_char_p
        _lib = L
        return L
    path = library_path()
    if not os.path.exists(path):
        raise FemShellError(-2, "libfemshell.so is missing: build it with `make -C fem-shell_amd/csrc` "
                                "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(path)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    vp = C.c_void_p
    L.femshell_last_error.restype = C.c_char_p
    L.femshell_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.femshell_destroy.argtypes = [vp]
    L.femshell_set_mesh.argtypes = [vp, C.c_int32, dp, C.c_int32, ip, C.c_int32, ip]
    L.femshell_set_dirichlet.argtypes = [vp, C.c_int32, ip, bp]
    L.femshell_set_loads.argtypes = [vp, C.c_int32, ip, dp]
    L.femshell_set_sections.argtypes = [vp, C.c_int32, dp, ip, ip]
    L.femshell_assemble.argtypes = [vp]
    L.femshell_assemble_async.argtypes = [vp]
    L.femshell_solve.argtypes = [vp, C.c_double, C.c_int32, dp, C.POINTER(SolveInfo)]
    L.femshell_get_solution.argtypes = [vp, dp]
    L.femshell_residual_history.argtypes = [vp, dp, C.c_int32]
    L.femshell_residual_history.restype = C.c_int32
    L.femshell_element_matrices.argtypes = [vp, C.c_int32, C.c_int32, dp]
    L.femshell_nnz_blocks.argtypes = [vp]
    L.femshell_nnz_blocks.restype = C.c_int64
    L.femshell_export_bsr.argtypes = [vp, ip, ip, dp, dp]
    L.femshell_spmv.argtypes = [vp, dp, dp]
    L.femshell_residual.argtypes = [vp, dp, dp]
    L.femshell_row_begin.argtypes = [vp]
    L.femshell_row_begin.restype = C.c_int32
    L.femshell_row_end.argtypes = [vp]
    L.femshell_row_end.restype = C.c_int32
    L.femshell_set_initial_guess.argtypes = [vp, dp]
    L.femshell_owned_nodes.argtypes = [vp, C.POINTER(C.c_int32)]
    L.femshell_owned_nodes.restype = C.c_int32
    L.femshell_comm_unique_id.argtypes = [bp]
    L.femshell_comm_init.argtypes = [vp, bp]
    L.femshell_comm_ranks.argtypes = [vp]
    L.femshell_comm_ranks.restype = C.c_int32
    L.femshell_time_kernel.argtypes = [vp, C.c_int, C.c_int32, dp, dp]
    L.femshell_sync.argtypes = [vp]
    L.femshell_pc_defaults.argtypes = [C.c_int32, C.POINTER(PcOptions)]
    L.femshell_set_preconditioner.argtypes = [vp, C.POINTER(PcOptions)]
    L.femshell_amg_levels.argtypes = [vp]
    L.femshell_amg_levels.restype = C.c_int32
    L.femshell_amg_level.argtypes = [vp, C.c_int32, C.POINTER(AmgLevelInfo)]
    L.femshell_amg_export.argtypes = [vp, C.c_int32, C.c_int32, C.c_void_p]
    L.femshell_amg_export.restype = C.c_int64
    L.femshell_amg_setup_stats.argtypes = [vp, dp]
    L.femshell_amg_dense_stats.argtypes = [vp, dp]
    L.femshell_amg_patch_info.argtypes = [vp, dp]
    L.femshell_amg_symbolic_info.argtypes = [vp, ip]
    L.femshell_pc_apply.argtypes = [vp, dp, dp]
    L.femshell_amg_partition_info.argtypes = [vp, dp]
    L.femshell_assembly_kernel.argtypes = [vp]
    L.femshell_comm_selftest.argtypes = [vp, dp]
    L.femshell_comm_counters.argtypes = [vp, C.POINTER(C.c_int64), C.c_int32]
    L.femshell_comm_bytes.argtypes = [vp, C.POINTER(C.c_int64), C.c_int32]
    L.femshell_amg_cycle_bytes.argtypes = [vp, dp, C.c_int32]
    L.femshell_amg_cycle_bytes.restype = C.c_int32
    L.femshell_set_density.argtypes = [vp, C.c_double, C.c_int32, dp]
    L.femshell_lumped_mass.argtypes = [vp, dp]
    L.femshell_dynamics_defaults.argtypes = [C.POINTER(DynamicsOptions)]
    L.femshell_dynamics_begin.argtypes = [vp, C.POINTER(DynamicsOptions), dp, dp]
    L.femshell_dynamics_step.argtypes = [vp, C.c_double, C.c_int32, C.POINTER(SolveInfo)]
    L.femshell_dynamics_accept.argtypes = [vp]
    L.femshell_dynamics_state.argtypes = [vp, C.c_int32, dp, dp, dp]
    L.femshell_dynamics_energy.argtypes = [vp, C.c_int32, dp]
    L.femshell_dynamics_end.argtypes = [vp]
    L.femshell_modal_defaults.argtypes = [C.POINTER(ModalOptions)]
    L.femshell_modes.argtypes = [vp, C.POINTER(ModalOptions), dp, dp, dp, C.POINTER(ModalInfo)]
    L.femshell_spmm.argtypes = [vp, C.c_int32, dp, dp]
    L.femshell_modal_gram.argtypes = [vp, C.c_int32, dp, C.c_int32, dp, C.c_int32, dp]
    L.femshell_set_prescribed.argtypes = [vp, C.c_int32, ip, dp]
    L.femshell_reactions.argtypes = [vp, dp, dp]
    L.femshell_element_product.argtypes = [vp, dp, dp]
    L.femshell_element_resultants.argtypes = [vp, dp, dp]
    L.femshell_nodal_resultants.argtypes = [vp, dp, dp, dp]
    L.femshell_set_element_loads.argtypes = [vp, dp, dp]
    L.femshell_element_load_vector.argtypes = [vp, dp]
    L.femshell_set_expansion.argtypes = [vp, C.c_double, C.c_int32, dp]
    L.femshell_set_thermal.argtypes = [vp, dp, dp]
    L.femshell_thermal_load_vector.argtypes = [vp, dp]
    L.femshell_set_foundation.argtypes = [vp, dp, dp]
    L.femshell_set_springs.argtypes = [vp, C.c_int32, ip, dp]
    L.femshell_support_stiffness.argtypes = [vp, dp]
    L.femshell_support_forces.argtypes = [vp, dp, dp]
    L.femshell_geometric_product.argtypes = [vp, dp, C.c_int32, dp, dp]
    L.femshell_buckling_defaults.argtypes = [C.POINTER(BucklingOptions)]
    L.femshell_buckling.argtypes = [vp, C.POINTER(BucklingOptions), dp, dp, dp, dp, C.POINTER(BucklingInfo)]
    L.femshell_solve_cases.argtypes = [vp, C.c_int32, dp, C.c_double, C.c_int32, dp, C.POINTER(CaseInfo), C.POINTER(CasesInfo)]
    L.femshell_combination_envelope.argtypes = [vp, C.c_int32, dp, dp, C.c_int32, dp, dp, ip, C.POINTER(EnvelopeInfo)]
    L.femshell_pool_stats.argtypes = [dp]
    L.femshell_amg_device_dense_inverse.argtypes = [vp, C.c_int32, ip, ip, dp, C.c_int32, dp, dp]
    L.femshell_amg_dense_apply.argtypes = [vp, C.c_int32, C.c_int32, dp, C.c_int32, dp, dp]
    L.femshell_amg_device_block_jacobi.argtypes = [vp, C.c_int32, ip, ip, dp, C.c_int32, dp, ip]
    L.femshell_block_jacobi_export.argtypes = [vp, C.c_int32, C.c_int32, dp]
    L.femshell_block_jacobi_apply.argtypes = [vp, C.c_int32, C.c_int32, dp, dp]
    L.femshell_krylov_grid.argtypes = [vp]
    L.femshell_krylov_set.argtypes = [vp, C.c_int32, dp, C.c_int64]
    L.femshell_krylov_get.argtypes = [vp, C.c_int32, dp, C.c_int64]
    L.femshell_krylov_launch.argtypes = [vp, C.c_int32, ip, C.c_double, ip, dp]
    L.femshell_cg_reduce.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp, dp, C.POINTER(C.c_uint32)]
    i64p = C.POINTER(C.c_int64)
    L.femshell_modal_combine.argtypes = [vp, C.c_int32, ip, C.POINTER(dp), dp, C.c_int32, C.c_int32, dp, i64p]
    L.femshell_modal_residual.argtypes = [vp, C.c_int32, dp, dp, dp, C.c_int32, ip, dp, dp, dp, i64p]
    L.femshell_modal_block_jacobi.argtypes = [vp, C.c_int32, dp, dp, i64p]
    L.femshell_modal_mask.argtypes = [vp, C.c_int32, dp, i64p]
    L.femshell_modal_start.argtypes = [vp, C.c_int32, dp, i64p]
    for name in SYMBOLS:
        if name != "femshell_last_error" and not name.startswith("femshell_nnz") and \
                not name.startswith("femshell_row") and name != "femshell_residual_history" and \
                name not in ("femshell_amg_levels", "femshell_amg_export", "femshell_comm_ranks"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _b(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None


def _check(rc):
    if rc != 0:
        raise FemShellError(rc, load_library().femshell_last_error().decode())


def pool_stats():
    """The device pool of this process as it stands (csrc/dev_pool.hpp; no context needed): bytes the driver has handed out through
    the pool, bytes in use, bytes kept for reuse, arenas and the bytes in them, blocks waiting for the end of a multigrid setup."""
    out = np.zeros(6)
    _check(load_library().femshell_pool_stats(_d(out)))
    return {"outstanding": int(out[0]), "live": int(out[1]), "cached": int(out[2]), "arenas": int(out[3]),
            "arena_bytes": int(out[4]), "pending": int(out[5])}


def comm_unique_id():
    buf = np.zeros(128, dtype=np.uint8)
    _check(load_library().femshell_comm_unique_id(_b(buf)))
    return buf


class FemShell:
    """One context = one GPU = one rank of the row partition."""

    def __init__(self, nu, E, thickness, flags=REF_DEFAULT, device=-1, rank=0, world_size=1):
        self._L = load_library()
        self._h = C.c_void_p()
        cfg = Config(float(nu), float(E), float(thickness), int(flags), int(device), int(rank), int(world_size))
        _check(self._L.femshell_create(C.byref(cfg), C.byref(self._h)))
        self.n_nodes = 0
        self.n_tri = 0
        self.n_quad = 0

    def close(self):
        if self._h:
            self._L.femshell_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def comm_init(self, unique_id):
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.size == 128
        _check(self._L.femshell_comm_init(self._h, _b(uid)))

    def comm_ranks(self):
        return int(self._L.femshell_comm_ranks(self._h))

    def set_mesh(self, xyz, tri=None, quad=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        tri = np.zeros((0, 3), np.int32) if tri is None else np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        quad = np.zeros((0, 4), np.int32) if quad is None else np.ascontiguousarray(quad, dtype=np.int32).reshape(-1, 4)
        _check(self._L.femshell_set_mesh(self._h, len(xyz), _d(xyz), len(tri), _i(tri), len(quad), _i(quad)))
        self.n_nodes, self.n_tri, self.n_quad = len(xyz), len(tri), len(quad)

    def set_dirichlet(self, mask, node_ids=None):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        ids = None if node_ids is None else np.ascontiguousarray(node_ids, dtype=np.int32)
        _check(self._L.femshell_set_dirichlet(self._h, len(mask), _i(ids), _b(mask)))

    def set_loads(self, f6, node_ids=None):
        f6 = np.ascontiguousarray(f6, dtype=np.float64).reshape(-1, 6)
        ids = None if node_ids is None else np.ascontiguousarray(node_ids, dtype=np.int32)
        _check(self._L.femshell_set_loads(self._h, len(f6), _i(ids), _d(f6)))

    def set_prescribed(self, u6, node_ids=None):
        """Prescribed displacements (femshell_set_prescribed): u6 is (n, 6), one row per entry of node_ids or per node; only the
        entries at dofs the Dirichlet set fixes are used.  set_prescribed(None) (or an empty array) clears them."""
        if u6 is None:
            _check(self._L.femshell_set_prescribed(self._h, 0, None, None))
            return
        u6 = np.ascontiguousarray(u6, dtype=np.float64).reshape(-1, 6)
        ids = None if node_ids is None else np.ascontiguousarray(node_ids, dtype=np.int32)
        if ids is not None and len(ids) != len(u6):
            raise ValueError("u6 needs one row per entry of node_ids")
        _check(self._L.femshell_set_prescribed(self._h, len(u6), _i(ids), _d(u6)))

    def reactions(self, u=None):
        """r = K_unc u - loads, (n_nodes, 6): the support reactions at fixed dofs, the negative residual at free ones.  u None:
        the solution of the last solve, prescribed part included."""
        r = np.zeros((self.n_nodes, 6))
        _check(self._L.femshell_reactions(self._h, _d(self._node_vector(u, "u")), _d(r)))
        return r

    def element_product(self, x):
        """y = K_unc x: the matrix-free product with the unconstrained stiffness (femshell_element_product)."""
        x = self._node_vector(x, "x")
        y = np.zeros_like(x)
        _check(self._L.femshell_element_product(self._h, _d(x), _d(y)))
        return y

    def element_resultants(self, u=None):
        """What the shell carries, (n_tri + n_quad, 14), the triangles of set_mesh in their order, then the quadrilaterals: membrane
        force tensor N [0:6] and moment tensor M [6:12] in global axes (xx, yy, zz, xy, yz, zx), the von Mises stress at the top
        [12] and the bottom [13] surface -- the element means by the element's own quadrature (femshell_element_resultants).
        u None: the solution of the last solve, prescribed part included."""
        out = np.zeros((self.n_tri + self.n_quad, 14))
        _check(self._L.femshell_element_resultants(self._h, _d(self._node_vector(u, "u")), _d(out)))
        return out

    def nodal_resultants(self, u=None):
        """The element tensors averaged to the nodes and the Zienkiewicz-Zhu indicator of the difference (femshell_nodal_resultants):
        (nodes (n_nodes, 14), elems (n_tri + n_quad, 2)).  nodes: N* [0:6] and M* [6:12], the area-weighted averages of the rows of
        element_resultants over the elements at the node, W = sum A_e [12] and the fold measure 1 - |sum a_e| / W [13] (0 on a flat,
        consistently oriented neighbourhood: where it is not, the average of M means little).  elems: e2 [0], twice the complementary
        energy of the element means, and eta^2 [1], the energy of the difference between the recovered field and the element's own
        value; relative_error(elems) is the mesh's figure.  At folds and section changes the jump is physical and counts as error.
        u None: the solution of the last solve, prescribed part included."""
        nodes = np.zeros((self.n_nodes, 14))
        elems = np.zeros((self.n_tri + self.n_quad, 2))
        _check(self._L.femshell_nodal_resultants(self._h, _d(self._node_vector(u, "u")), _d(nodes), _d(elems)))
        return nodes, elems

    def set_element_loads(self, tri_load=None, quad_load=None):
        """Pressure and traction per element (femshell_set_element_loads): tri_load is (n_tri, 4), quad_load (n_quad, 4), rows
        (p, qx, qy, qz) in the element order of set_mesh -- p along the element's own normal, q per area in global axes.  None for
        one kind leaves it unloaded, both None clears.  The loads in force are the nodal loads of set_loads plus the lumped nodal
        equivalents; only the right-hand side is rebuilt."""
        tl = None if tri_load is None else np.ascontiguousarray(tri_load, dtype=np.float64).reshape(-1, 4)
        ql = None if quad_load is None else np.ascontiguousarray(quad_load, dtype=np.float64).reshape(-1, 4)
        if tl is not None and len(tl) != self.n_tri:
            raise ValueError("tri_load needs one row per triangle (%d), got %d" % (self.n_tri, len(tl)))
        if ql is not None and len(ql) != self.n_quad:
            raise ValueError("quad_load needs one row per quadrilateral (%d), got %d" % (self.n_quad, len(ql)))
        _check(self._L.femshell_set_element_loads(self._h, _d(tl), _d(ql)))

    def element_load_vector(self):
        """S, (n_nodes, 6): the nodal equivalents of the element loads in force alone, in the caller's numbering, not masked;
        zeros when none are set (femshell_element_load_vector)."""
        f = np.zeros((self.n_nodes, 6))
        _check(self._L.femshell_element_load_vector(self._h, _d(f)))
        return f

    def set_expansion(self, alpha, section_alpha=None):
        """Thermal expansion coefficient: one value for the whole shell, or section_alpha with one per section of set_sections
        (femshell_set_expansion).  set_sections forgets it, and the temperatures with it."""
        if section_alpha is None:
            _check(self._L.femshell_set_expansion(self._h, float(alpha), 0, None))
            return
        sa = np.ascontiguousarray(section_alpha, dtype=np.float64).ravel()
        _check(self._L.femshell_set_expansion(self._h, 0.0, len(sa), _d(sa)))

    def set_thermal(self, tri_temp=None, quad_temp=None):
        """Temperatures per element (femshell_set_thermal): tri_temp is (n_tri, 2), quad_temp (n_quad, 2), rows (Tm, Tg) in the
        element order of set_mesh -- Tm the temperature change of the mid-surface, Tg = T_top - T_bottom with the top at +t/2
        along the element's own normal.  None for one kind leaves it cold, both None clears.  The loads in force are
        (nodal + element loads) + the work-equivalent thermal loads; element_resultants, geometric_product and buckling see the
        stress state of the heated shell.  Needs set_expansion first."""
        tt = None if tri_temp is None else np.ascontiguousarray(tri_temp, dtype=np.float64).reshape(-1, 2)
        qt = None if quad_temp is None else np.ascontiguousarray(quad_temp, dtype=np.float64).reshape(-1, 2)
        if tt is not None and len(tt) != self.n_tri:
            raise ValueError("tri_temp needs one row per triangle (%d), got %d" % (self.n_tri, len(tt)))
        if qt is not None and len(qt) != self.n_quad:
            raise ValueError("quad_temp needs one row per quadrilateral (%d), got %d" % (self.n_quad, len(qt)))
        _check(self._L.femshell_set_thermal(self._h, _d(tt), _d(qt)))

    def thermal_load_vector(self):
        """T, (n_nodes, 6): the nodal equivalents of the temperatures in force alone, in the caller's numbering, not masked;
        zeros when none are set (femshell_thermal_load_vector)."""
        f = np.zeros((self.n_nodes, 6))
        _check(self._L.femshell_thermal_load_vector(self._h, _d(f)))
        return f

    def set_foundation(self, tri_k=None, quad_k=None):
        """Elastic foundation per element (femshell_set_foundation): tri_k is (n_tri, 2), quad_k (n_quad, 2), rows (kn, kt) >= 0 in
        the element order of set_mesh -- force per volume, kn along the element's own normal, kt in its plane.  None for one kind
        leaves it without a foundation, both None clears.  K in HBM is K + mask(K_sup) after the next assembly, which the next
        use makes."""
        tk = None if tri_k is None else np.ascontiguousarray(tri_k, dtype=np.float64).reshape(-1, 2)
        qk = None if quad_k is None else np.ascontiguousarray(quad_k, dtype=np.float64).reshape(-1, 2)
        if tk is not None and len(tk) != self.n_tri:
            raise ValueError("tri_k needs one row per triangle (%d), got %d" % (self.n_tri, len(tk)))
        if qk is not None and len(qk) != self.n_quad:
            raise ValueError("quad_k needs one row per quadrilateral (%d), got %d" % (self.n_quad, len(qk)))
        _check(self._L.femshell_set_foundation(self._h, _d(tk), _d(qk)))

    def set_springs(self, *args):
        """Nodal springs (femshell_set_springs): set_springs(k6) with one row (kx, ky, kz, krx, kry, krz) >= 0 per node, or
        set_springs(ids, k6) with one row per listed node (the others get none); global axes.  set_springs(None) (or an empty
        array) clears them."""
        if len(args) == 1:
            ids, k6 = None, args[0]
        elif len(args) == 2:
            ids, k6 = args
        else:
            raise TypeError("set_springs(k6) or set_springs(ids, k6)")
        if k6 is None:
            _check(self._L.femshell_set_springs(self._h, 0, None, None))
            return
        k6 = np.ascontiguousarray(k6, dtype=np.float64).reshape(-1, 6)
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if ids is not None and len(ids) != len(k6):
            raise ValueError("k6 needs one row per entry of ids (%d), got %d" % (len(ids), len(k6)))
        if ids is None and len(k6) not in (0, self.n_nodes):
            raise ValueError("k6 needs one row per node (%d), got %d" % (self.n_nodes, len(k6)))
        _check(self._L.femshell_set_springs(self._h, len(k6), _i(ids), _d(k6)))

    def support_stiffness(self):
        """The support table in force, (n_nodes, 9), in the caller's numbering, not masked: the summed foundation tensor (xx, yy,
        zz, xy, yz, zx) with the translational springs on its first three words, then the three rotational springs; zeros when
        nothing is set (femshell_support_stiffness)."""
        s = np.zeros((self.n_nodes, 9))
        _check(self._L.femshell_support_stiffness(self._h, _d(s)))
        return s

    def support_forces(self, u=None):
        """-K_sup u, (n_nodes, 6): the force and moment the elastic supports exert on the shell (femshell_support_forces).  u None:
        the solution of the last solve, prescribed part included."""
        f = np.zeros((self.n_nodes, 6))
        _check(self._L.femshell_support_forces(self._h, _d(self._node_vector(u, "u")), _d(f)))
        return f

    def set_sections(self, sections, tri_section=None, quad_section=None):
        """Shell sections: `sections` is an (n, 3) array-like of (nu, E, thickness), tri_section / quad_section give every
        triangle / quadrilateral of the mesh (in the order of set_mesh) its row of it.  set_sections(None) returns to the
        uniform material of the context.  K and the preconditioner are rebuilt at the next assemble / solve."""
        if sections is None:
            _check(self._L.femshell_set_sections(self._h, 0, None, None, None))
            return
        sec = np.ascontiguousarray(sections, dtype=np.float64).reshape(-1, 3)
        ts = None if tri_section is None else np.ascontiguousarray(tri_section, dtype=np.int32).ravel()
        qs = None if quad_section is None else np.ascontiguousarray(quad_section, dtype=np.int32).ravel()
        if ts is not None and len(ts) != self.n_tri:
            raise ValueError("tri_section needs one entry per triangle (%d), got %d" % (self.n_tri, len(ts)))
        if qs is not None and len(qs) != self.n_quad:
            raise ValueError("quad_section needs one entry per quadrilateral (%d), got %d" % (self.n_quad, len(qs)))
        _check(self._L.femshell_set_sections(self._h, len(sec), _d(sec), _i(ts), _i(qs)))

    def set_density(self, rho, section_rho=None):
        """Mass density: one value for the whole shell, or section_rho with one density per section of set_sections."""
        if section_rho is None:
            _check(self._L.femshell_set_density(self._h, float(rho), 0, None))
            return
        sr = np.ascontiguousarray(section_rho, dtype=np.float64).ravel()
        _check(self._L.femshell_set_density(self._h, 0.0, len(sr), _d(sr)))

    def lumped_mass(self):
        """The diagonal of the lumped mass matrix, (n_nodes, 6) in the caller's numbering (not masked by the Dirichlet set)."""
        m = np.zeros((self.n_nodes, 6))
        _check(self._L.femshell_lumped_mass(self._h, _d(m)))
        return m

    def _node_vector(self, x, name):
        if x is None:
            return None
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if len(x) != 6 * self.n_nodes:
            raise ValueError("%s needs n_nodes x 6 entries" % name)
        return x

    def dynamics_begin(self, dt, beta=0.25, gamma=0.5, alpha=0.0, u0=None, v0=None):
        """Newmark time stepping with damping alpha M from the state (u0, v0) (None: zero) under the loads in force; while it is
        active the matrix in HBM (export_bsr, spmv) is K + (a0 + alpha a1) M on the free dofs."""
        o = DynamicsOptions(float(dt), float(beta), float(gamma), float(alpha))
        _check(self._L.femshell_dynamics_begin(self._h, C.byref(o), _d(self._node_vector(u0, "u0")), _d(self._node_vector(v0, "v0"))))

    def dynamics_step(self, rtol=1e-10, max_it=10000):
        """One step from the committed state under the loads in force: the candidate state; returns the solve's info."""
        info = SolveInfo()
        _check(self._L.femshell_dynamics_step(self._h, float(rtol), int(max_it), C.byref(info)))
        return {f[0]: getattr(info, f[0]) for f in SolveInfo._fields_}

    def dynamics_accept(self):
        _check(self._L.femshell_dynamics_accept(self._h))

    def dynamics_state(self, candidate=False):
        """(u, v, a), each (n_nodes, 6), of the committed state or of the candidate of the last step."""
        u, v, a = (np.zeros((self.n_nodes, 6)) for _ in range(3))
        _check(self._L.femshell_dynamics_state(self._h, 1 if candidate else 0, _d(u), _d(v), _d(a)))
        return u, v, a

    def dynamics_energy(self, candidate=False):
        """(kinetic, strain) energy of the committed state or of the candidate."""
        out = np.zeros(2)
        _check(self._L.femshell_dynamics_energy(self._h, 1 if candidate else 0, _d(out)))
        return float(out[0]), float(out[1])

    def dynamics_end(self):
        _check(self._L.femshell_dynamics_end(self._h))

    def modes(self, n_modes, tol=1e-6, shift=0.0, guard=4, max_it=500, want_modes=True):
        """The n_modes lowest pairs of K x = lambda M x on the free dofs (femshell_modes; a density must be set): returns
        (lam[n_modes] ascending, modes (n_modes, n_nodes, 6) M-orthonormal or None, residuals[n_modes], info dict).  shift > 0
        solves with K + shift M (an unconstrained shell); lam comes back with the shift subtracted."""
        o = ModalOptions(int(n_modes), int(guard), int(max_it), 0, float(tol), float(shift))
        nm = max(int(n_modes), 0)
        lam = np.zeros(nm)
        res = np.zeros(nm)
        modes = np.zeros((nm, self.n_nodes, 6)) if want_modes else None
        info = ModalInfo()
        _check(self._L.femshell_modes(self._h, C.byref(o), _d(lam), _d(modes), _d(res), C.byref(info)))
        return lam, modes, res, {f[0]: getattr(info, f[0]) for f in ModalInfo._fields_}

    def spmm(self, X):
        """Y = K X for a block X of shape (n_cols, n_nodes * 6) (or (n_cols, n_nodes, 6)): femshell_spmm"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        shape = X.shape
        X = X.reshape(shape[0], -1)
        if X.shape[1] != 6 * self.n_nodes:
            raise ValueError("X needs n_nodes x 6 entries per column")
        Y = np.zeros_like(X)
        _check(self._L.femshell_spmm(self._h, X.shape[0], _d(X), _d(Y)))
        return Y.reshape(shape)

    def geometric_product(self, u, X):
        """Y = K_G(u) X, unconstrained: the geometric (initial-stress) stiffness of the membrane forces of u (u None: of the last
        solution, prescribed part included) times a block X of shape (n_cols, n_nodes * 6) or (n_cols, n_nodes, 6), or one vector
        of n_nodes x 6 entries: femshell_geometric_product"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        shape = X.shape
        X = X.reshape(1, -1) if X.size == 6 * self.n_nodes else X.reshape(shape[0], -1)
        if X.shape[1] != 6 * self.n_nodes:
            raise ValueError("X needs n_nodes x 6 entries per column")
        Y = np.zeros_like(X)
        _check(self._L.femshell_geometric_product(self._h, _d(self._node_vector(u, "u")), X.shape[0], _d(X), _d(Y)))
        return Y.reshape(shape)

    def buckling(self, n_modes=4, guard=4, tol=1e-8, max_it=100, u=None, inner_rtol=0.0, want_modes=True):
        """The n_modes load factors of smallest magnitude of (K + lambda K_G(u)) x = 0 on the free dofs, signed and ordered by
        |lambda| (femshell_buckling): returns (lam[n_modes], modes (n_modes, n_nodes, 6) each with its largest translational entry
        +1, or None, info dict with the convergence measures under "rho").  u None: the prestress of the last solution."""
        o = BucklingOptions(int(n_modes), int(guard), int(max_it), 0, float(tol), float(inner_rtol))
        nm = max(int(n_modes), 0)
        lam = np.zeros(nm)
        rho = np.zeros(nm)
        modes = np.zeros((nm, self.n_nodes, 6)) if want_modes else None
        info = BucklingInfo()
        _check(self._L.femshell_buckling(self._h, C.byref(o), _d(self._node_vector(u, "u")), _d(lam), _d(modes), _d(rho), C.byref(info)))
        d = {f[0]: getattr(info, f[0]) for f in BucklingInfo._fields_}
        d["rho"] = rho
        return lam, modes, d

    def solve_cases(self, loads, rtol=1e-10, max_it=10000):
        """Several load cases on the K of this context (femshell_solve_cases): loads is (n_cases, n_nodes, 6) or (n_cases,
        n_nodes * 6), or one vector of n_nodes x 6 entries; a case's vector is its whole load -- the context's own loads are not
        added, the Dirichlet set applies with zero values.  Returns (u (n_cases, n_nodes, 6), a list of per-case dicts with
        iterations, converged (1, 0, -1: breakdown) and rel_residual, an info dict).  Every case is bit for bit what it is when
        solved alone.  After a breakdown in a case the FemShellError carries u, cases and info as attributes."""
        loads = np.ascontiguousarray(loads, dtype=np.float64)
        n6 = 6 * self.n_nodes
        if loads.size == 0 or loads.size % n6 != 0:
            raise ValueError("loads needs n_nodes x 6 entries per case")
        loads = loads.reshape(-1, n6)
        n_cases = loads.shape[0]
        u = np.zeros((n_cases, self.n_nodes, 6))
        ci = (CaseInfo * n_cases)()
        info = CasesInfo()
        rc = self._L.femshell_solve_cases(self._h, n_cases, _d(loads), float(rtol), int(max_it), _d(u), ci, C.byref(info))
        cases = [{f[0]: getattr(ci[j], f[0]) for f in CaseInfo._fields_} for j in range(n_cases)]
        d = {f[0]: getattr(info, f[0]) for f in CasesInfo._fields_ if f[0] != "reserved"}
        if rc != 0:
            err = FemShellError(rc, load_library().femshell_last_error().decode())
            err.u, err.cases, err.info = u, cases, d
            raise err
        return u, cases, d

    def combination_envelope(self, u, factors, case_thermal=None):
        """The stress envelope of every element over load combinations (femshell_combination_envelope): u is (n_cases, n_nodes, 6)
        as solve_cases returns it (or one vector of n_nodes x 6 entries), factors (n_combos, n_cases) -- combination c is
        sum_j factors[c, j] (case j) --, case_thermal (n_cases,) the multiple of the free thermal state each case was loaded with
        (None: zeros).  Returns (env (n_elements, 6): max von Mises top and bottom, max N1, min N2, max M1, min M2 over the
        combinations; gov (n_elements, 6) int32: the lowest combination index, from 0, that attains each; an info dict).  Rows
        are the triangles of set_mesh in their order, then the quadrilaterals."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        n6 = 6 * self.n_nodes
        if u.size == 0 or n6 == 0 or u.size % n6 != 0:
            raise ValueError("u needs n_nodes x 6 entries per case")
        u = u.reshape(-1, n6)
        n_cases = u.shape[0]
        factors = np.ascontiguousarray(factors, dtype=np.float64)
        if factors.ndim == 1:
            factors = factors.reshape(1, -1)
        if factors.ndim != 2 or factors.shape[0] == 0 or factors.shape[1] != n_cases:
            raise ValueError("factors needs n_cases entries per combination")
        if case_thermal is not None:
            case_thermal = np.ascontiguousarray(case_thermal, dtype=np.float64).reshape(-1)
            if case_thermal.size != n_cases:
                raise ValueError("case_thermal needs one entry per case")
        ne = self.n_tri + self.n_quad
        env = np.zeros((ne, 6))
        gov = np.zeros((ne, 6), dtype=np.int32)
        info = EnvelopeInfo()
        _check(self._L.femshell_combination_envelope(self._h, n_cases, _d(u), _d(case_thermal), factors.shape[0], _d(factors), _d(env), _i(gov),
                                                     C.byref(info)))
        return env, gov, {f[0]: getattr(info, f[0]) for f in EnvelopeInfo._fields_}

    def modal_gram(self, A, B, weighted):
        """A^T diag(w) B by the Gram kernel of modes(): A (qa, n_nodes * 6), B (qb, n_nodes * 6), columns as rows of the arrays;
        weighted: w = the lumped mass, else 1.  Returns (qa, qb)."""
        A = np.ascontiguousarray(A, dtype=np.float64).reshape(len(A), -1)
        B = np.ascontiguousarray(B, dtype=np.float64).reshape(len(B), -1)
        if A.shape[1] != 6 * self.n_nodes or B.shape[1] != 6 * self.n_nodes:
            raise ValueError("A and B need n_nodes x 6 entries per column")
        G = np.zeros((len(A), len(B)))
        _check(self._L.femshell_modal_gram(self._h, len(A), _d(A), len(B), _d(B), 1 if weighted else 0, _d(G)))
        return G

    def assemble(self, wait=True):
        """wait=False: femshell_assemble_async -- enqueued only; sync(), solve() ... report a failed element."""
        _check(self._L.femshell_assemble(self._h) if wait else self._L.femshell_assemble_async(self._h))

    def solve(self, rtol=1e-10, max_it=10000, fetch=True):
        u = np.zeros((self.n_nodes, 6)) if fetch else None
        info = SolveInfo()
        _check(self._L.femshell_solve(self._h, float(rtol), int(max_it), _d(u), C.byref(info)))
        d = {f[0]: getattr(info, f[0]) for f in SolveInfo._fields_}
        return u, d

    def get_solution(self):
        u = np.zeros((self.n_nodes, 6))
        _check(self._L.femshell_get_solution(self._h, _d(u)))
        return u

    def residual_history(self, cap=1 << 20):
        h = np.zeros(cap)
        n = self._L.femshell_residual_history(self._h, _d(h), cap)
        return h[:n].copy()

    def element_matrices(self, first, count):
        size = 324 if first < self.n_tri else 576
        out = np.zeros((count, size))
        _check(self._L.femshell_element_matrices(self._h, int(first), int(count), _d(out)))
        n = 18 if size == 324 else 24
        return out.reshape(count, n, n)

    def nnz_blocks(self):
        return int(self._L.femshell_nnz_blocks(self._h))

    def export_bsr(self):
        nb = self.nnz_blocks()
        rowptr = np.zeros(self.n_nodes + 1, dtype=np.int32)
        colidx = np.zeros(nb, dtype=np.int32)
        vals = np.zeros((nb, 6, 6))
        F = np.zeros(6 * self.n_nodes)
        _check(self._L.femshell_export_bsr(self._h, _i(rowptr), _i(colidx), _d(vals), _d(F)))
        return rowptr, colidx, vals, F

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.zeros_like(x)
        _check(self._L.femshell_spmv(self._h, _d(x), _d(y)))
        return y

    def pc_apply(self, r):
        """z = M^-1 r, one application of the multigrid cycle (femshell_pc_apply): 6 values per node, the caller's numbering; on a
        row-partitioned context the rank's owned rows in the order of owned_nodes() (collective)."""
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
        if len(r) != 6 * int(self._L.femshell_owned_nodes(self._h, None)):
            raise ValueError("r needs 6 values per owned node")
        z = np.zeros_like(r)
        _check(self._L.femshell_pc_apply(self._h, _d(r), _d(z)))
        return z

    def residual(self, x):
        """F - K x with double-double products and row sums."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        r = np.zeros_like(x)
        _check(self._L.femshell_residual(self._h, _d(x), _d(r)))
        return r

    def row_range(self):
        return int(self._L.femshell_row_begin(self._h)), int(self._L.femshell_row_end(self._h))

    def set_initial_guess(self, u0=None):
        """The next solve starts from u0 (n_nodes x 6) -- None: from the previous solve's solution, where it lies in HBM."""
        if u0 is not None:
            u0 = np.ascontiguousarray(u0, dtype=np.float64).reshape(-1)
            if len(u0) != 6 * self.n_nodes:
                raise ValueError("u0 needs n_nodes x 6 entries")
        _check(self._L.femshell_set_initial_guess(self._h, _d(u0)))

    def owned_nodes(self):
        """the caller's ids of the node rows this rank owns, in the order export_bsr gives them"""
        n = int(self._L.femshell_owned_nodes(self._h, None))
        ids = np.zeros(n, dtype=np.int32)
        self._L.femshell_owned_nodes(self._h, _i(ids))
        return ids

    def time_kernel(self, which, reps=10):
        ms = C.c_double()
        by = C.c_double()
        _check(self._L.femshell_time_kernel(self._h, int(which), int(reps), C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def sync(self):
        _check(self._L.femshell_sync(self._h))

    def set_preconditioner(self, kind="amg", **options):
        """kind: "jacobi" (6x6 block-Jacobi, the default) or "amg" (smoothed-aggregation multigrid);
        options: cycle ("V"/"K"), smoother_degree, coarse_degree, coarsest_nodes, max_levels, refine_passes, eig_ratio."""
        o = PcOptions()
        _check(self._L.femshell_pc_defaults(PC_AMG if kind == "amg" else PC_BLOCK_JACOBI, C.byref(o)))
        for k, v in options.items():
            if k == "cycle":
                v = CYCLE_K if str(v).upper() == "K" else CYCLE_V
            if not hasattr(o, k):
                raise TypeError("unknown preconditioner option " + k)
            setattr(o, k, v)
        _check(self._L.femshell_set_preconditioner(self._h, C.byref(o)))

    def amg_levels(self):
        """Per-level facts of the multigrid hierarchy of the last solve (empty with block-Jacobi)."""
        out = []
        for l in range(self._L.femshell_amg_levels(self._h)):
            info = AmgLevelInfo()
            _check(self._L.femshell_amg_level(self._h, l, C.byref(info)))
            out.append({f[0]: getattr(info, f[0]) for f in AmgLevelInfo._fields_})
        return out

    def comm_bytes(self, clear=False):
        """(bytes handed to the sends of halo exchanges, bytes contributed to all-reduces and broadcasts) since the last clear"""
        out = (C.c_int64 * 2)()
        rc = self._L.femshell_comm_bytes(self._h, out, 1 if clear else 0)
        if rc < 0:
            _check(rc)
        return int(out[0]), int(out[1])

    def comm_counters(self, clear=False):
        """Communication enqueued since the counters were cleared (femshell_comm_counters)."""
        out = (C.c_int64 * 4)()
        rc = self._L.femshell_comm_counters(self._h, out, 1 if clear else 0)
        if rc < 0:
            _check(rc)
        return {"halo_exchanges_on_the_halo_stream": int(out[0]), "halo_exchanges_on_the_main_stream": int(out[1]),
                "allreduces": int(out[2]), "row_gathers": int(out[3])}

    def comm_selftest(self):
        """Microseconds of the three communication patterns femshell_comm_init checked on first contact (None: no communicator)."""
        out = np.zeros(3)
        rc = self._L.femshell_comm_selftest(self._h, _d(out))
        if rc < 0:
            _check(rc)
        return None if rc == 0 else {"halo_send_recv_on_second_stream_beside_allreduce_us": float(out[0]),
                                     "grouped_broadcast_row_gather_us": float(out[1]), "allreduce_3_words_us": float(out[2])}

    def amg_cycle_bytes(self):
        """Algorithmic HBM bytes of one multigrid cycle per level (femshell_amg_cycle_bytes)."""
        out = np.zeros(32)
        n = self._L.femshell_amg_cycle_bytes(self._h, _d(out), 32)
        if n < 0:
            _check(n)
        return out[:n].copy()

    def amg_setup_stats(self):
        """Device timings of the first coarsening step of the last multigrid setup."""
        out = np.zeros(7)
        _check(self._L.femshell_amg_setup_stats(self._h, _d(out)))
        return {"prolongator_ms": out[0], "ap_ms": out[1], "restriction_ms": out[2], "galerkin_ms": out[3],
                "galerkin_useful_flops": out[4], "galerkin_mfma_flops_issued": out[5], "galerkin_on_matrix_cores": bool(out[6])}

    def amg_symbolic_info(self):
        """Coarsening steps of the last setup by where their patterns were built."""
        out = np.zeros(3, dtype=np.int32)
        _check(self._L.femshell_amg_symbolic_info(self._h, _i(out)))
        return {"in_hbm": int(out[0]), "host_after_overflow": int(out[1]), "host_by_rule": int(out[2])}

    def assembly_kernel(self):
        """Name of the kernel femshell_assemble launches for this mesh."""
        k = self._L.femshell_assembly_kernel(self._h)
        if k < 0:
            _check(k)
        return "k_assemble_pipe" if k == 1 else "k_assemble"

    def amg_dense_stats(self):
        """The dense inverse of the coarsest operator when the matrix cores computed it (n = 0: host path)."""
        out = np.zeros(6)
        _check(self._L.femshell_amg_dense_stats(self._h, _d(out)))
        return {"n": int(out[0]), "ms": out[1], "mfma_flops_issued": out[2], "useful_flops": out[3], "dropped_directions": int(out[4]),
                "bytes": out[5]}

    def amg_device_dense_inverse(self, rowptr, colidx, vals, single_precision=False):
        """The device dense inverse (csrc/amg_dense.hip) of a caller's block CSR matrix, for tests: (inverse as doubles, stats as
        amg_dense_stats gives them).  The context's own hierarchy is not touched."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        n = 6 * (len(rowptr) - 1)
        inv, out = np.zeros((n, n)), np.zeros(6)
        _check(self._L.femshell_amg_device_dense_inverse(self._h, len(rowptr) - 1, _i(rowptr), _i(colidx), _d(vals),
                                                         1 if single_precision else 0, _d(inv), _d(out)))
        return inv, {"n": int(out[0]), "ms": out[1], "mfma_flops_issued": out[2], "useful_flops": out[3],
                     "dropped_directions": int(out[4]), "bytes": out[5]}

    def amg_dense_apply(self, inv, b, n_pad6, as_float=False, y_prefill=None):
        """One launch of k_dense_gemv_big on a caller's n x n inverse, for tests: y of n_pad6 + 8 doubles (prefilled by the
        caller, NaN by default) as the device left it."""
        inv = np.ascontiguousarray(inv, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        n = inv.shape[0]
        assert inv.shape == (n, n) and b.shape == (n,)
        y = np.full(n_pad6 + 8, np.nan) if y_prefill is None else np.array(y_prefill, dtype=np.float64)
        assert y.shape == (n_pad6 + 8,)
        _check(self._L.femshell_amg_dense_apply(self._h, n, int(n_pad6), _d(inv), 1 if as_float else 0, _d(b), _d(y)))
        return y

    def amg_device_block_jacobi(self, rowptr, colidx, vals, symmetric_storage=0):
        """The block-Jacobi setup kernel (k_block_jacobi) on a caller's block CSR matrix packed as a coarse level operator is, for
        tests: (inverse diagonal blocks [n, 6, 6], status word).  symmetric_storage 0: full; 1: diagonal + upper blocks; 2: the
        same, read as K's own diagonal slots are (upper triangle only).  The context's own state is not touched."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        n = len(rowptr) - 1
        inv, status = np.zeros((n, 6, 6)), np.zeros(1, dtype=np.int32)
        _check(self._L.femshell_amg_device_block_jacobi(self._h, n, _i(rowptr), _i(colidx), _d(vals), int(symmetric_storage), _d(inv),
                                                        _i(status)))
        return inv, int(status[0])

    def _block_jacobi_nodes(self, level):
        return self.n_nodes if level <= 0 or level >= self._L.femshell_amg_levels(self._h) else self.amg_levels()[level]["n_nodes"]

    def block_jacobi_export(self, level=0, single_precision=False):
        """The block-Jacobi inverse the context holds, [n, 6, 6]: level 0 of K (the caller's numbering), level >= 1 of that
        operator of the multigrid hierarchy; single_precision: the copy the smoothers read, widened."""
        if self._L.femshell_amg_levels(self._h) == 0 and level > 0:  # (builds what is missing, or refuses)
            _check(self._L.femshell_block_jacobi_export(self._h, 0, 0, _d(np.zeros((self.n_nodes, 6, 6)))))
        out = np.zeros((self._block_jacobi_nodes(level), 6, 6))
        _check(self._L.femshell_block_jacobi_export(self._h, int(level), 1 if single_precision else 0, _d(out)))
        return out

    def block_jacobi_apply(self, level, path, r):
        """z = D^-1 r over the padded vector of a level (6 x 32 x ceil(n / 32) doubles as they lie in HBM) by the lane-per-row
        reader (path 0) or the lane-per-node reader (path 1: the smoothers', from the single-precision copy where there is one)."""
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
        if self._L.femshell_amg_levels(self._h) == 0 and level > 0:
            _check(self._L.femshell_block_jacobi_export(self._h, 0, 0, _d(np.zeros((self.n_nodes, 6, 6)))))
        n_pad = (self._block_jacobi_nodes(level) + 31) // 32 * 32
        if len(r) != 6 * n_pad:
            raise ValueError("r needs 6 values per node of the padded level: %d" % (6 * n_pad))
        z = np.zeros_like(r)
        _check(self._L.femshell_block_jacobi_apply(self._h, int(level), int(path), _d(r), _d(z)))
        return z

    # ---- the Krylov loops launch by launch, for tests (femshell_krylov_*, csrc/api_krylov_probe.cpp)
    def krylov_grid(self):
        """workgroups of the per-slice kernels = partial sums per array"""
        return int(self._L.femshell_krylov_grid(self._h))

    def krylov_set(self, which, data):
        """Writes one array of the context's CG state (KRYLOV_ARRAYS): a vector as (n_nodes, 6) in the caller's numbering, the
        partial sums as raw words from the start, the scalars as a KrylovScalars, the history buffer (its length becomes the cap),
        "history_cap" as a number."""
        if isinstance(data, KrylovScalars):
            data = np.frombuffer(bytes(data), dtype=np.float64).copy()
        data = np.ascontiguousarray(np.atleast_1d(data), dtype=np.float64).reshape(-1)
        _check(self._L.femshell_krylov_set(self._h, KRYLOV_ARRAYS[which], _d(data), data.size))

    def krylov_get(self, which, n=None):
        """Reads one array of the CG state back: a vector as (n_nodes, 6), n words of the partial sums or of the history, the
        scalars as a KrylovScalars."""
        if which == "scalars":
            out = np.zeros(C.sizeof(KrylovScalars) // 8)
            _check(self._L.femshell_krylov_get(self._h, KRYLOV_ARRAYS[which], _d(out), out.size))
            return KrylovScalars.from_buffer_copy(out.tobytes())
        vector = KRYLOV_ARRAYS[which] <= KRYLOV_ARRAYS["b"]
        if not vector and which != "history_cap" and n is None:
            raise ValueError("krylov_get(%r) needs n, the number of words to read" % which)
        out = np.zeros(6 * self.n_nodes if vector else (1 if which == "history_cap" else int(n)))
        _check(self._L.femshell_krylov_get(self._h, KRYLOV_ARRAYS[which], _d(out), out.size))
        return out.reshape(-1, 6) if vector else (int(out[0]) if which == "history_cap" else out)

    def krylov_launch(self, step, *args, rtol=0.0):
        """One production launch of KRYLOV_STEPS on the CG state, synchronised.  Returns (n_partials the step reports -- 0: the
        grid --, the grid, the two sums of "two_dots")."""
        a = np.zeros(5, dtype=np.int32)
        a[:len(args)] = args
        iout, dout = np.zeros(2, dtype=np.int32), np.zeros(2)
        _check(self._L.femshell_krylov_launch(self._h, KRYLOV_STEPS[step], _i(a), float(rtol), _i(iout), _d(dout)))
        return int(iout[0]), int(iout[1]), dout

    def cg_reduce(self, partials, n_partials, nsums=1, len3=0):
        """The two-stage reduction (k_cg_scalar, reduce only) on the caller's arrays: nsums arrays of n_partials words one behind
        the other, the third len3 long.  Returns (red[3], the ticket behind the launch)."""
        partials = np.ascontiguousarray(partials, dtype=np.float64).reshape(-1)
        need = 2 * n_partials + len3 if nsums == 3 else nsums * n_partials
        if partials.size != need:
            raise ValueError("partials needs %d words" % need)
        red, ticket = np.zeros(3), C.c_uint32(12345)
        _check(self._L.femshell_cg_reduce(self._h, int(n_partials), int(nsums), int(len3), _d(partials), _d(red), C.byref(ticket)))
        return red, int(ticket.value)

    # ---- the block kernels of the eigen-solvers one launch at a time, for tests (femshell_modal_*, csrc/api_modal_probe.cpp)
    def _block(self, X, name):
        X = np.ascontiguousarray(X, dtype=np.float64)
        X = X.reshape(len(X), -1)
        if X.shape[1] != 6 * self.n_nodes:
            raise ValueError("%s needs n_nodes x 6 entries per column" % name)
        return X

    def modal_combine(self, sources, Cm, n_out):
        """Y = sum_k S_k C_k by k_block_combine: sources, up to three blocks (q_k, n_nodes * 6), None or empty for q_k = 0; Cm
        (sum q_k, ldc) with ldc >= n_out, the rows of source k behind those of source k - 1.  Returns (Y (n_out, n_nodes * 6),
        stray)."""
        S = [None if s is None or len(s) == 0 else self._block(s, "a source") for s in sources]
        q = np.array([0 if s is None else len(s) for s in S], dtype=np.int32)
        Cm = np.ascontiguousarray(Cm, dtype=np.float64)
        if Cm.ndim != 2 or Cm.shape[0] != int(q.sum()):
            raise ValueError("Cm needs one row per source column")
        ptrs = (C.POINTER(C.c_double) * 3)(*[_d(s) for s in S] + [None] * (3 - len(S)))
        Y = np.zeros((max(int(n_out), 0), 6 * self.n_nodes))
        stray = C.c_int64(-1)
        _check(self._L.femshell_modal_combine(self._h, len(S), _i(q), ptrs, _d(Cm), Cm.shape[1], int(n_out), _d(Y), C.byref(stray)))
        return Y, int(stray.value)

    def modal_residual(self, KX, X, theta, cols):
        """R_i = KX_c - theta[c] m o X_c, c = cols[i], by k_block_residual: KX, X (mb, n_nodes * 6), theta[mb].  Returns
        (R (n, n_nodes * 6), norms[n], partials (n, 128) as the kernel left them, stray)."""
        KX, X = self._block(KX, "KX"), self._block(X, "X")
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        if len(KX) != len(X) or len(theta) != len(X):
            raise ValueError("KX, X and theta need the same number of columns")
        n = len(cols)
        R, norms, partials = np.zeros((n, 6 * self.n_nodes)), np.zeros(n), np.zeros((n, 128))
        stray = C.c_int64(-1)
        _check(self._L.femshell_modal_residual(self._h, len(X), _d(KX), _d(X), _d(theta), n, _i(cols), _d(R), _d(norms), _d(partials),
                                               C.byref(stray)))
        return R, norms, partials, int(stray.value)

    def modal_block_jacobi(self, R):
        """Z = D^-1 R, masked, by k_block_bj: R (n, n_nodes * 6).  Returns (Z, stray)."""
        R = self._block(R, "R")
        Z = np.zeros_like(R)
        stray = C.c_int64(-1)
        _check(self._L.femshell_modal_block_jacobi(self._h, len(R), _d(R), _d(Z), C.byref(stray)))
        return Z, int(stray.value)

    def modal_mask(self, X):
        """mask(X) by k_block_mask: X (n, n_nodes * 6), left as it is.  Returns (the masked copy, stray)."""
        X = self._block(X, "X").copy()
        stray = C.c_int64(-1)
        _check(self._L.femshell_modal_mask(self._h, len(X), _d(X), C.byref(stray)))
        return X, int(stray.value)

    def modal_start(self, n_cols):
        """The start vectors of modes() by k_modal_init.  Returns (X (n_cols, n_nodes * 6), stray)."""
        X = np.zeros((max(int(n_cols), 0), 6 * self.n_nodes))
        stray = C.c_int64(-1)
        _check(self._L.femshell_modal_start(self._h, int(n_cols), _d(X), C.byref(stray)))
        return X, int(stray.value)

    def amg_patch_info(self):
        """The patch smoother of level 0 (csrc/amg_patch.hpp): rigid edges, clusters, nodes in them; all zero without rigid edges."""
        out = np.zeros(6)
        _check(self._L.femshell_amg_patch_info(self._h, _d(out)))
        return {"rigid_edges": int(out[0]), "clusters": int(out[1]), "nodes_in_clusters": int(out[2]), "not_positive_definite": int(out[3]),
                "tau": out[4], "max_nodes": int(out[5])}

    def amg_partition_info(self):
        """Row-partitioned hierarchy (femshell_amg_partition_info): levels split over the ranks, bytes that shrink with the
        rank count, bytes every rank holds in full."""
        out = np.zeros(6)
        _check(self._L.femshell_amg_partition_info(self._h, _d(out)))
        return {"partitioned_levels": int(out[0]), "bytes_partitioned": out[1], "bytes_replicated": out[2],
                "rows_on_last_partitioned_level": int(out[3]), "ghost_rows_on_last_partitioned_level": int(out[4]),
                "nodes_of_first_replicated_level": int(out[5])}

    def amg_export(self, level):
        """Host copies of a level (small problems): dict with agg, A (rowptr, cols, vals), P (rowptr, cols, vals)."""
        names = {"agg": (0, np.int32), "A_rowptr": (1, np.int64), "A_cols": (2, np.int32), "A_vals": (3, np.float64),
                 "P_rowptr": (4, np.int64), "P_cols": (5, np.int32), "P_vals": (6, np.float64),
                 "coarse_inverse": (7, np.float64),  # (the coarsest level only: its dense inverse, n x n)
                 "patch_labels": (8, np.int32)}      # (level 0: cluster of every node or -1; None without clusters)
        out = {}
        for name, (which, dt) in names.items():
            n = self._L.femshell_amg_export(self._h, level, which, None)
            if n < 0:
                out[name] = None
                continue
            a = np.zeros(n, dtype=dt)
            if n:
                self._L.femshell_amg_export(self._h, level, which, a.ctypes.data_as(C.c_void_p))
            out[name] = a.reshape(-1, 6, 6) if name.endswith("vals") else (a.reshape(int(round(np.sqrt(n))), -1) if name == "coarse_inverse" else a)
        return out


# ---- host-only plan inspection (include/femshell_plan.h); needs no GPU -----------------------

PLAN_INFO = ["n_own", "n_pad", "n_ghost", "n_slices", "n_ltri", "n_lquad", "total_slots", "n_pairs",
             "n_peers", "row_begin", "row_end", "nnz_blocks", "n_interior_slices", "n_items",
             "n_multi_round_slices", "max_slice_elems", "max_slice_width", "symmetric", "stored_blocks", "pipe"]
PLAN_ARRAYS = {
    "ghost_global": (0, np.int32), "tri_local": (1, np.int32), "tri_global_id": (2, np.int32),
    "quad_local": (3, np.int32), "quad_global_id": (4, np.int32), "slice_width": (5, np.int32),
    "slice_base": (6, np.int64), "cols": (7, np.int32), "pair_ptr": (8, np.int32), "pairs": (9, np.uint32),
    "xyz_local": (10, np.float64), "peer_ranks": (11, np.int32), "peer_recv_offset": (12, np.int32),
    "peer_recv_count": (13, np.int32), "peer_send_ptr": (14, np.int32), "peer_send_nodes": (15, np.int32),
    "spmv_order": (16, np.int32), "in_width": (17, np.int32), "in_base": (18, np.int64), "in_slots": (19, np.int32),
    "gat_slots": (20, np.int32), "loc_list": (21, np.uint8), "loc_index": (22, np.uint8),
    "item_ptr": (23, np.int32), "items": (24, np.uint32), "pairs16": (25, np.uint16), "slice_elem_ptr": (26, np.int32),
}


def build_plan(xyz, tri=None, quad=None, rank=0, world_size=1):
    """Returns the symbolic plan of one rank as a dict of numpy arrays (CPU only)."""
    L = load_library()
    L.femshell_plan_create.argtypes = [C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32),
                                       C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                       C.POINTER(C.c_void_p)]
    L.femshell_plan_create.restype = C.c_int
    L.femshell_plan_destroy.argtypes = [C.c_void_p]
    L.femshell_plan_destroy.restype = None
    L.femshell_plan_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.femshell_plan_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.femshell_plan_array.restype = C.c_int64
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    tri = np.zeros((0, 3), np.int32) if tri is None else np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    quad = np.zeros((0, 4), np.int32) if quad is None else np.ascontiguousarray(quad, dtype=np.int32).reshape(-1, 4)
    h = C.c_void_p()
    _check(L.femshell_plan_create(len(xyz), _d(xyz), len(tri), _i(tri), len(quad), _i(quad), rank, world_size,
                                  C.byref(h)))
    try:
        info = np.zeros(len(PLAN_INFO), dtype=np.int64)
        _check(L.femshell_plan_info(h, info.ctypes.data_as(C.POINTER(C.c_int64))))
        out = {k: int(v) for k, v in zip(PLAN_INFO, info)}
        for name, (which, dt) in PLAN_ARRAYS.items():
            n = L.femshell_plan_array(h, which, None)
            a = np.zeros(n, dtype=dt)
            if n:
                L.femshell_plan_array(h, which, a.ctypes.data_as(C.c_void_p))
            out[name] = a
    finally:
        L.femshell_plan_destroy(h)
    return out


def plan_node_normals(xyz, tri=None, quad=None, from_gather_lists=True, rank=0, world_size=1):
    """Unit normals of the owned nodes of one rank's plan (CPU only): by the walk over all elements or from the gather lists."""
    L = load_library()
    L.femshell_plan_create.argtypes = [C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32),
                                       C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                       C.POINTER(C.c_void_p)]
    L.femshell_plan_create.restype = C.c_int
    L.femshell_plan_destroy.argtypes = [C.c_void_p]
    L.femshell_plan_destroy.restype = None
    L.femshell_plan_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.femshell_plan_node_normals.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    L.femshell_plan_node_normals.restype = C.c_int
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    tri = np.zeros((0, 3), np.int32) if tri is None else np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    quad = np.zeros((0, 4), np.int32) if quad is None else np.ascontiguousarray(quad, dtype=np.int32).reshape(-1, 4)
    h = C.c_void_p()
    _check(L.femshell_plan_create(len(xyz), _d(xyz), len(tri), _i(tri), len(quad), _i(quad), rank, world_size, C.byref(h)))
    try:
        info = np.zeros(len(PLAN_INFO), dtype=np.int64)
        _check(L.femshell_plan_info(h, info.ctypes.data_as(C.POINTER(C.c_int64))))
        out = np.zeros((int(info[PLAN_INFO.index("n_own")]), 3))
        _check(L.femshell_plan_node_normals(h, 1 if from_gather_lists else 0, _d(out)))
    finally:
        L.femshell_plan_destroy(h)
    return out


# ---- host-only pieces of the multigrid setup (include/femshell_plan.h); need no GPU --------------------------

COARSEN_ARRAYS = {"agg": (0, np.int32), "P_rowptr": (1, np.int64), "P_cols": (2, np.int32), "P_vals": (3, np.float64),
                  "Ac_rowptr": (4, np.int64), "Ac_cols": (5, np.int32), "Ac_vals": (6, np.float64), "Bc": (7, np.float64)}


def amg_host_rbm(xyz, dmask=None):
    L = load_library()
    L.femshell_amg_host_rbm.argtypes = [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_double)]
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    dm = None if dmask is None else np.ascontiguousarray(dmask, dtype=np.uint8)
    B = np.zeros((len(xyz), 6, 6))
    _check(L.femshell_amg_host_rbm(len(xyz), _d(xyz), _b(dm), _d(B)))
    return B


def amg_host_coarsen(rowptr, colidx, vals, B, lambda_max):
    """One coarsening step of the library's host setup: dict with agg, P (BSR arrays), Ac (BSR arrays), Bc."""
    L = load_library()
    L.femshell_amg_host_coarsen.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_void_p)]
    L.femshell_amg_coarsening_destroy.argtypes = [C.c_void_p]
    L.femshell_amg_coarsening_destroy.restype = None
    L.femshell_amg_coarsening_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.femshell_amg_coarsening_array.restype = C.c_int64
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    h = C.c_void_p()
    _check(L.femshell_amg_host_coarsen(len(rowptr) - 1, _i(rowptr), _i(colidx), _d(vals), _d(B), float(lambda_max), C.byref(h)))
    try:
        out = {}
        for name, (which, dt) in COARSEN_ARRAYS.items():
            n = L.femshell_amg_coarsening_array(h, which, None)
            a = np.zeros(n, dtype=dt)
            if n:
                L.femshell_amg_coarsening_array(h, which, a.ctypes.data_as(C.c_void_p))
            out[name] = a
    finally:
        L.femshell_amg_coarsening_destroy(h)
    out["P_vals"] = out["P_vals"].reshape(-1, 6, 6)
    out["Ac_vals"] = out["Ac_vals"].reshape(-1, 6, 6)
    out["Bc"] = out["Bc"].reshape(-1, 6, 6)
    return out


def amg_host_aggregate(rowptr, colidx, visit=None):
    """The library's greedy aggregation of a node graph: (agg, n_aggregates); visit = order of the passes (optional)."""
    L = load_library()
    L.femshell_amg_host_aggregate.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32)]
    L.femshell_amg_host_aggregate.restype = C.c_int32
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    agg = np.zeros(len(rowptr) - 1, dtype=np.int32)
    v = None if visit is None else np.ascontiguousarray(visit, dtype=np.int32)
    na = L.femshell_amg_host_aggregate(len(rowptr) - 1, _i(rowptr), _i(colidx), None if v is None else _i(v), _i(agg))
    if na < 0:
        _check(-1)  # FEMSHELL_ERR_INVALID; the message is in femshell_last_error
    return agg, na


def amg_host_patch_clusters(rowptr, colidx, vals, tau=0.8, max_nodes=8):
    """Clusters of rigidly coupled nodes of a host matrix (csrc/amg_patch.hpp): (labels, n_clusters, rigid edges)."""
    L = load_library()
    L.femshell_amg_host_patch_clusters.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_double,
                                                   C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.femshell_amg_host_patch_clusters.restype = C.c_int32
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    labels = np.zeros(len(rowptr) - 1, dtype=np.int32)
    edges = C.c_int64(0)
    nc = L.femshell_amg_host_patch_clusters(len(rowptr) - 1, _i(rowptr), _i(colidx), _d(vals), tau, max_nodes, _i(labels), C.byref(edges))
    if nc < 0:
        _check(-1)
    return labels, nc, edges.value


def amg_host_aggregate_glued(rowptr, colidx, labels, visit=None):
    """The aggregation with the clusters glued into one node each: (agg, n_aggregates)."""
    L = load_library()
    L.femshell_amg_host_aggregate_glued.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.femshell_amg_host_aggregate_glued.restype = C.c_int32
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    agg = np.zeros(len(rowptr) - 1, dtype=np.int32)
    v = None if visit is None else np.ascontiguousarray(visit, dtype=np.int32)
    na = L.femshell_amg_host_aggregate_glued(len(rowptr) - 1, _i(rowptr), _i(colidx), _i(labels), None if v is None else _i(v), _i(agg))
    if na < 0:
        _check(-1)
    return agg, na


def amg_host_dense_inverse(rowptr, colidx, vals):
    L = load_library()
    L.femshell_amg_host_dense_inverse.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double)]
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    n = 6 * (len(rowptr) - 1)
    inv = np.zeros((n, n))
    _check(L.femshell_amg_host_dense_inverse(len(rowptr) - 1, _i(rowptr), _i(colidx), _d(vals), _d(inv)))
    return inv


def amg_host_block_inverse(blocks):
    """The host's 6 x 6 block-Jacobi inverse (block_diagonal_inverse) of [n, 6, 6] blocks: (inverses [n, 6, 6], ok [n]: 1 =
    inverted, 0 = not positive definite and the identity returned)."""
    L = load_library()
    L.femshell_amg_host_block_inverse.argtypes = [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.femshell_amg_host_block_inverse.restype = C.c_int32
    blocks = np.ascontiguousarray(blocks, dtype=np.float64).reshape(-1, 6, 6)
    inv, ok = np.zeros_like(blocks), np.zeros(len(blocks), dtype=np.int32)
    _check(L.femshell_amg_host_block_inverse(len(blocks), _d(blocks), _d(inv), _i(ok)))
    return inv, ok


def amg_host_dense_tile_map(nt):
    """Super-block lists of the device dense inverse's trailing update for nt tiles per side: int32 array [8, per_xcd] of
    (I << 16) | J, -1 = none."""
    L = load_library()
    L.femshell_amg_host_dense_tile_map.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    L.femshell_amg_host_dense_tile_map.restype = C.c_int32
    per = L.femshell_amg_host_dense_tile_map(int(nt), None, 0)
    if per < 0:
        raise ValueError("femshell_amg_host_dense_tile_map: invalid nt")
    out = np.full((8, per), -1, dtype=np.int32)
    L.femshell_amg_host_dense_tile_map(int(nt), _i(out), out.size)
    return out


def amg_host_pack(rowptr, colidx, vals, diag_first):
    """Sliced block ELL image of a BSR matrix: (slice_width, slice_base, cols, ell_vals)."""
    L = load_library()
    L.femshell_amg_host_pack.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.femshell_amg_host_pack.restype = C.c_int64
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    n = len(rowptr) - 1
    total = L.femshell_amg_host_pack(n, _i(rowptr), _i(colidx), _d(vals), int(diag_first), None, None, None, None)
    ns = (n + 31) // 32
    sw = np.zeros(ns, dtype=np.int32)
    sb = np.zeros(ns + 1, dtype=np.int64)
    cols = np.zeros(total, dtype=np.int32)
    ev = np.zeros(total * 36)
    L.femshell_amg_host_pack(n, _i(rowptr), _i(colidx), _d(vals), int(diag_first), _i(sw),
                             sb.ctypes.data_as(C.POINTER(C.c_int64)), _i(cols), _d(ev))
    return sw, sb, cols, ev


def amg_host_pack_sym(rowptr, colidx, vals):
    """Symmetric-storage image of a square BSR matrix: dict of the ELL arrays and the in-lists."""
    L = load_library()
    i32, i64, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    L.femshell_amg_host_pack_sym.argtypes = [C.c_int32, i32, i32, dbl, i32, i64, i32, dbl, i32, i64, i32, i32, i64]
    L.femshell_amg_host_pack_sym.restype = C.c_int64
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    n = len(rowptr) - 1
    in_total = C.c_int64()
    total = L.femshell_amg_host_pack_sym(n, _i(rowptr), _i(colidx), _d(vals), None, None, None, None, None, None, None, None,
                                         C.byref(in_total))
    ns = (n + 31) // 32
    out = {"slice_width": np.zeros(ns, np.int32), "slice_base": np.zeros(ns + 1, np.int64), "cols": np.zeros(total, np.int32),
           "vals": np.zeros(total * 36), "in_width": np.zeros(ns, np.int32), "in_base": np.zeros(ns + 1, np.int64),
           "in_slots": np.zeros(in_total.value, np.int32), "in_rows": np.zeros(in_total.value, np.int32)}
    p64 = lambda a: a.ctypes.data_as(i64)  # noqa: E731
    L.femshell_amg_host_pack_sym(n, _i(rowptr), _i(colidx), _d(vals), _i(out["slice_width"]), p64(out["slice_base"]),
                                 _i(out["cols"]), _d(out["vals"]), _i(out["in_width"]), p64(out["in_base"]),
                                 _i(out["in_slots"]), _i(out["in_rows"]), C.byref(in_total))
    return out


def reorder_host(kind, xyz, tri=None, quad=None):
    """perm[new index] = caller's node id of the library's optional renumbering ("morton" or "rcm")."""
    L = load_library()
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    L.femshell_reorder_host.argtypes = [C.c_int32, C.c_int32, dbl, C.c_int32, i32, C.c_int32, i32, i32]
    L.femshell_reorder_host.restype = C.c_int
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    tri = np.zeros((0, 3), np.int32) if tri is None else np.ascontiguousarray(tri, dtype=np.int32)
    quad = np.zeros((0, 4), np.int32) if quad is None else np.ascontiguousarray(quad, dtype=np.int32)
    perm = np.zeros(len(xyz), np.int32)
    rc = L.femshell_reorder_host({"morton": 0, "rcm": 1}[kind], len(xyz), _d(xyz), len(tri), _i(tri) if len(tri) else None,
                                 len(quad), _i(quad) if len(quad) else None, _i(perm))
    if rc:
        raise FemShellError(-1, "femshell_reorder_host: invalid mesh")
    return perm


def grid_cap(text, fallback):
    """The workgroup cap the library takes from the text of a grid knob (femshell_grid_cap; text None: not set).  CPU only."""
    L = load_library()
    L.femshell_grid_cap.argtypes = [C.c_char_p, C.c_int32]
    L.femshell_grid_cap.restype = C.c_int32
    return int(L.femshell_grid_cap(None if text is None else str(text).encode(), int(fallback)))


def knob_long(name, default):
    """The number the library reads from the environment variable `name` (femshell_knob_long; unset: default).  CPU only."""
    L = load_library()
    L.femshell_knob_long.argtypes = [C.c_char_p, C.c_long]
    L.femshell_knob_long.restype = C.c_long
    return int(L.femshell_knob_long(str(name).encode(), int(default)))


def knob_flag(name, default):
    """The switch the library reads from the environment variable `name` (femshell_knob_flag; unset: default).  CPU only."""
    L = load_library()
    L.femshell_knob_flag.argtypes = [C.c_char_p, C.c_int]
    L.femshell_knob_flag.restype = C.c_int
    return bool(L.femshell_knob_flag(str(name).encode(), int(bool(default))))


# the derived products of a context and the changes that make them stale, in the order of csrc/derived.hpp
DERIVED_PRODUCTS = ["K", "F", "Jacobi", "Hierarchy", "Mass", "Ubar", "Solution", "WarmStart", "Fp64Only"]
STATE_CHANGES = ["mesh", "dirichlet", "sections", "sections_cleared_none_set", "loads", "prescribed", "density", "pc_options",
                 "assembled", "matrix_shifted", "dynamics_begin", "matrix_spoiled", "dynamics_end", "fp64_fallback", "krylov_probe"]


def stale_after(change):
    """The derived products of a context (names of DERIVED_PRODUCTS, a frozenset) that the change `change` (a name of
    STATE_CHANGES, or its number) makes stale (femshell_stale_after).  CPU only."""
    L = load_library()
    L.femshell_stale_after.argtypes = [C.c_int32]
    L.femshell_stale_after.restype = C.c_int32
    mask = int(L.femshell_stale_after(STATE_CHANGES.index(change) if isinstance(change, str) else int(change)))
    if mask < 0:
        raise FemShellError(-1, "femshell_stale_after: no such change")
    assert mask >> len(DERIVED_PRODUCTS) == 0
    return frozenset(name for bit, name in enumerate(DERIVED_PRODUCTS) if mask >> bit & 1)
