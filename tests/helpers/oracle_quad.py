"""ctypes binding of the quad-precision build of the oracle's element path (oracle/libfemshell_oracle_quad.so,
`make -C oracle quad`: femshell_oracle.c with __float128 as its arithmetic type, gcc + libquadmath).

Test infrastructure of the CPU tests and of tools/gen_golden_truth.py only.  Inputs are doubles (exact in binary128), every
result is the binary128 value rounded once to double.  GPU tests never load this: they read tests/golden/element_truth.npz.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers.oracle import ORACLE_DIR, Material, Tri3Parts, _d

QUAD_LIB_PATH = os.path.join(ORACLE_DIR, "libfemshell_oracle_quad.so")
_lib = None


def build():
    """(Re)build the quad library if it is missing or older than one of its sources."""
    srcs = [os.path.join(ORACLE_DIR, f) for f in ("femshell_oracle_quad.c", "femshell_oracle.c", "femshell_oracle.h")]
    if (not os.path.exists(QUAD_LIB_PATH)) or os.path.getmtime(QUAD_LIB_PATH) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s", "quad"])


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(QUAD_LIB_PATH)
        dp = C.POINTER(C.c_double)
        L.fsoq_material_matrices.argtypes = [C.POINTER(Material), dp, dp]
        L.fsoq_material_matrices.restype = None
        L.fsoq_element_tri3.argtypes = [dp, C.POINTER(Material), dp, C.POINTER(Tri3Parts)]
        L.fsoq_element_tri3.restype = C.c_int
        L.fsoq_element_quad4.argtypes = [dp, C.POINTER(Material), dp, dp, dp, dp, dp]
        L.fsoq_element_quad4.restype = C.c_int
        _lib = L
    return _lib


def material_matrices(mat):
    Dm = np.zeros(9)
    Dp = np.zeros(9)
    lib().fsoq_material_matrices(C.byref(mat), _d(Dm), _d(Dp))
    return Dm.reshape(3, 3), Dp.reshape(3, 3)


def element_tri3(xyz, mat):
    """xyz: (3,3).  Returns Ke (18,18), variable-major, and the parts of oracle.element_tri3(want_parts=True)."""
    X = np.ascontiguousarray(xyz, dtype=np.float64).reshape(9)
    Ke = np.zeros(324)
    parts = Tri3Parts()
    if lib().fsoq_element_tri3(_d(X), C.byref(mat), _d(Ke), C.byref(parts)):
        raise ValueError("degenerate TRI3 element")
    p = {
        "trafo": np.array(parts.trafo).reshape(3, 3),
        "transUV": np.array(parts.transUV).reshape(3, 2),
        "dphi": np.array(parts.dphi).reshape(3, 2),
        "area": parts.area,
        "Ke_m": np.array(parts.Ke_m).reshape(6, 6),
        "Ke_p": np.array(parts.Ke_p).reshape(9, 9),
        "K_local": np.array(parts.K_local).reshape(18, 18),
        "K_global_nm": np.array(parts.K_global_nm).reshape(18, 18),
    }
    return Ke.reshape(18, 18), p


def element_quad4(xyz, mat):
    """xyz: (4,3).  Returns Ke (24,24), variable-major, and Ke_m, Ke_p, K_global_nm and the frame (rows = local axes)."""
    X = np.ascontiguousarray(xyz, dtype=np.float64).reshape(12)
    Ke, Km, Kp, Kg, T = np.zeros(576), np.zeros(64), np.zeros(144), np.zeros(576), np.zeros(9)
    if lib().fsoq_element_quad4(_d(X), C.byref(mat), _d(Ke), _d(Km), _d(Kp), _d(Kg), _d(T)):
        raise ValueError("degenerate QUAD4 element")
    return Ke.reshape(24, 24), {"Ke_m": Km.reshape(8, 8), "Ke_p": Kp.reshape(12, 12),
                                "K_global_nm": Kg.reshape(24, 24), "trafo": T.reshape(3, 3)}
