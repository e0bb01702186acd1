"""The reference of the load combinations (tests/helpers/envelope.py) held to itself on the CPU: its two routes agree
within the bound the device is judged by, the checker catches planted defects, and the bitwise consequences of the definition hold
in float64."""
import functools

import numpy as np
import pytest

from tests.helpers import envelope as ev, meshes, prescribed as pr, resultants as rs, thermal as th

N_CASES, N_COMBOS = 5, 7
ALPHA = 1.2e-5


def _factors(n_combos=N_COMBOS, n_cases=N_CASES, seed=21):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (n_combos, n_cases))


def _cases(n_nodes, n_cases=N_CASES):
    return np.array([rs.random_u(n_nodes, seed=30 + j) for j in range(n_cases)])


MESHES = {
    "strip33": lambda: pr.strip33() + (None,),
    "mixed_petals24": lambda: meshes.mixed_petals(24),
    "one_quadrilateral": lambda: rs.device_meshes()["one_quadrilateral"]()[:3],
}


@functools.lru_cache(maxsize=None)
def _petals():
    """mixed_petals24 with temperatures in force and case 0 loaded with them: (xyz, tri, quad, u, tau, thermal, G, S, t)"""
    xyz, tri, quad = meshes.mixed_petals(24)
    u = _cases(len(xyz))
    tt, qt = th.random_temps(len(tri), len(quad))
    thermal = {"tri_temp": tt, "quad_temp": qt, "alpha": ALPHA}
    tau = np.array([1.0, 0.0, 0.0, 0.0, 0.0])
    G, S = ev.case_rows(xyz, tri, quad, u, tau, thermal=thermal)
    return xyz, tri, quad, u, tau, thermal, G, S, ev.element_thickness(len(tri), len(quad))


@pytest.mark.parametrize("name", list(MESHES))
def test_the_two_routes_of_the_reference_agree(name):
    """rows of the combined vector against combined rows, and the frame-free von Mises and principal values against the local
    form: mesh_resultants of u_c = sum_j f_cj u_j gives words 12 and 13 in the element frame and the tensors whose eigenvalues the
    principal values are; the restatement combines the cases' global words.  Both within 1e-12 S_c."""
    xyz, tri, quad = MESHES[name]()
    u, f = _cases(len(xyz)), _factors()
    ref = ev.reference(xyz, tri, quad, u, f)
    worst = 0.0
    for c in range(N_COMBOS):
        uc = np.tensordot(f[c], u, axes=1)
        out, _ = rs.mesh_resultants(xyz, tri, quad, uc, rs.NU, rs.E, rs.T)
        pn, pm = ev.principal_free(out[:, :6]), ev.principal_free(out[:, 6:12])
        direct = np.stack([out[:, 12], out[:, 13], pn[:, 0], pn[:, 1], pm[:, 0], pm[:, 1]], axis=1)
        worst = max(worst, rs.bound_ratio(ref.q[c], direct, ref.S[c]))
    print("envelope reference, two routes on %-18s max difference / (1e-12 S_c) = %.3e" % (name, worst))
    assert worst <= 1.0
    assert ev.check(ref.env, ref.gov, ref) == 0.0


# ------------------------------------------------------------------ planted defects

def _defective(kind, G, S, factors, t_elem, tau_rows=None):
    """a copy of the restatement with one defect: (env, gov) as a device with that defect would return them.  tau_rows: the rows
    (G with tau = 1 for EVERY case) the defect 'tau_everywhere' combines."""
    f = np.asarray(factors, dtype=np.float64)
    n_combos, n_cases = f.shape
    if kind == "transposed":
        f = f.ravel()[np.arange(n_cases)[None, :] * n_combos + np.arange(n_combos)[:, None]]
    if kind == "tail_case":
        f = f.copy()
        f[:, -1] = 0.0
    q = ev.values(ev.combine(tau_rows if kind == "tau_everywhere" else G, f), t_elem)
    env, gov = q[0].copy(), np.zeros(q.shape[1:], dtype=np.int32)
    is_min = ev.IS_MIN.copy()
    if kind == "q3_swapped":
        is_min[3] = False
    for c in range(1, n_combos):
        if kind == "last_on_tie":
            take = np.where(is_min, q[c] <= env, q[c] >= env)
        else:
            take = np.where(is_min, q[c] < env, q[c] > env)
        env = np.where(take, q[c], env)
        gov = np.where(take, c, gov).astype(np.int32)
    return env, gov


@pytest.mark.parametrize("kind", ["none", "last_on_tie", "q3_swapped", "transposed", "tail_case", "tau_everywhere"])
def test_the_checker_catches_planted_defects(kind):
    xyz, tri, quad, u, tau, thermal, G, S, t_elem = _petals()
    f = _factors()
    f[5] = f[2]  # two equal combinations: a tie in every element
    ref = ev.Reference(G, S, f, t_elem)
    tau_rows = ev.case_rows(xyz, tri, quad, u, np.ones(N_CASES), thermal=thermal)[0] if kind == "tau_everywhere" else None
    env, gov = _defective(kind, G, S, f, t_elem, tau_rows)
    if kind == "none":
        assert ev.check(env, gov, ref) == 0.0
    else:
        with pytest.raises(AssertionError):
            ev.check(env, gov, ref)


# ------------------------------------------------------------------ bitwise consequences of the definition, in float64

def test_bitwise_consequences_hold_in_float64():
    _, _, _, _, _, _, G, S, t_elem = _petals()
    f = _factors()
    ref = ev.Reference(G, S, f, t_elem)
    # a factor of exactly 0 leaves no trace of its case
    f0 = f.copy()
    f0[:, 3] = 0.0
    G_other = G.copy()
    G_other[3] = 1e3 * G[3][::-1]
    a, b = ev.Reference(G, S, f0, t_elem), ev.Reference(G_other, S, f0, t_elem)
    assert np.array_equal(a.q, b.q) and np.array_equal(a.gov, b.gov)
    without = ev.Reference(np.delete(G, 3, axis=0), np.delete(S, 3, axis=0), np.delete(f0, 3, axis=1), t_elem)
    assert np.array_equal(a.q, without.q)
    # factors scaled by 2^10 scale the values by 2^10
    big = ev.Reference(G, S, 1024.0 * f, t_elem)
    assert np.array_equal(big.q, 1024.0 * ref.q) and np.array_equal(big.env, 1024.0 * ref.env) and np.array_equal(big.gov, ref.gov)
    # duplicate rows: the same values, the lower index governs
    fd = np.concatenate([f, f[1:3]])
    dup = ev.Reference(G, S, fd, t_elem)
    assert np.array_equal(dup.q[7:], dup.q[1:3]) and np.array_equal(dup.env, ref.env) and np.array_equal(dup.gov, ref.gov)
    # a permutation of the combinations leaves env and permutes gov (no two combinations tie here)
    perm = np.random.default_rng(2).permutation(N_COMBOS)
    p = ev.Reference(G, S, f[perm], t_elem)
    assert np.array_equal(p.env, ref.env) and np.array_equal(perm[p.gov], ref.gov)

