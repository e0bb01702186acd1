"""Load combinations on the device (femshell_combination_envelope, FemShell.combination_envelope) against
tests/helpers/envelope.py, the reference tests/test_envelope_cpu.py holds to itself, judged by its one checker."""
import functools

import numpy as np
import pytest

from tests.helpers import envelope as ev, meshes, prescribed as pr, resultants as rs, sections, thermal as th
from tests.helpers.product import ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

N_CASES, N_COMBOS = 5, 7
ALPHA = 1.2e-5
SEC_ALPHA = [1.1e-5, 2.3e-5, 0.7e-5]


def _counts(tri, quad):
    return (0 if tri is None else len(tri)), (0 if quad is None else len(quad))


def _context(xyz, tri, quad, sec=None):
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    fs.set_mesh(xyz, tri, quad)
    if sec is not None:
        fs.set_sections(sec[0], sec[1], sec[2])
    return fs


def _cases(n_nodes, n_cases=N_CASES):
    return np.array([rs.random_u(n_nodes, seed=30 + j) for j in range(n_cases)])


def _factors(n_combos=N_COMBOS, n_cases=N_CASES, seed=21):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (n_combos, n_cases))


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return rs.device_meshes()[name]()


@functools.lru_cache(maxsize=None)
def _rows(name):
    """(u, G, S, t_elem) of the five random cases on a mesh of device_meshes(): computed once, shared, never written"""
    xyz, tri, quad, sec, _ = _mesh(name)
    u = _cases(len(xyz))
    G, S = ev.case_rows(xyz, tri, quad, u, sec=sec)
    nt, nq = _counts(tri, quad)
    for a in (u, G, S):
        a.setflags(write=False)
    return u, G, S, ev.element_thickness(nt, nq, rs.T, sec)


def _device(name, monkeypatch=None):
    xyz, tri, quad, sec, env = _mesh(name)
    if monkeypatch is not None:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return _context(xyz, tri, quad, sec)


# ------------------------------------------------------------------ 1. device against reference

@pytest.mark.parametrize("name", list(rs.device_meshes()))
def test_envelope_matches_the_reference(name, monkeypatch):
    """five cases of random u, seven combinations with factors in (-2, 2): the checker of tests/helpers/envelope.py"""
    fs = _device(name, monkeypatch)
    u, G, S, t_elem = _rows(name)
    f = _factors()
    env, gov, info = fs.combination_envelope(u, f)
    assert gov.dtype == np.int32
    worst = ev.check(env, gov, ev.Reference(G, S, f, t_elem))
    print("envelope_vs_reference %-28s elements %5d  max |env - q_ref[gov]| / (1e-12 S) = %.3e" % (name, len(env), worst))


@pytest.mark.parametrize("name", ["one_triangle", "one_quadrilateral", "mixed_petals24", "panel_three_sections", "trimmed_panel_257"])
def test_identity_factors_give_the_rows_of_element_resultants(name, monkeypatch):
    """stage 1 alone: with the unit matrix as factors and one combination per call, q0 and q1 of case j are words 12 and 13 of
    element_resultants(u_j), q2..q5 the in-plane eigenvalues of its tensors, within 1e-12 S of that case"""
    fs = _device(name, monkeypatch)
    u, G, S, t_elem = _rows(name)
    worst = 0.0
    for j in range(N_CASES):
        f = np.zeros((1, N_CASES))
        f[0, j] = 1.0
        env, gov, _ = fs.combination_envelope(u, f)
        assert not gov.any()
        out = fs.element_resultants(u[j])
        pn, pm = ev.principal_free(out[:, :6]), ev.principal_free(out[:, 6:12])
        direct = np.stack([out[:, 12], out[:, 13], pn[:, 0], pn[:, 1], pm[:, 0], pm[:, 1]], axis=1)
        worst = max(worst, rs.bound_ratio(env, direct, ev.value_scales(S[j])))
    print("envelope identity rows %-28s max difference / (1e-12 S) = %.3e" % (name, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------ 2. bits

@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24"])
def test_bits(name):
    fs = _device(name)
    u, _, _, _ = _rows(name)
    f = _factors()
    env, gov, _ = fs.combination_envelope(u, f)
    # two calls agree
    again = fs.combination_envelope(u, f)
    assert np.array_equal(env, again[0]) and np.array_equal(gov, again[1])
    # the envelope over all combinations is the elementwise extreme, with the first index, of the calls with one combination
    single = np.array([fs.combination_envelope(u, f[c:c + 1])[0] for c in range(N_COMBOS)])
    e1, g1 = ev.extremes(single)
    assert np.array_equal(env, e1) and np.array_equal(gov, g1)
    # a unit combination in the company of 1, 2, 3, 4, 5 and 7 cases, in two orders: the bits of the one-case call
    seven = _cases(u.shape[1], 7)
    alone = fs.combination_envelope(seven[2:3], np.ones((1, 1)))[0]
    for n in (1, 2, 3, 4, 5, 7):
        for order in (np.arange(n), np.arange(n)[::-1]):
            company = seven[(2 + order) % 7]  # case 2 first, or last
            unit = np.zeros((1, n))
            unit[0, int(np.flatnonzero(order == 0)[0])] = 1.0
            assert np.array_equal(fs.combination_envelope(company, unit)[0], alone), (n, order)
    # a factor of exactly 0 leaves no trace of its case
    f0 = f.copy()
    f0[:, 3] = 0.0
    other = np.array(u)
    other[3] = 1e3 * rs.random_u(u.shape[1], seed=99)
    a, b = fs.combination_envelope(u, f0), fs.combination_envelope(other, f0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = fs.combination_envelope(np.delete(u, 3, axis=0), np.delete(f0, 3, axis=1))
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    # factors times 2^10 scale env bit for bit
    big = fs.combination_envelope(u, 1024.0 * f)
    assert np.array_equal(big[0], 1024.0 * env) and np.array_equal(big[1], gov)
    # two equal combinations report the lower index
    fd = np.concatenate([f, f])
    dup = fs.combination_envelope(u, fd)
    assert np.array_equal(dup[0], env) and np.array_equal(dup[1], gov)
    # permuting the combinations leaves env and permutes gov
    perm = np.random.default_rng(2).permutation(N_COMBOS)
    p = fs.combination_envelope(u, f[perm])
    assert np.array_equal(p[0], env) and np.array_equal(perm[p[1]], gov)


# ------------------------------------------------------------------ 3. temperatures

@pytest.mark.parametrize("name", ["lifted_panel", "one_quadrilateral", "mixed_petals24", "panel_three_sections"])
def test_temperatures_with_the_cases_that_carry_them(name):
    """temperatures in force, tau = (1, 0, 0): against the reference; the identity row of case 0 against element_resultants(u_0) of
    the same context (which subtracts the free state); case_thermal = None gives the bits of a twin without temperatures"""
    xyz, tri, quad, sec, _ = _mesh(name)
    nt, nq = _counts(tri, quad)
    fs = _device(name)
    sa = None
    if sec is None:
        fs.set_expansion(ALPHA)
    else:
        fs.set_expansion(0.0, SEC_ALPHA)
        sa = SEC_ALPHA
    tt, qt = th.random_temps(nt, nq)
    fs.set_thermal(tt, qt)
    u = _cases(len(xyz), 3)
    u[0] *= 1e-3  # (the free strains are of the size alpha T = 1e-3: neither part drowns the other)
    tau = np.array([1.0, 0.0, 0.0])
    f = _factors(N_COMBOS, 3, seed=22)
    thermal = {"tri_temp": tt, "quad_temp": qt, "alpha": ALPHA, "sec_alpha": sa}
    G, S = ev.case_rows(xyz, tri, quad, u, tau, sec=sec, thermal=thermal)
    t_elem = ev.element_thickness(nt, nq, rs.T, sec)
    env, gov, _ = fs.combination_envelope(u, f, tau)
    worst = ev.check(env, gov, ev.Reference(G, S, f, t_elem))
    cold = ev.Reference(ev.case_rows(xyz, tri, quad, u, sec=sec)[0], S, f, t_elem)
    with pytest.raises(AssertionError):  # the temperatures show
        ev.check(env, gov, cold)
    # the identity row of case 0
    e0 = fs.combination_envelope(u, np.array([[1.0, 0.0, 0.0]]), tau)[0]
    out = fs.element_resultants(u[0])
    pn, pm = ev.principal_free(out[:, :6]), ev.principal_free(out[:, 6:12])
    direct = np.stack([out[:, 12], out[:, 13], pn[:, 0], pn[:, 1], pm[:, 0], pm[:, 1]], axis=1)
    ident = rs.bound_ratio(e0, direct, ev.value_scales(S[0]))
    print("envelope thermal %-24s vs reference %.3e, identity row of the heated case %.3e (of 1e-12 S)" % (name, worst, ident))
    assert ident <= 1.0
    # no case carries them: the bits of a context that has none
    twin = _device(name)
    a, b = fs.combination_envelope(u, f), twin.combination_envelope(u, f)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    z = fs.combination_envelope(u, f, np.zeros(3))
    assert np.array_equal(a[0], z[0]) and np.array_equal(a[1], z[1])


# ------------------------------------------------------------------ 4. order

@pytest.mark.parametrize("reorder", ["", "rcm", "morton"])
def test_rows_are_the_callers_elements(reorder, monkeypatch):
    """mixed mesh, one section per element, all different: row i is the caller's element i -- its triangles, then its
    quadrilaterals -- whatever numbering the library uses inside.  No other row of the reference passes for it."""
    if reorder:
        monkeypatch.setenv("FEMSHELL_REORDER", reorder)
    xyz, tri, quad = meshes.mixed_petals(24)
    ne = len(tri) + len(quad)
    table = np.stack([0.05 + 0.01 * np.arange(ne), 1e5 * (1.0 + 0.37 * np.arange(ne)), 0.02 * (1.0 + 0.11 * np.arange(ne))], axis=1)
    sec = (table, np.arange(len(tri), dtype=np.int32), len(tri) + np.arange(len(quad), dtype=np.int32))
    fs = _context(xyz, tri, quad, sec)
    u, f = _cases(len(xyz)), _factors()
    env, gov, _ = fs.combination_envelope(u, f)
    G, S = ev.case_rows(xyz, tri, quad, u, sec=sec)
    ref = ev.Reference(G, S, f, ev.element_thickness(len(tri), len(quad), rs.T, sec))
    ev.check(env, gov, ref)
    for i in range(ne):
        for j in range(ne):
            if i != j:
                assert rs.bound_ratio(ref.env[j], ref.env[i], np.take_along_axis(ref.S[:, i], ref.gov[i][None].astype(np.int64), axis=0)[0]) > 1.0, (i, j)


# ------------------------------------------------------------------ 5. limits

@pytest.mark.parametrize("name", ["one_triangle", "trimmed_panel_257"])
def test_the_largest_counts(name):
    """32 cases x 256 combinations: every pass of both kernels full and their loops at their longest"""
    xyz, tri, quad, sec, _ = _mesh(name)
    fs = _device(name)
    u = _cases(len(xyz), 32)
    f = _factors(256, 32, seed=23)
    G, S = ev.case_rows(xyz, tri, quad, u, sec=sec)
    env, gov, _ = fs.combination_envelope(u, f)
    ev.check(env, gov, ev.Reference(G, S, f, ev.element_thickness(len(tri), 0)))


# ------------------------------------------------------------------ 6. the context is left as it was

def test_the_call_leaves_the_context_as_it_was():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    loads = np.zeros((n, 6))
    loads[:, :3] = np.random.default_rng(3).normal(size=(n, 3))
    results = []
    for call in (False, True):
        fs = _context(xyz, tri, None)
        fs.set_dirichlet(mask)
        fs.set_loads(loads)
        u0, i0 = fs.solve(rtol=1e-10, max_it=5000)
        if call:
            fs.combination_envelope(_cases(n), _factors())
        u1, i1 = fs.solve(rtol=1e-10, max_it=5000)
        s1 = fs.element_resultants()
        uc, _, _ = fs.solve_cases(np.stack([loads, 2.0 * loads[::-1]]), rtol=1e-10, max_it=5000)
        results.append((u0, u1, i1["iterations"], s1, uc))
    for a, b in zip(*results):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 7. refusals

def test_refusals_leave_the_context_usable():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    u, f = _cases(n, 3), _factors(4, 3)
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    L, h = fs._L, fs._h
    from importlib import import_module
    b = import_module(pkg.__name__ + ".binding")
    env_buf, gov_buf = np.full((len(tri), 6), -7.0), np.full((len(tri), 6), -7, np.int32)

    def raw(n_cases=3, uu=u, tau=None, n_combos=4, ff=f, env=env_buf):
        rc = L.femshell_combination_envelope(h, n_cases, b._d(uu), b._d(tau), n_combos, b._d(ff), b._d(env), b._i(gov_buf), None)
        assert (env_buf == -7.0).all() and (gov_buf == -7).all()  # outputs not written
        return rc, L.femshell_last_error().decode()

    rc, msg = raw()
    assert rc == -1 and "no mesh" in msg
    fs.set_mesh(xyz, tri)
    good = fs.combination_envelope(u, f)

    def still_good():
        again = fs.combination_envelope(u, f)
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])

    assert L.femshell_combination_envelope(None, 3, b._d(u), None, 4, b._d(f), b._d(env_buf), None, None) == -1
    for kw in ({"uu": None}, {"ff": None}, {"env": None}):
        rc, msg = raw(**kw)
        assert rc == -1 and "null argument" in msg
        still_good()
    for kw in ({"n_cases": 0}, {"n_cases": 33}, {"n_combos": 0}, {"n_combos": 257}):
        rc, msg = raw(**kw)
        assert rc == -1 and "must be in" in msg
        still_good()
    bad_u, bad_f = u.copy(), f.copy()
    bad_u[2, 5, 2] = np.inf
    bad_f[1, 1] = np.nan
    for kw in ({"uu": bad_u}, {"ff": bad_f}, {"tau": np.array([0.0, np.inf, 0.0])}):
        rc, msg = raw(**kw)
        assert rc == -1 and "non-finite" in msg
        still_good()
    rc, msg = raw(tau=np.array([0.0, 1.0, 0.0]))
    assert rc == -1 and "no temperatures" in msg
    still_good()
    # the binding's own shape checks
    for bu, bf, bt in ((np.zeros(7), f, None), (u, np.zeros((4, 2)), None), (u, np.zeros((0, 3)), None), (u, f, np.zeros(2))):
        with pytest.raises(ValueError):
            fs.combination_envelope(bu, bf, bt)
    still_good()
    # dynamics
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    fs.set_dirichlet(mask)
    fs.set_density(7.8e-9)
    fs.dynamics_begin(1e-3)
    rc, msg = raw()
    assert rc == -1 and "dynamics" in msg
    fs.dynamics_end()
    still_good()
    # a degenerate element (zero area, three different nodes) is reported by its number in the caller's list
    flat_xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=np.float64)
    other = pkg.FemShell(rs.NU, rs.E, rs.T)
    other.set_mesh(flat_xyz, np.array([[0, 1, 3], [1, 2, 3], [0, 1, 2]], np.int32))
    with pytest.raises(pkg.FemShellError) as e:
        other.combination_envelope(_cases(4, 3), f)
    assert e.value.code == -4 and "triangle 2" in str(e.value)
    still_good()
    # a row partition
    part = pkg.FemShell(rs.NU, rs.E, rs.T, rank=0, world_size=2)
    assert L.femshell_combination_envelope(part._h, 3, b._d(u), None, 4, b._d(f), b._d(env_buf), b._i(gov_buf), None) == -7
    assert "single-rank" in L.femshell_last_error().decode() and (env_buf == -7.0).all()


# ------------------------------------------------------------------ 8. byte model

@pytest.mark.parametrize("with_sections", [False, True])
def test_info_returns_the_byte_model(with_sections):
    """DESIGN.md 8n.  Stage 1: the ids of every element, coordinates once per node (24 B), a section index per element with
    sections (4 B), temperatures per element in a call that carries them (16 B); per case 48 B of displacements per node, 48 B
    written per element and, with temperatures, the 8 B of tau.  Stage 2: the table once per pass of four combinations, the
    factors once, 48 + 24 B written per element, a section index per element with sections."""
    xyz, tri, quad = meshes.mixed_petals(24)
    sec = (sections.THREE, np.arange(len(tri), dtype=np.int32) % 3, np.arange(len(quad), dtype=np.int32) % 3) if with_sections else None
    fs = _context(xyz, tri, quad, sec)
    ne, nn = len(tri) + len(quad), len(xyz)
    for n_cases, n_combos, heated in ((5, 7, False), (3, 4, True), (1, 1, False)):
        tau = None
        if heated:
            if with_sections:
                fs.set_expansion(0.0, SEC_ALPHA)
            else:
                fs.set_expansion(ALPHA)
            fs.set_thermal(*th.random_temps(len(tri), len(quad)))
            tau = np.array([0.0, 1.0, 0.0])
        _, _, info = fs.combination_envelope(_cases(nn, n_cases), _factors(n_combos, n_cases), tau)
        fixed = 12 * len(tri) + 16 * len(quad) + 24 * nn + (4 * ne if with_sections else 0) + (16 * ne if heated else 0)
        assert info["bytes_cases"] == fixed + n_cases * (48 * nn + 48 * ne + (8 if heated else 0))
        passes = -(-n_combos // 4)
        assert info["bytes_envelope"] == passes * n_cases * 48 * ne + 8 * n_combos * n_cases + 72 * ne + (4 * ne if with_sections else 0)
        assert info["seconds_cases"] > 0.0 and info["seconds_envelope"] > 0.0
