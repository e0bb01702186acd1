"""Load combinations (femshell_combination_envelope): the reference of the tests, numpy on top of
tests/helpers/resultants.py and tests/helpers/thermal.py, and the one checker the device tests call.

The restatement needs no local frame.  Per case the twelve GLOBAL tensor words of mesh_resultants (thermal.mesh_resultants for a
case loaded with the free thermal state, tau_j = 1); a combination is the factored sum of the cases' words, added in index order;
from the combined 3 x 3 tensors N and M of an element, with its thickness t:
    q0, q1 = von Mises of sigma = N / t +- 6 M / t^2 as sqrt((3 sigma:sigma - (tr sigma)^2) / 2)
    q2, q3 = the two eigenvalues of N that do not belong to the normal (eigvalsh; the one of smallest magnitude is the normal's
             zero: where a principal value is smaller still, the two differ by the rounding of the tensor, far inside the bound)
    q4, q5 = those of M
and the envelope takes max, max, max, min, max, min over the combinations with the FIRST index that attains each.

Scales, by linearity: S_c = sum_j |f_cj| S_j of the fourteen words of mesh_resultants.  von Mises: words 12 and 13.  A principal
value moves by at most the Frobenius norm of the change of its tensor: S_xx + S_yy + S_zz + 2 (S_xy + S_yz + S_zx) of the N or
the M words.  A value agrees with the reference when |value - ref| <= 1e-12 scale."""
import numpy as np

from tests.helpers import resultants as rs

TINY = rs.TINY
IS_MIN = np.array([False, False, False, True, False, True])


def element_thickness(n_tri, n_quad, t=rs.T, sec=None):
    """(n_tri + n_quad,): the thickness of every element, triangles then quadrilaterals"""
    if sec is None:
        return np.full(n_tri + n_quad, float(t))
    table = np.asarray(sec[0], dtype=np.float64).reshape(-1, 3)
    idx = [np.asarray(s, dtype=np.int64) for s, n in ((sec[1], n_tri), (sec[2], n_quad)) if n]
    return table[np.concatenate(idx), 2]


def case_rows(xyz, tri, quad, u, case_thermal=None, sec=None, thermal=None, nu=rs.NU, E=rs.E, t=rs.T):
    """(G (n_cases, ne, 12), S (n_cases, ne, 14)): the global tensor words of every case and the scales of its fourteen values.
    thermal = dict(tri_temp, quad_temp, alpha, sec_alpha): the temperatures in force, used by the cases with case_thermal[j] = 1
    (entries other than 0 and 1 are not restated)."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, len(xyz), 6)
    G, S = [], []
    for j, uj in enumerate(u):
        tau = 0.0 if case_thermal is None else float(case_thermal[j])
        if tau == 0.0:
            o, s = rs.mesh_resultants(xyz, tri, quad, uj, nu, E, t, sec=sec)
        else:
            assert tau == 1.0 and thermal is not None
            from tests.helpers import thermal as th
            o, s = th.mesh_resultants(xyz, tri, quad, uj, thermal["tri_temp"], thermal["quad_temp"], thermal["alpha"], nu=nu, E=E, t=t, sec=sec,
                                      sec_alpha=thermal.get("sec_alpha"))
        G.append(o[:, :12])
        S.append(s)
    return np.array(G), np.array(S)


def combine(G, factors):
    """(n_combos, ne, w): sum_j f_cj G_j, added case after case in index order from zero"""
    factors = np.asarray(factors, dtype=np.float64)
    out = np.zeros((len(factors),) + G.shape[1:])
    for c, f in enumerate(factors):
        for j in range(G.shape[0]):
            out[c] = out[c] + f[j] * G[j]
    return out


def _tensor(w6):
    """(..., 3, 3) from (..., 6) words xx yy zz xy yz zx"""
    T = np.zeros(w6.shape[:-1] + (3, 3))
    for k, (p, q) in enumerate(rs.VOIGT):
        T[..., p, q] = w6[..., k]
        T[..., q, p] = w6[..., k]
    return T


def von_mises_free(sig6):
    s = _tensor(sig6)
    ss = (s * s).sum(axis=(-1, -2))
    tr = np.trace(s, axis1=-2, axis2=-1)
    return np.sqrt(np.maximum((3.0 * ss - tr * tr) / 2.0, 0.0))


def principal_free(w6):
    """(..., 2): the larger and the smaller in-plane eigenvalue of a tensor whose normal direction carries nothing"""
    lam = np.linalg.eigvalsh(_tensor(w6))
    drop = np.abs(lam).argmin(axis=-1)
    keep = np.ones(lam.shape, bool)
    np.put_along_axis(keep, drop[..., None], False, axis=-1)
    two = lam[keep].reshape(lam.shape[:-1] + (2,))  # ascending
    return two[..., ::-1]


def values(Gc, t_elem):
    """(..., ne, 6) = q0..q5 of combined global words (..., ne, 12)"""
    t = np.asarray(t_elem, dtype=np.float64)[:, None]
    N, M = Gc[..., :6], Gc[..., 6:12]
    pn, pm = principal_free(N), principal_free(M)
    return np.stack([von_mises_free(N / t + 6.0 * M / (t * t)), von_mises_free(N / t - 6.0 * M / (t * t)), pn[..., 0], pn[..., 1], pm[..., 0],
                     pm[..., 1]], axis=-1)


def value_scales(Sc):
    """(..., ne, 6): the scales of q0..q5 from the combined scales (..., ne, 14)"""
    fro = lambda s: s[..., 0] + s[..., 1] + s[..., 2] + 2.0 * (s[..., 3] + s[..., 4] + s[..., 5])  # noqa: E731
    sn, sm = fro(Sc[..., :6]), fro(Sc[..., 6:12])
    return np.stack([Sc[..., 12], Sc[..., 13], sn, sn, sm, sm], axis=-1)


def extremes(q):
    """(env (ne, 6), gov (ne, 6)) of q (n_combos, ne, 6): the first index wins (a later one only when strictly beyond)"""
    env, gov = q[0].copy(), np.zeros(q.shape[1:], dtype=np.int32)
    for c in range(1, len(q)):
        take = np.where(IS_MIN, q[c] < env, q[c] > env)
        env = np.where(take, q[c], env)
        gov = np.where(take, c, gov).astype(np.int32)
    return env, gov


class Reference:
    """what the checker compares with: q (n_combos, ne, 6), its scales, the envelope and the governing combinations"""

    def __init__(self, G, S, factors, t_elem):
        self.factors = np.asarray(factors, dtype=np.float64).reshape(-1, G.shape[0])
        self.q = values(combine(G, self.factors), t_elem)
        self.S = value_scales(combine(S, np.abs(self.factors)))
        self.env, self.gov = extremes(self.q)


def reference(xyz, tri, quad, u, factors, case_thermal=None, sec=None, thermal=None, nu=rs.NU, E=rs.E, t=rs.T):
    G, S = case_rows(xyz, tri, quad, u, case_thermal, sec, thermal, nu, E, t)
    n_tri = 0 if tri is None else len(tri)
    n_quad = 0 if quad is None else len(quad)
    return Reference(G, S, factors, element_thickness(n_tri, n_quad, t, sec))


def check(env, gov, ref):
    """The one judgement of an envelope against the reference, per element and k:
      - gov is a combination;
      - |env - q_ref[gov]| <= 1e-12 S[gov];
      - no combination of the reference beats env by more than the bound of that combination;
      - among combinations with the same row of factors -- whose values are the same bits wherever they stand -- the lowest governs.
    Near-ties need no exclusion: whichever of two close combinations governs, each statement holds within its own bound.
    Returns the largest ratio of a difference to its bound (for the tests' printed figures)."""
    env, gov = np.asarray(env), np.asarray(gov)
    n_combos, ne, _ = ref.q.shape
    assert env.shape == (ne, 6) and gov.shape == (ne, 6)
    assert gov.min() >= 0 and gov.max() < n_combos, "gov out of range"
    q_at = np.take_along_axis(ref.q, gov[None].astype(np.int64), axis=0)[0]
    S_at = np.take_along_axis(ref.S, gov[None].astype(np.int64), axis=0)[0]
    worst = rs.bound_ratio(env, q_at, S_at)
    assert worst <= 1.0, "env differs from the reference of its governing combination: %.3e of the bound" % worst
    sign = np.where(IS_MIN, -1.0, 1.0)
    beat = sign * (ref.q - env[None])  # > 0: combination c lies beyond env
    over = beat - TINY * ref.S
    assert not (over > 0.0).any(), "a combination of the reference beats env: %s" % (np.argwhere(over > 0.0)[:4],)
    first_equal = np.array([min(d for d in range(n_combos) if np.array_equal(ref.factors[d], ref.factors[c])) for c in range(n_combos)])
    assert np.array_equal(first_equal[gov], gov), "a combination governs although an equal one stands in front of it"
    return worst
