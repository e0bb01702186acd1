"""The block kernels of the eigen-solvers (csrc/modal.hip: k_block_combine, k_block_residual and its sums, k_block_bj,
k_block_mask, k_modal_init) against a truth, kernel by kernel: the truths, the derived bounds, the assertions the GPU tests
(tests/test_gpu_modal_truth.py) and the CPU pins (tests/test_modal_truth_cpu.py) share, and a restatement of every kernel that
takes planted defects.  numpy and the standard library only; built on residual_truth.py and krylov_truth.py (two_product, gamma,
exact_dot, within, U = 2^-53).  A block is an array (columns, 6 n_nodes) in the caller's numbering; `free` is bool[6 n_nodes].

combine   Y[o][r] = sum_k sum_c S_k[c][r] C_k[c][o] is one chain of Q = sum q_k products and additions from +0.0, each product
          contracted into its addition or not.  Truth: the correctly rounded sum of the error-free products (exact_dot).
          Bound: gamma_Q sum |s c| + u |truth| -- gamma_Q covers Q roundings of products and additions in any order, contracted
          or not (Higham, Accuracy and Stability, section 3.1); u is the truth's own rounding.  A selection matrix (one entry
          2^k per output column) leaves one exact product and additions of zeros: bit for bit.
residual  r = kx - theta (m x) in long double.  The device rounds t = m x (u |m x|), then either contracts theta t into the
          subtraction (one rounding, u |r|) or rounds theta t (u |theta t|) and the difference (u |r|):
          |err| <= u |r| + gamma_2 |theta m x|.  (The truth's own products are rounded to 64 bits: 2^-11 of that bound.)
          Constrained dofs are +0.0.
sums      norms[i] is the float64 sum of partials[i][0 .. 127] in index order, bit for bit: plain additions, nothing to contract.
partials  partial b of a column is the sum of r^2 / m over the free dofs with m > 0 of the nodes [b per, min((b + 1) per, n_pad)),
          per = ceil(n_pad / 128), of the DEVICE's own R: terms in long double, split into two doubles and added by math.fsum.
          Every device term carries two roundings (the square, the quotient), a sum of n terms in any order gamma_(n - 1):
          (gamma_n + 2 u) sum terms.  Workgroups past the rows give +0.0.
norm      end to end against sum r*^2 / m of the truth residual: the row bound b carried through the square,
          sum (2 |r*| b + b^2) / m, plus (gamma_n + 2 u + gamma_128)(1 + 1e-10) times the sum -- n the terms of the longest
          stretch, gamma_128 for the 127 additions of the partial sums.
bj        z_i = sum_j Dinv[i][j] r_j over the device's own exported inverse: exact_dot of 6 terms; gamma_6 sum |.| + u |truth|.
          Constrained dofs are +0.0 whatever R holds there.
mask      no arithmetic: free entries keep their bits, the others are +0.0.
start     splitmix64 in Python integers (and in numpy's wrapping uint64, pinned equal), then the kernel's mapping in float64:
          (float(k) + 0.5) 2^-53 with k = h >> 11, and 2 u - 1.  k < 2^53 converts exactly and the scalings are by powers of two.
          Below 2^52 the sum k + 0.5 is exact and 2 u - 1 = (2 k + 1 - 2^53) 2^-53, a 53-bit integer times a power of two; from
          2^52 on the sum rounds to an integer n (ties to even) and 2 u - 1 = (n - 2^52) 2^-52: every operation but the one
          addition is exact, and that one rounds the same way everywhere -- bit for bit.  (Two values of k in 2^53 land on an
          excluded point: k = 2^52 rounds down to u = 1/2, x = 0, and k = 2^53 - 1 rounds up to u = 1, x = 1; assert_start checks
          |x| < 1 and x != 0 on what it is given.)

Every model takes defect=None or one of its DEFECTS; tests/test_modal_truth_cpu.py shows that each planted defect fails the
assertion its kernel is held to."""
import math

import numpy as np

from tests.helpers import krylov_truth as kt
from tests.helpers import residual_truth as rt

U = rt.U
LD = np.longdouble
GRID = 128  # kGramGrid: the workgroups of k_block_residual = the partial sums of a column
CHUNK = 32  # kCombineChunk


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, label=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    bad = np.flatnonzero((g != w).reshape(-1))
    assert bad.size == 0, "%s: %d words differ, the first at %d: %r, expected %r" % (
        label, bad.size, int(bad[0]), float(np.asarray(got).reshape(-1)[bad[0]]), float(np.asarray(want).reshape(-1)[bad[0]]))


def within(got, want, bound):
    """kt.within, and no entry of got is NaN or infinite (a comparison with NaN is false: it would pass)"""
    got = np.asarray(got, dtype=np.float64)
    bad = np.flatnonzero(~np.isfinite(got).reshape(-1))
    assert bad.size == 0, "%d entries are not finite, the first at %d" % (bad.size, int(bad[0]))
    return kt.within(got, want, bound)


def free_dofs(dmask, n_nodes):
    if dmask is None:
        return np.ones(6 * n_nodes, dtype=bool)
    dm = np.asarray(dmask, dtype=np.uint8)
    return (((dm[:, None] >> np.arange(6)[None, :]) & 1) == 0).ravel()


def exact_dots(A, B):
    """the correctly rounded sum over axis 0 of A * B, column by column (exact_dot of krylov_truth, many at once)"""
    A, B = np.broadcast_arrays(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))
    P, E = rt.two_product(np.ascontiguousarray(A), np.ascontiguousarray(B))
    rows = np.concatenate([P, E]).reshape(2 * len(A), -1).T.tolist()
    return np.array([math.fsum(r) for r in rows]).reshape(A.shape[1:])


# ------------------------------------------------------------------ combine

# (q of the sources, n_out, ldc - n_out): every q of {1, 31, 32, 33, 64, 65, 96} alone, three sources -- one of them empty --, every
# n_out of {1, 2, 3, 4, 5, 17, 63, 64}, the contract's corner (96, 64)
COMBINE_SHAPES = (((1,), 1, 0), ((31,), 2, 3), ((32,), 3, 0), ((33,), 4, 3), ((64,), 5, 0), ((65,), 17, 3), ((96,), 63, 3),
                  ((96,), 64, 0), ((12, 7, 12), 5, 0), ((12, 7, 12), 17, 3), ((32, 32, 32), 4, 0), ((32, 32, 32), 64, 3),
                  ((5, 0, 3), 1, 0), ((5, 0, 3), 2, 0), ((5, 0, 3), 5, 3))
# the thinner list of the 475-node patch under random coefficients (an exact dot product per entry)
COMBINE_SHAPES_THIN = (((1,), 1, 0), ((33,), 4, 3), ((65,), 17, 3), ((96,), 5, 0), ((12, 7, 12), 17, 3), ((32, 32, 32), 4, 0),
                       ((5, 0, 3), 5, 3))


def combine_defect_shows(defect, q, n_out, extra):
    """the shapes at which a planted defect changes what the kernel computes"""
    return {"drop_chunk_last": max(q) >= CHUNK, "swap_wave_e": n_out >= 5, "ldc_is_n_out": extra > 0 and sum(q) > 1,
            "skip_after_empty": len(q) == 3 and q[1] == 0 and q[2] > 0}[defect]


COMBINE_DEFECTS = ("drop_chunk_last", "swap_wave_e", "ldc_is_n_out", "skip_after_empty")


def _sources(sources):
    return [None if s is None or len(s) == 0 else np.ascontiguousarray(s, dtype=np.float64).reshape(len(s), -1) for s in sources]


def stacked(sources):
    """the source columns one behind the other: (Q, 6 n)"""
    return np.concatenate([s for s in _sources(sources) if s is not None])


def combine_truth(sources, Cm, n_out):
    """(truth (n_out, 6 n), bound)"""
    S = stacked(sources)
    Cm = np.asarray(Cm, dtype=np.float64)
    assert Cm.shape[0] == len(S) and Cm.shape[1] >= n_out
    g = kt.gamma(len(S))
    truth, bound = np.zeros((n_out, S.shape[1])), np.zeros((n_out, S.shape[1]))
    for o in range(n_out):
        c = Cm[:, o][:, None]
        truth[o] = exact_dots(S, c)
        bound[o] = (g * np.abs(S.astype(LD) * c.astype(LD)).sum(axis=0) + U * np.abs(truth[o])).astype(np.float64)
    return truth, bound


def assert_combine(Y, sources, Cm, n_out):
    """returns the largest share of the bound used"""
    truth, bound = combine_truth(sources, Cm, n_out)
    assert np.shape(Y) == truth.shape
    return within(Y, truth.astype(LD), bound)


def selection(q, n_out, ldc, seed=0):
    """(Cm (sum q, ldc), pi[n_out], k[n_out]): output o is 2^k[o] times source column pi[o] -- a fixed map with repeats that
    crosses sources and chunks: multiples of a stride coprime to Q, so neighbouring outputs land in different chunks; the columns
    of Cm beyond n_out hold a value no output may pick up"""
    Q = int(np.sum(q))
    stride = next(s for s in (37, 41, 43, 47, 53) if math.gcd(s, Q) == 1 or Q == 1)
    pi = (np.arange(n_out) * stride + seed + Q - 1) % Q
    if n_out >= 3:
        pi[2] = pi[0]  # a repeat
    k = (np.arange(n_out) % 5) - 2
    Cm = np.zeros((Q, ldc))
    Cm[:, n_out:] = 3.0
    Cm[pi, np.arange(n_out)] = 2.0 ** k
    return Cm, pi, k


def assert_selection(Y, sources, pi, k, label=""):
    S = stacked(sources)
    assert_same_bits(Y, S[pi] * (2.0 ** np.asarray(k, dtype=np.float64))[:, None], label)


def combine_model(sources, Cm, n_out, defect=None):
    """k_block_combine in float64, uncontracted: per output a chain over the sources, the chunks of 32 columns and the columns.
    defect: None, or
      "drop_chunk_last"   the last column of a full 32-column chunk is left out
      "swap_wave_e"       output o = wave + 4 e >= 4 takes the coefficients of output 4 wave + e (where that is one)
      "ldc_is_n_out"      the rows of C are taken n_out apart, not ldc
      "skip_after_empty"  the walk over the sources ends at the first empty one"""
    assert defect is None or defect in COMBINE_DEFECTS
    srcs = _sources(sources)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    ldc, flat = Cm.shape[1], Cm.reshape(-1)
    n6 = next(s.shape[1] for s in srcs if s is not None)
    Y = np.zeros((n_out, n6))
    for o in range(n_out):
        oc = o
        if defect == "swap_wave_e" and o >= 4:
            t = 4 * (o % 4) + o // 4
            oc = t if (o // 4 < 4 and t < n_out) else o
        acc, row0 = np.zeros(n6), 0
        for s in srcs:
            qk = 0 if s is None else len(s)
            if qk == 0 and defect == "skip_after_empty":
                break
            for c in range(qk):
                if defect == "drop_chunk_last" and c % CHUNK == CHUNK - 1:
                    continue
                cf = flat[row0 * ldc + c * n_out + oc] if defect == "ldc_is_n_out" else Cm[row0 + c, oc]
                acc = acc + s[c] * cf
            row0 += qk
        Y[o] = acc
    return Y


# ------------------------------------------------------------------ residual

# (mb, cols): one column, a non-monotonic subset and all columns of 12 and of 32
RESIDUAL_SHAPES = ((1, (0,)), (12, (5, 0, 11, 3)), (12, tuple(range(12))), (32, (31, 2, 17, 0, 9)), (32, tuple(range(32))))


def residual_defect_shows(defect, cols, n_nodes, n_pad):
    last = stretches(n_pad)[-1]
    return {"theta_i": tuple(cols) != tuple(range(len(cols))), "no_mask": True, "stretch_loses_last": True,
            "sum_misses_last": last[0] < min(last[1], n_nodes)}[defect]


RESIDUAL_DEFECTS = ("theta_i", "no_mask", "sum_misses_last", "stretch_loses_last")


def stretches(n_pad):
    """[(begin, end)] of the GRID workgroups, in nodes"""
    per = -(-n_pad // GRID)
    return [(min(b * per, n_pad), min((b + 1) * per, n_pad)) for b in range(GRID)]


def residual_truth(KX, X, theta, cols, mass, free):
    """(r (n, 6 n_nodes) in long double, the bound per entry)"""
    cols = np.asarray(cols, dtype=np.int64)
    kx, x = np.asarray(KX, dtype=np.float64)[cols].astype(LD), np.asarray(X, dtype=np.float64)[cols].astype(LD)
    th = np.asarray(theta, dtype=np.float64)[cols].astype(LD)[:, None]
    m = np.asarray(mass, dtype=np.float64).reshape(-1).astype(LD)[None, :]
    t = th * (m * x)
    r = np.where(free[None, :], kx - t, LD(0.0))
    bound = np.where(free[None, :], U * np.abs(r) + kt.gamma(2) * np.abs(t), LD(0.0)).astype(np.float64)
    return r, bound


def assert_residual_rows(R, KX, X, theta, cols, mass, free):
    r, bound = residual_truth(KX, X, theta, cols, mass, free)
    R = np.asarray(R, dtype=np.float64)
    assert R.shape == r.shape
    assert (bits(R[:, ~free]) == 0).all(), "a constrained dof of R is not +0.0"
    return within(R, r, bound)


def index_order_sum(partials):
    """the float64 sum of every row in index order"""
    p = np.asarray(partials, dtype=np.float64)
    s = np.zeros(len(p))
    for g in range(p.shape[1]):
        s = s + p[:, g]
    return s


def assert_residual_sums(norms, partials):
    assert_same_bits(norms, index_order_sum(partials), "norms against their partial sums")


def _terms(r, mass, free):
    """(hi, lo, counted): r^2 / m of every dof as two doubles (long double, split), zero where the dof does not count"""
    m = np.asarray(mass, dtype=np.float64).reshape(-1)
    counted = free & (m > 0.0)
    t = np.where(counted, np.asarray(r).astype(LD) ** 2 / np.where(counted, m, 1.0).astype(LD), LD(0.0))
    hi = t.astype(np.float64)
    return hi, (t - hi.astype(LD)).astype(np.float64), counted


def assert_residual_partials(partials, R, mass, free, n_pad):
    """every partial sum against the exact sum over its stretch of the device's own R; returns the largest share of the bound"""
    R = np.asarray(R, dtype=np.float64)
    partials = np.asarray(partials, dtype=np.float64)
    assert partials.shape == (len(R), GRID)
    n_nodes = R.shape[1] // 6
    want, bound = np.zeros(partials.shape), np.zeros(partials.shape)
    for i in range(len(R)):
        hi, lo, counted = _terms(R[i], mass, free)
        for b, (s, e) in enumerate(stretches(n_pad)):
            s6, e6 = 6 * min(s, n_nodes), 6 * min(e, n_nodes)
            n = int(counted[s6:e6].sum())
            want[i, b] = math.fsum(hi[s6:e6].tolist() + lo[s6:e6].tolist())
            bound[i, b] = (kt.gamma(max(n, 1)) + 2.0 * U) * want[i, b]
    empty = bound == 0.0
    assert (bits(partials[empty]) == 0).all(), "a workgroup without counted rows left something other than +0.0"
    return within(partials, want.astype(LD), bound)


def assert_residual_norms(norms, KX, X, theta, cols, mass, free, n_pad):
    """end to end: the norms against those of the truth residual"""
    r, b = residual_truth(KX, X, theta, cols, mass, free)
    m = np.asarray(mass, dtype=np.float64).reshape(-1)
    counted = free & (m > 0.0)
    md = np.where(counted, m, 1.0).astype(LD)[None, :]
    want = np.where(counted[None, :], r * r / md, LD(0.0)).sum(axis=1)
    carried = np.where(counted[None, :], (2.0 * np.abs(r) * b + b.astype(LD) ** 2) / md, LD(0.0)).sum(axis=1)
    n_terms = max(int(counted[6 * s:6 * e].sum()) for s, e in stretches(n_pad))
    g = (kt.gamma(max(n_terms, 1)) + 2.0 * U + kt.gamma(GRID)) * (1.0 + 1e-10)
    bound = (carried + g * (want + carried)).astype(np.float64)
    return within(norms, want, bound)


def residual_model(KX, X, theta, cols, mass, free, n_pad, defect=None):
    """(R, norms, partials) of k_block_residual and k_block_residual_sums in float64, uncontracted.  defect: None, or
      "theta_i"             column i is taken with theta[i], not theta[cols[i]]
      "no_mask"             constrained dofs keep kx - theta m x
      "sum_misses_last"     the sums stop one partial short
      "stretch_loses_last"  every workgroup's stretch ends one node early"""
    assert defect is None or defect in RESIDUAL_DEFECTS
    cols = np.asarray(cols, dtype=np.int64)
    KX, X = np.asarray(KX, dtype=np.float64), np.asarray(X, dtype=np.float64)
    theta, m = np.asarray(theta, dtype=np.float64), np.asarray(mass, dtype=np.float64).reshape(-1)
    n_nodes = len(m) // 6
    th = theta[np.arange(len(cols))] if defect == "theta_i" else theta[cols]
    R = KX[cols] - th[:, None] * (m[None, :] * X[cols])
    if defect != "no_mask":
        R = np.where(free[None, :], R, 0.0)
    counted = free & (m > 0.0)
    terms = np.where(counted[None, :], R * R / np.where(counted, m, 1.0)[None, :], 0.0)
    partials = np.zeros((len(cols), GRID))
    for b, (s, e) in enumerate(stretches(n_pad)):
        if defect == "stretch_loses_last":
            e = max(e - 1, s)
        partials[:, b] = terms[:, 6 * min(s, n_nodes):6 * min(e, n_nodes)].sum(axis=1)
    norms = index_order_sum(partials[:, :GRID - 1] if defect == "sum_misses_last" else partials)
    return R, norms, partials


# ------------------------------------------------------------------ block-Jacobi, mask

BJ_DEFECTS = ("wrong_transposed_word", "no_mask")


def bj_truth(Dinv, R, free):
    """(truth (n, 6 n_nodes), bound): Dinv [n_nodes, 6, 6] as block_jacobi_export(level=0) gives it"""
    Dinv = np.asarray(Dinv, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    n_nodes = len(Dinv)
    r = R.reshape(len(R), n_nodes, 6)
    A = Dinv.transpose(2, 0, 1)[:, None, :, :]  # [j, 1, node, i]
    B = r.transpose(2, 0, 1)[:, :, :, None]     # [j, col, node, 1]
    A, B = np.broadcast_arrays(A, B)
    truth = exact_dots(A, B).reshape(len(R), -1)
    scale = np.abs(A.astype(LD) * B.astype(LD)).sum(axis=0).reshape(len(R), -1)
    bound = (kt.gamma(6) * scale + U * np.abs(truth)).astype(np.float64)
    truth = np.where(free[None, :], truth, 0.0)
    return truth, np.where(free[None, :], bound, 0.0)


def assert_block_jacobi(Z, Dinv, R, free):
    truth, bound = bj_truth(Dinv, R, free)
    Z = np.asarray(Z, dtype=np.float64)
    assert Z.shape == truth.shape
    assert (bits(Z[:, ~free]) == 0).all(), "a constrained dof of Z is not +0.0"
    return within(Z, truth.astype(LD), bound)


def bj_model(Dinv, R, free, defect=None):
    """k_block_bj in float64: per row j ascending from zero.  defect: None, or
      "wrong_transposed_word"  entry (4, 2), below the diagonal, is read from the word of (2, 3), not of (2, 4)
      "no_mask"                constrained dofs keep their value"""
    assert defect is None or defect in BJ_DEFECTS
    D = np.array(Dinv, dtype=np.float64)
    if defect == "wrong_transposed_word":
        D[:, 4, 2] = D[:, 2, 3]
    R = np.asarray(R, dtype=np.float64)
    r = R.reshape(len(R), len(D), 6)
    z = np.zeros_like(r)
    for j in range(6):
        z = z + D[None, :, :, j] * r[:, :, j][:, :, None]
    z = z.reshape(len(R), -1)
    return z if defect == "no_mask" else np.where(free[None, :], z, 0.0)


def assert_mask(Y, X, free):
    assert_same_bits(Y, np.where(free[None, :], np.asarray(X, dtype=np.float64), 0.0), "mask")


# ------------------------------------------------------------------ start vectors

START_DEFECTS = ("internal_id", "column_inside")
M64 = (1 << 64) - 1
COLUMN_KEY = 0xD1B54A32D192ED03


def splitmix64(x):
    """Python integers"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def splitmix64_np(x):
    """the same on numpy's uint64, which wraps"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def start_value(h):
    """the kernel's mapping of a hash (Python integer) in float64"""
    u01 = (float(h >> 11) + 0.5) * 2.0 ** -53
    return 2.0 * u01 - 1.0


def start_entry(node, dof, col):
    """one entry by Python integers alone"""
    return start_value(splitmix64(splitmix64(node * 6 + dof) ^ ((col * COLUMN_KEY) & M64)))


def start_model(n_nodes, free, n_cols, internal_of=None, defect=None):
    """k_modal_init in the caller's numbering: X (n_cols, 6 n_nodes).  internal_of[a]: the library's id of the caller's node a
    (None: the same) -- only the defect "internal_id" looks at it.  defect: None, or
      "internal_id"    the library's node id is hashed, not the caller's
      "column_inside"  the column key goes into the inner hash: splitmix64(splitmix64((6 id + dof) ^ col key))"""
    assert defect is None or defect in START_DEFECTS
    ids = np.arange(n_nodes, dtype=np.uint64)
    if defect == "internal_id":
        ids = np.asarray(internal_of, dtype=np.uint64)
    cell = (ids[:, None] * np.uint64(6) + np.arange(6, dtype=np.uint64)[None, :]).reshape(-1)
    with np.errstate(over="ignore"):
        key = np.arange(n_cols, dtype=np.uint64) * np.uint64(COLUMN_KEY)
    if defect == "column_inside":
        h = splitmix64_np(splitmix64_np(cell[None, :] ^ key[:, None]))
    else:
        h = splitmix64_np(splitmix64_np(cell)[None, :] ^ key[:, None])
    u01 = ((h >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return np.where(free[None, :], 2.0 * u01 - 1.0, 0.0)


def assert_start(X, free, n_cols):
    X = np.asarray(X, dtype=np.float64)
    want = start_model(X.shape[1] // 6, free, n_cols)
    assert_same_bits(X, want, "start vectors")
    assert (np.abs(X[:, free]) < 1.0).all() and (X[:, free] != 0.0).all(), "a start value outside (-1, 1) or zero"
