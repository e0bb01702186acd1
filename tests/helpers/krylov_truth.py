"""The layer that drives every operator of the solve phase -- the three Krylov recurrences (cg_classic, cg_single_reduction of
csrc/cg_driver.cpp, the flexible PCG of cg_amg), their vector kernels and fused dot products, the two-stage reduction k_cg_scalar
and the scalar state machine cg_scalar_phase (csrc/cg_kernels.hip) -- against an exact truth: the truths, the bounds, a
restatement of the scalar phases that the device must match bit for bit, models that take planted defects, and the assertions
the GPU tests (tests/test_gpu_krylov_truth.py) and the CPU pins (tests/test_krylov_truth_cpu.py) share.  numpy and the standard
library only.

exact_dot      the correctly rounded a.b: every product as an error-free pair (residual_truth.two_product), all of them through
               math.fsum, which is exact and rounds once.
dot_bound      gamma_n sum |a_i b_i|, gamma_n = n u / (1 - n u), u = 2^-53: the bound of a recursive or pairwise FP64 dot product
               of n terms in ANY order, fused or not (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5).
               n is the number of terms that can meet in one accumulation chain plus the tree above it; the crude n = len(a)
               holds for every order.  What the tests compare carries two roundings more -- the fsum of the device's partial sums
               rounds once, and so does the truth -- and the chains that really meet (the slices one workgroup walks, six words a
               node, a wave tree of six levels, three or four wave sums) are shorter than len(a) - 2 on every mesh used (198 words
               at the least), so the crude n covers them.  Derived, not measured.
axpy_bound     x + alpha p in long double; the device may or may not contract the product into the sum: u (|result| + |alpha p|)
               covers both (contracted: one rounding of the result; not: one of the product, one of the sum).
scalar_phase   cg_scalar_phase in numpy doubles, folded_step the copy of it inside k_cgcg_update.  The phases use + - * / sqrt fmax
               fmin only and no expression offers a contraction (no product feeds an addition: zaz - beta * rzn / alpha divides the
               product first), divisions and square roots are correctly rounded on both sides: device and restatement agree bit
               for bit.
reduce_model   the two-stage order of k_cg_scalar: chunks, the lane's strided chain of four loads in flight, the wave tree of
               __shfl_down, the wave sums in index order, then the same over the stage-1 sums.
"""
import math

import numpy as np

from tests.helpers import residual_truth as rt

U = rt.U
LD = np.longdouble

# CgPhase of csrc/kernels.hpp
NONE, INIT, ALPHA, BETA, RESTART, FUSED_INIT, FUSED_STEP = 0, 1, 2, 3, 4, 5, 6
FLEX_INIT, FLEX_RZ0, FLEX_CONV, FLEX_BETA, FLEX_RESTART, FLEX_WARM = 7, 8, 9, 10, 11, 12
PHASES = {"none": NONE, "init": INIT, "alpha": ALPHA, "beta": BETA, "restart": RESTART, "fused_init": FUSED_INIT,
          "fused_step": FUSED_STEP, "flex_init": FLEX_INIT, "flex_rz0": FLEX_RZ0, "flex_conv": FLEX_CONV, "flex_beta": FLEX_BETA,
          "flex_restart": FLEX_RESTART, "flex_warm": FLEX_WARM}
# the phases whose launch also runs on a finished solve (k_cg_scalar's gate rule)
UNGATED = (INIT, RESTART, FUSED_INIT, FLEX_INIT, FLEX_RESTART, FLEX_WARM)
REDUCE_GROUPS, REDUCE_THRESHOLD = 64, 4096  # kReduceGroups; launch_cg_scalar: G >= 4096 partial sums take 64 workgroups
REFINE_DROP, REFINE_TARGET, REFINE_DROP_MIN, REFINE_DROP_MAX = 1.0e-4, 0.2, 1.0e-6, 1.0e-2

F64 = np.float64


# ------------------------------------------------------------------ truths and bounds

def exact_dot(a, b):
    """the correctly rounded sum of a_i b_i"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape
    p, e = rt.two_product(a, b)
    return math.fsum(p.tolist() + e.tolist())


def exact_sum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def gamma(n):
    return float(rt.gamma(n))


def abs_dot(a, b):
    """sum |a_i b_i|, in long double and rounded once"""
    return float(np.abs(np.asarray(a, dtype=np.float64).reshape(-1).astype(LD) * np.asarray(b, dtype=np.float64).reshape(-1).astype(LD)).sum())


def dot_bound(a, b, n=None):
    n = np.asarray(a).size if n is None else n
    return gamma(max(int(n), 1)) * abs_dot(a, b)


def sum_bound(partials):
    """|red - exact| <= gamma_len sum |partials|: a sum of len terms in any order"""
    p = np.asarray(partials, dtype=np.float64).reshape(-1)
    return gamma(max(p.size, 1)) * float(np.abs(p.astype(LD)).sum())


def axpy_truth(x, alpha, p):
    """(x + alpha p in long double, u (|result| + |alpha p|))"""
    ap = LD(alpha) * np.asarray(p, dtype=np.float64).astype(LD)
    want = np.asarray(x, dtype=np.float64).astype(LD) + ap
    return want, U * (np.abs(want) + np.abs(ap))


def axpy_bound(x, alpha, p):
    return axpy_truth(x, alpha, p)[1]


def within(got, want, bound):
    """every entry of got within its bound of want (long double); returns the largest share of a bound used"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
    bad = err > bound
    assert not bad.any(), "entry %d: error %.3e, bound %.3e" % (int(np.flatnonzero(bad.reshape(-1))[0]), float(err[bad].max()), float(np.asarray(bound)[bad].min()))
    pos = np.asarray(bound) > 0
    return float((err[pos] / np.asarray(bound)[pos]).max()) if pos.any() else 0.0


def fused_dot_truth(K, x):
    """(exact_dot(x, K x) with K x the correctly rounded rows of the exported matrix, the bound of the product's fused dot).
    The kernels form y_i (or its direct part and the transposed products beside it) from up to 6 nb_i products, nb_i the blocks of
    row i, and then a dot product over the rows: |device - x.Kx| <= (gamma_{6 nb} + gamma_n (1 + gamma_{6 nb})) S with
    S = sum_i |x_i| (|K||x|)_i, nb the longest row and n = len(x); the truth's two roundings (of K x, of the dot) add 2 u S."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    Kx = -rt.exact(K, np.zeros_like(x), x)
    truth = exact_dot(x, Kx)
    S = float((np.abs(x).astype(LD) * rt.scale(K, np.zeros_like(x), x).astype(LD)).sum())
    g_row = gamma(6.0 * float(rt.blocks_per_row(K).max()))
    return truth, (g_row + gamma(x.size) * (1.0 + g_row) + 2.0 * U) * S


# ------------------------------------------------------------------ the assertions the GPU tests and the planted defects share

def assert_reduction_exact(red, partials, label=""):
    """integer-valued partial sums: red equals the exact integer, bit for bit -- and the difference names what was lost or doubled"""
    want = exact_sum(partials)
    assert want == float(int(want)) and abs(want) < 2.0 ** 53
    assert red == want, "%s: red = %r, exact %r: difference %r" % (label, red, want, red - want)


def assert_reduction_within(red, partials, label=""):
    want, bound = exact_sum(partials), sum_bound(partials)
    assert abs(red - want) <= bound, "%s: |%r - %r| = %.3e > %.3e" % (label, red, want, abs(red - want), bound)
    return abs(red - want) / bound if bound > 0 else 0.0


def assert_dot(partials, a, b, label="", exact=False, truth=None, bound=None):
    """the fsum of a kernel's partial sums against exact_dot of the vectors it read (exact: integer-valued inputs, bit for bit);
    truth and bound: those of fused_dot_truth, for a product's fused dot, in place of exact_dot(a, b) and dot_bound(a, b);
    returns the share of the bound used"""
    got = exact_sum(partials)
    want = exact_dot(a, b) if truth is None else truth
    if exact:
        assert got == want, "%s: partial sums add to %r, the exact dot is %r" % (label, got, want)
        return 0.0
    bound = dot_bound(a, b) if bound is None else bound
    assert abs(got - want) <= bound, "%s: |%r - %r| = %.3e > %.3e" % (label, got, want, abs(got - want), bound)
    return abs(got - want) / bound if bound > 0 else 0.0


SCALAR_FIELDS = ("rz", "alpha", "beta", "rr", "bb", "tol2", "done", "iters", "pass_xx", "pass_rhs_rr", "pass_rtol")


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def assert_scalars_equal(got, want, label="", fields=SCALAR_FIELDS + ("red", "ring_rz", "ring_alpha")):
    """two Scalars, field by field, bit for bit (NaN equals NaN of the same bits)"""
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        if f in ("done", "iters"):
            assert int(g) == int(w), "%s: %s = %r, restated %r" % (label, f, g, w)
        else:
            assert np.array_equal(bits(g), bits(w)), "%s: %s = %r, restated %r" % (label, f, g, w)


# ------------------------------------------------------------------ the scalar state machine

class Scalars:
    """CgScalars without the words of the reduction"""

    def __init__(self, **kw):
        self.rz = self.alpha = self.beta = self.rr = self.bb = self.tol2 = F64(0.0)
        self.red = np.zeros(3)
        self.done = 0
        self.iters = 0
        self.ring_rz = np.zeros(2)
        self.ring_alpha = np.zeros(2)
        self.pass_xx = self.pass_rhs_rr = self.pass_rtol = F64(0.0)
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, np.array(v, dtype=np.float64) if k in ("red", "ring_rz", "ring_alpha") else (int(v) if k in ("done", "iters") else F64(v)))

    def copy(self):
        out = Scalars()
        for k, v in self.__dict__.items():
            setattr(out, k, v.copy() if isinstance(v, np.ndarray) else v)
        return out

    @classmethod
    def from_struct(cls, st):
        out = cls()
        for f in SCALAR_FIELDS:
            setattr(out, f, int(getattr(st, f)) if f in ("done", "iters") else F64(getattr(st, f)))
        out.red, out.ring_rz, out.ring_alpha = np.array(st.red[:]), np.array(st.ring_rz[:]), np.array(st.ring_alpha[:])
        return out

    def into_struct(self, st):
        for f in SCALAR_FIELDS:
            setattr(st, f, int(getattr(self, f)) if f in ("done", "iters") else float(getattr(self, f)))
        for f in ("red", "ring_rz", "ring_alpha"):
            for i, v in enumerate(getattr(self, f)):
                getattr(st, f)[i] = float(v)
        return st


def gated(gate_phase, done):
    """k_cg_scalar returns at once: a launch that belongs to a gated phase on a finished (or broken) solve"""
    return gate_phase not in UNGATED and done != 0


def _fmax(a, b):  # C fmax / fmin: the number, when one side is NaN
    return b if a != a else (a if b != b else (a if a >= b else b))


def _fmin(a, b):
    return b if a != a else (a if b != b else (a if a <= b else b))


def _record(s, rr, hist, hist_cap):
    s.rr = rr
    s.iters = s.iters + 1
    if hist is not None and s.iters <= hist_cap:
        hist[s.iters - 1] = rr / s.bb


def scalar_phase(phase, s, rtol, hist=None, hist_cap=0):
    """cg_scalar_phase(v, phase, rtol) on the Scalars s (changed in place and returned); hist: the history words (an array,
    changed in place) with their cap, or None for the null pointer"""
    rtol = F64(rtol)
    r0, r1, r2 = (F64(v) for v in s.red)
    zero = F64(0.0)
    with np.errstate(all="ignore"):
        if phase == INIT:
            s.rz, s.bb, s.rr = r0, r1, r1
            s.tol2 = rtol * rtol * r1 if rtol > 0.0 else zero
            s.alpha = s.beta = zero
            s.iters = 0
            s.done = 1 if r1 == 0.0 else 0
        elif phase == RESTART:
            s.rz, s.rr = r0, r1
            s.done = 1 if r1 <= s.tol2 else 0
        elif phase == ALPHA:
            if not r0 > 0.0:
                s.done = -1
            else:
                s.alpha = s.rz / r0
        elif phase == FUSED_INIT:
            s.rz, s.bb, s.rr = r0, r1, r1
            s.tol2 = rtol * rtol * r1 if rtol > 0.0 else zero
            s.beta = s.alpha = zero
            s.iters = 0
            s.done = 1 if r1 == 0.0 else 0
            if s.done == 0:
                if not r2 > 0.0:
                    s.done = -1
                else:
                    s.alpha = r0 / r2
            s.ring_rz[0] = s.rz
            s.ring_alpha[0] = s.alpha
        elif phase == FUSED_STEP:
            _record(s, r1, hist, hist_cap)
            if r1 <= s.tol2:
                s.done = 1
            else:
                beta = r0 / s.rz
                denom = r2 - beta * r0 / s.alpha
                if not denom > 0.0:
                    s.done = -1
                else:
                    s.beta, s.alpha, s.rz = beta, r0 / denom, r0
        elif phase == FLEX_INIT:
            s.pass_xx = s.pass_rhs_rr = zero
            s.bb = s.rr = r0
            s.tol2 = rtol * rtol * r0 if rtol > 0.0 else zero
            s.alpha = s.beta = s.rz = zero
            s.iters = 0
            s.done = 1 if r0 == 0.0 else 0
        elif phase == FLEX_RESTART:
            s.rr = r0
            s.alpha = s.beta = s.rz = zero
            tol2_solve = rtol * rtol * s.bb if rtol > 0.0 else zero
            s.done = 1 if r0 <= tol2_solve else 0
            s.tol2 = _fmax(tol2_solve, F64(REFINE_DROP) * F64(REFINE_DROP) * r0)
            s.pass_rhs_rr = r0
        elif phase == FLEX_WARM:
            s.rr = r0
            s.done = 1 if r0 <= s.tol2 else 0
        elif phase == FLEX_RZ0:
            s.rz = r0
            if not r0 > 0.0:
                s.done = -1
        elif phase == FLEX_CONV:
            _record(s, r0, hist, hist_cap)
            if s.pass_xx > 0.0 and s.pass_rhs_rr > 0.0 and r1 > 0.0:
                drop = F64(REFINE_TARGET) * s.pass_rtol * np.sqrt(s.pass_xx / r1)
                d = _fmin(_fmax(drop, F64(REFINE_DROP_MIN)), F64(REFINE_DROP_MAX))
                s.tol2 = d * d * s.pass_rhs_rr
            if r0 <= s.tol2:
                s.done = 1
        elif phase == FLEX_BETA:
            if not r0 > 0.0:
                s.done = -1
            else:
                s.beta = -s.alpha * r1 / s.rz
                s.rz = r0
        elif phase == BETA:
            _record(s, r1, hist, hist_cap)
            if r1 <= s.tol2:
                s.done = 1
            else:
                s.beta = r0 / s.rz
                s.rz = r0
        else:
            assert phase == NONE, phase
    return s


FOLD_DEFECTS = ("wrong_parity",)


def folded_step(s, step, hist=None, hist_cap=0, defect=None):
    """The scalar step inside k_cgcg_update(step >= 0): every workgroup derives (alpha, beta, done) from red[] and ring[step & 1],
    workgroup 0 publishes them and writes ring[(step & 1) ^ 1].  Returns (alpha, beta, done) as the vector part of the kernel uses
    them; s is changed in place.  A launch on done != 0 is a no-op: (None, None, done).
    defect "wrong_parity": the previous (r.z, alpha) are read from the other half of the ring."""
    assert defect is None or defect in FOLD_DEFECTS
    if s.done != 0:
        return None, None, s.done
    par = step & 1
    rd = par ^ 1 if defect == "wrong_parity" else par
    rz_old, alpha_old = F64(s.ring_rz[rd]), F64(s.ring_alpha[rd])
    rzn, rr, zaz = (F64(v) for v in s.red)
    done, alpha, beta = 0, F64(0.0), F64(0.0)
    with np.errstate(all="ignore"):
        if rr <= s.tol2:
            done = 1
        else:
            beta = rzn / rz_old
            denom = zaz - beta * rzn / alpha_old
            if not denom > 0.0:
                done = -1
            else:
                alpha = rzn / denom
        _record(s, rr, hist, hist_cap)
    if done == 0:
        s.beta, s.alpha, s.rz = beta, alpha, rzn
        s.ring_rz[par ^ 1] = rzn
        s.ring_alpha[par ^ 1] = alpha
    s.done = done
    return alpha, beta, done


# ------------------------------------------------------------------ the two-stage reduction

REDUCE_DEFECTS = ("drop_last_chunk",)


def _block_sum(v):
    """block_sum of device_common.hpp over 256 lanes: the __shfl_down tree of every wave, the four wave sums in index order"""
    w = np.array(v, dtype=np.float64).reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w[:, :64 - off] = w[:, :64 - off] + w[:, off:]  # (lanes whose partner is beyond the wave keep a value nobody reads)
    t = F64(0.0)
    for i in range(4):
        t = t + w[i, 0]
    return t


def reduce_groups(n_partials):
    return REDUCE_GROUPS if n_partials >= REDUCE_THRESHOLD else 1


def reduce_model(partials, n_groups=None, defect=None):
    """k_cg_scalar's sum of one partial array, operation by operation: n_groups workgroups of 256 lanes take contiguous chunks of
    ceil(len / n_groups); lane t adds the words lo + t + 256 q (+ 1024 per round), four at a time in index order; the workgroup's
    block_sum is the stage-1 sum, and the block_sum over the stage-1 sums (lane g holds group g's, the others zero) is red.
    defect "drop_last_chunk": the last workgroup's stage-1 sum never arrives."""
    assert defect is None or defect in REDUCE_DEFECTS
    p = np.asarray(partials, dtype=np.float64).reshape(-1)
    n = p.size
    nwg = reduce_groups(n) if n_groups is None else n_groups
    chunk = (n + nwg - 1) // nwg
    stage = np.zeros(256)
    for g in range(nwg):
        lo, hi = g * chunk, min(n, g * chunk + chunk)
        acc = np.zeros(256)
        for base in range(lo, hi, 1024):
            for q in range(4):
                idx = base + 256 * q + np.arange(256)
                acc = acc + np.where(idx < hi, p[np.minimum(idx, n - 1)], 0.0)
        stage[g] = _block_sum(acc)
    if defect == "drop_last_chunk":
        stage[nwg - 1] = 0.0
    return float(_block_sum(stage))


# ------------------------------------------------------------------ models of the fused dots, for the planted defects

DOT_DEFECTS = ("in_slice_twice", "ghost_row")


def sym_fused_dot_model(K, x, defect=None, slice_nodes=32):
    """k_spmv_sym's identity x.Kx = sum_a x_a.(direct y_a) + sum over stored off-diagonal blocks (a, c), c > a, of x_c.u with
    u = K_ac^T x_a, in long double (the order of the device's sum is not the point here).
    defect "in_slice_twice": the products whose row c lies in the slice of a are counted when they are formed AND when they join
    the direct part at the end of the slice."""
    assert defect is None or defect in DOT_DEFECTS
    rowptr, colidx, vals = (np.asarray(a) for a in K[:3])
    vals = vals.reshape(-1, 6, 6).astype(LD)
    x6 = np.asarray(x, dtype=np.float64).reshape(-1, 6).astype(LD)
    total = LD(0.0)
    for a in range(len(rowptr) - 1):
        for q in range(rowptr[a], rowptr[a + 1]):
            c = int(colidx[q])
            if c < a:
                continue  # not stored: the row takes it from the transposed block of (c, a)
            total += x6[a] @ (vals[q] @ x6[c])
            if c > a:
                u = vals[q].T @ x6[a]
                total += x6[c] @ u
                if defect == "in_slice_twice" and c // slice_nodes == a // slice_nodes:
                    total += x6[c] @ u
    return float(total)


def owned_dot_model(a, b, n_owned, defect=None):
    """a.b over the owned rows (six words a node) of vectors that carry ghost rows behind them; defect "ghost_row": one ghost row
    is counted too"""
    assert defect is None or defect in DOT_DEFECTS
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    n = 6 * (n_owned + (1 if defect == "ghost_row" else 0))
    return float((a[:n].astype(LD) * b[:n].astype(LD)).sum())


# ------------------------------------------------------------------ the recurrences, restated from scalar_phase

def _dots(*pairs):
    out = np.zeros(3)
    for i, (a, b) in enumerate(pairs):
        out[i] = a @ b
    return out


def classic(A, Minv, b, rtol, max_it):
    """cg_classic: (x, history of r.r / b.b, Scalars).  A: anything with @; Minv: r -> z.  Every vector kernel is a no-op once
    done != 0, as on the device."""
    s, hist = Scalars(), np.zeros(max(max_it, 1))
    x, r = np.zeros_like(b), b.copy()
    z = Minv(r)
    p = z.copy()
    s.red = _dots((r, z), (r, r))
    scalar_phase(INIT, s, rtol)
    for _ in range(max_it):
        if s.done != 0:
            break
        q = A @ p
        s.red[0] = p @ q
        scalar_phase(ALPHA, s, rtol)
        if s.done != 0:
            break
        x = x + s.alpha * p
        r = r - s.alpha * q
        z = Minv(r)
        s.red[:2] = (r @ z, r @ r)
        scalar_phase(BETA, s, rtol, hist, len(hist))
        if s.done == 0:
            p = z + s.beta * p
    return x, hist[:s.iters], s


def single_reduction(A, Minv, b, rtol, max_it, fold=True, defect=None):
    """cg_single_reduction (Chronopoulos and Gear): fold -- the scalar step of iteration k is taken inside the update kernel of
    iteration k + 1 (folded_step, ring parity (k - 1) & 1 ... ), and a FUSED_STEP launch closes the last iteration"""
    s, hist = Scalars(), np.zeros(max(max_it, 1))
    x, r = np.zeros_like(b), b.copy()
    z = Minv(r)
    p, sv = np.zeros_like(b), np.zeros_like(b)
    w = A @ z
    s.red = _dots((r, z), (r, r), (z, w))
    scalar_phase(FUSED_INIT, s, rtol)
    open_step = False
    for it in range(max_it):
        if fold and it > 0:
            folded_step(s, (it - 1) & 1, hist, len(hist), defect=defect)
            open_step = False
        if s.done != 0:
            break
        p = z + s.beta * p
        sv = w + s.beta * sv
        x = x + s.alpha * p
        r = r - s.alpha * sv
        z = Minv(r)
        w = A @ z
        s.red = _dots((r, z), (r, r), (z, w))
        if fold:
            open_step = True
        else:
            scalar_phase(FUSED_STEP, s, rtol, hist, len(hist))
    if open_step and s.done == 0:
        scalar_phase(FUSED_STEP, s, rtol, hist, len(hist))
    return x, hist[:s.iters], s


def flexible(A, M, b, rtol, max_it):
    """the flexible PCG of cg_amg without refinement passes: M: r -> z, any preconditioner"""
    s, hist = Scalars(), np.zeros(max(max_it, 1))
    x, r = np.zeros_like(b), b.copy()
    s.red[0] = b @ b
    scalar_phase(FLEX_INIT, s, rtol)
    if s.done != 0:
        return x, hist[:0], s
    z = M(r)
    s.red[0] = r @ z
    scalar_phase(FLEX_RZ0, s, rtol)
    p = z.copy()
    for _ in range(max_it):
        if s.done != 0:
            break
        q = A @ p
        s.red[0] = p @ q
        scalar_phase(ALPHA, s, rtol)
        if s.done != 0:
            break
        x = x + s.alpha * p
        r = r - s.alpha * q
        s.red[:2] = (r @ r, x @ x)
        scalar_phase(FLEX_CONV, s, rtol, hist, len(hist))
        if s.done != 0:
            break
        z = M(r)
        s.red[:2] = (r @ z, z @ q)
        scalar_phase(FLEX_BETA, s, rtol)
        if s.done == 0:
            p = z + s.beta * p
    return x, hist[:s.iters], s


# ------------------------------------------------------------------ input makers

def integer_partials(n):
    """partials[i] = i + 1: every sum of them is exact in every order (n (n + 1) / 2 < 2^53), and a lost or doubled entry shows
    as its own index + 1"""
    return np.arange(1, n + 1, dtype=np.float64)


def small_integers(rng, shape, top=3):
    """small-integer words: dots and, with alpha = 1, updates of them are exact in every order"""
    return rng.integers(-top, top + 1, size=shape).astype(np.float64)


def random_partials(rng, n):
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 3.0, size=n)


def cancelling(rng, n):
    """words whose exact sum is about 1e-12 of the sum of their magnitudes: pairs (v, -v) in random places and a small rest"""
    v = rng.standard_normal(n // 2) * 10.0 ** rng.uniform(-1.0, 1.0, size=n // 2)
    out = np.concatenate([v, -v, np.zeros(n - 2 * (n // 2))])
    out[-1] += 1.0e-12 * float(np.abs(out).sum()) if n > 1 else 1.0
    return out[rng.permutation(n)] if n > 2 else out


def one_hot(n, i):
    out = np.zeros(n)
    out[i] = 1.0
    return out


def chunk_edges(n):
    """the indices at both sides of every chunk boundary of the reduction of n words, with 0 and n - 1"""
    nwg = reduce_groups(n)
    chunk = (n + nwg - 1) // nwg
    edges = {0, n - 1}
    for g in range(1, nwg):
        for i in (g * chunk - 1, g * chunk):
            if 0 <= i < n:
                edges.add(i)
    return sorted(edges)


REDUCE_LENGTHS = (1, 7, 8, 255, 256, 257, 1024, 4095, 4096, 4097, 8232, 65536)
