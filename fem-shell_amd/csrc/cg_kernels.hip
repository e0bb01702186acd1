// cg_kernels.hip -- vector and scalar kernels of the conjugate-gradient solves (cg_driver.cpp): the block-Jacobi steps of the
// classic and of the single-reduction recurrence, the two-stage reduction with the scalar step, and the halo pack.
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "kernels assume 32-node slices");

// =====================================================================================
// CG vector kernels (one lane per scalar row and one workgroup per slice, unless named _node)
// =====================================================================================

__global__ __launch_bounds__(192) void k_cg_init(DeviceMatrix m, CgVectors v, int restart)
{
    __shared__ double rs[kSliceRows];
    __shared__ double sh[3];
    const int G = gridDim.x, t = threadIdx.x;
    double d0 = 0.0, d1 = 0.0;
    for (SliceWalk w(m.n_slices); w.valid(); w.next()) {
        const int sl = w.s;
        const int64_t row = (int64_t)sl * kSliceRows + t;
        const MinvRow mr = load_minv(m, sl, t);
        const double bv = restart ? v.b[row] - v.q[row] : v.b[row]; // the residual to start from
        __syncthreads();
        rs[t] = bv;
        __syncthreads();
        const double z = apply_minv(mr, t, rs);
        if (!restart) v.x[row] = 0.0;
        v.r[row] = bv;
        v.z[row] = z;
        v.p[row] = z;
        d0 += bv * z;
        d1 += bv * bv;
    }
    const double t0 = block_sum(d0, sh);
    const double t1 = block_sum(d1, sh);
    if (threadIdx.x == 0) {
        v.partials[blockIdx.x] = t0;
        v.partials[G + blockIdx.x] = t1;
    }
}

void launch_cg_init(const DeviceMatrix &m, const CgVectors &v, bool restart, hipStream_t st)
{
    hipLaunchKernelGGL(k_cg_init, dim3(slice_grid(m)), dim3(192), 0, st, m, v, restart ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_copy(const double2 *src, double2 *dst, int64_t n2)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

void launch_copy_x_to_p(const DeviceMatrix &m, const CgVectors &v, hipStream_t st)
{
    const int64_t n2 = (int64_t)m.n_pad * 3;
    const int64_t blocks = (n2 + 255) / 256;
    hipLaunchKernelGGL(k_copy, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st,
                       reinterpret_cast<const double2 *>(v.x), reinterpret_cast<double2 *>(v.p), n2);
}

// x += alpha p ; r -= alpha q ; z = M^-1 r ; partial sums of r.z and r.r.  One lane per node (device_common.hpp): no LDS, no
// barrier (launched with the grid of the per-slice kernels: the scalar step reduces slice_grid(m) partial sums per array)
// (kGather: symmetric storage, q holds the direct part of K p only; the node adds the transposed products of its in-list here
// instead of in a k_sym_gather_node pass of its own -- one read and one write of q and a launch less)
template <bool kGather>
__global__ __launch_bounds__(64) void k_cg_update_node(DeviceMatrix m, CgVectors v)
{
    if (v.s->done != 0) return;
    const int G = gridDim.x, half = threadIdx.x >> 5, n = threadIdx.x & 31;
    const double alpha = v.s->alpha;
    double d0 = 0.0, d1 = 0.0;
    for (SliceWalk w(node_pairs(m.n_slices)); w.valid(); w.next()) {
        const int sl = 2 * w.s + half;
        if (sl >= m.n_slices) continue;
        const int64_t node = (int64_t)sl * kSliceNodes + n;
        double mv[kMinvWords], pv[6], xv[6], rv[6], qv[6], z[6];
        node_minv(m, sl, n, false, mv);
        load_node6(v.p, node, false, pv);
        load_node6(v.x, node, false, xv);
        load_node6(v.r, node, false, rv);
        load_node6(v.q, node, false, qv);
        if (kGather) node_gather<false>(m, sl, n, qv);
#pragma unroll
        for (int j = 0; j < 6; j++) {
            xv[j] = xv[j] + alpha * pv[j];
            rv[j] = rv[j] - alpha * qv[j];
        }
        store_node6(v.x, node, false, xv);
        store_node6(v.r, node, false, rv);
        node_minv_apply(mv, rv, z);
        store_node6(v.z, node, false, z);
#pragma unroll
        for (int j = 0; j < 6; j++) {
            d0 += rv[j] * z[j];
            d1 += rv[j] * rv[j];
        }
    }
    const double t0 = wave_sum(d0), t1 = wave_sum(d1);
    if (threadIdx.x == 0) {
        v.partials[blockIdx.x] = t0;
        v.partials[G + blockIdx.x] = t1;
    }
}

void launch_cg_update(const DeviceMatrix &m, const CgVectors &v, hipStream_t st, bool gather)
{
    if (gather) hipLaunchKernelGGL(k_cg_update_node<true>, dim3(slice_grid(m)), dim3(64), 0, st, m, v);
    else hipLaunchKernelGGL(k_cg_update_node<false>, dim3(slice_grid(m)), dim3(64), 0, st, m, v);
}

// ---- single-reduction recurrence (multi-rank solves): see kernels.hpp
__global__ __launch_bounds__(192) void k_cgcg_init(DeviceMatrix m, CgVectors v)
{
    __shared__ double rs[kSliceRows];
    __shared__ double sh[3];
    const int G = gridDim.x, t = threadIdx.x;
    double d0 = 0.0, d1 = 0.0;
    for (SliceWalk w(m.n_slices); w.valid(); w.next()) {
        const int sl = w.s;
        const int64_t row = (int64_t)sl * kSliceRows + t;
        const MinvRow mr = load_minv(m, sl, t);
        const double bv = v.b[row];
        __syncthreads();
        rs[t] = bv;
        __syncthreads();
        const double z = apply_minv(mr, t, rs);
        v.x[row] = 0.0;
        v.r[row] = bv;
        v.z[row] = z;
        v.p[row] = 0.0;
        v.sv[row] = 0.0;
        d0 += bv * z;
        d1 += bv * bv;
    }
    const double t0 = block_sum(d0, sh);
    const double t1 = block_sum(d1, sh);
    if (threadIdx.x == 0) {
        v.partials[blockIdx.x] = t0;
        v.partials[G + blockIdx.x] = t1;
    }
}

void launch_cgcg_init(const DeviceMatrix &m, const CgVectors &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_cgcg_init, dim3(slice_grid(m)), dim3(192), 0, st, m, v);
}

// (kGather: the row adds the transposed products of its in-list, as the nodes of k_cg_update_node<true> do.  step >= 0: the scalar step of the previous iteration is done here, by every workgroup
// for itself and published by workgroup 0 -- a launch less between the all-reduce and the next product; the arithmetic
// is that of cg_scalar_phase(CG_PHASE_FUSED_STEP))
template <bool kGather>
__global__ __launch_bounds__(192) void k_cgcg_update(DeviceMatrix m, CgVectors v, int step)
{
    __shared__ double rs[kSliceRows];
    __shared__ double sh[3];
    CgScalars *s = v.s;
    if (s->done != 0) return; // set by an earlier launch: the same in every workgroup
    const int G = gridDim.x, t = threadIdx.x;
    double alpha, beta;
    if (step >= 0) {
        const int par = step & 1;
        const double rz_old = s->ring_rz[par], alpha_old = s->ring_alpha[par];
        const double rzn = s->red[0], rr = s->red[1], zaz = s->red[2];
        int done = 0;
        alpha = 0.0;
        beta = 0.0;
        if (rr <= s->tol2) done = 1;
        else {
            beta = rzn / rz_old;
            const double denom = zaz - beta * rzn / alpha_old;
            if (!(denom > 0.0)) done = -1;
            else alpha = rzn / denom;
        }
        if (blockIdx.x == 0 && t == 0) {
            s->rr = rr;
            const int it = s->iters + 1;
            s->iters = it;
            if (v.hist != nullptr && it <= v.hist_cap) v.hist[it - 1] = rr / s->bb;
            if (done == 0) {
                s->beta = beta;
                s->alpha = alpha;
                s->rz = rzn;
                s->ring_rz[par ^ 1] = rzn;
                s->ring_alpha[par ^ 1] = alpha;
            }
            s->done = done; // read by the later launches only: this one has taken its decision from red[]
        }
        if (done != 0) return;
    } else {
        alpha = s->alpha;
        beta = s->beta;
    }
    double d0 = 0.0, d1 = 0.0;
    for (SliceWalk w(m.n_slices); w.valid(); w.next()) {
        const int sl = w.s;
        const int64_t row = (int64_t)sl * kSliceRows + t;
        const MinvRow mr = load_minv(m, sl, t);
        const double uv = v.z[row], pv = v.p[row], sv = v.sv[row], xv = v.x[row], rv = v.r[row];
        double wv = v.q[row];
        if (kGather) {
            const int Wi = m.in_width[sl], n = t / 6, j = t % 6;
            const int64_t ib = m.in_base[sl];
            for (int k = 0; k < Wi; k++) {
                const int32_t slot = m.gat_slots[ib + (int64_t)k * kSliceNodes + n];
                if (slot >= 0) wv += m.tbuf[(int64_t)slot * 6 + j];
            }
        }
        const double pn = uv + beta * pv, sn = wv + beta * sv;
        v.p[row] = pn;
        v.sv[row] = sn;
        v.x[row] = xv + alpha * pn;
        const double rn = rv - alpha * sn;
        v.r[row] = rn;
        __syncthreads();
        rs[t] = rn;
        __syncthreads();
        const double z = apply_minv(mr, t, rs);
        v.z[row] = z;
        d0 += rn * z;
        d1 += rn * rn;
    }
    const double t0 = block_sum(d0, sh);
    const double t1 = block_sum(d1, sh);
    if (threadIdx.x == 0) {
        v.partials[blockIdx.x] = t0;
        v.partials[G + blockIdx.x] = t1;
    }
}

void launch_cgcg_update(const DeviceMatrix &m, const CgVectors &v, hipStream_t st, int step, bool gather)
{
    if (gather) hipLaunchKernelGGL(k_cgcg_update<true>, dim3(slice_grid(m)), dim3(192), 0, st, m, v, step);
    else hipLaunchKernelGGL(k_cgcg_update<false>, dim3(slice_grid(m)), dim3(192), 0, st, m, v, step);
}

// p = z + beta p over the owned (padded) rows, 16 bytes per lane
__global__ __launch_bounds__(256) void k_cg_direction(CgVectors v, int64_t n2)
{
    if (v.s->done != 0) return;
    const double beta = v.s->beta;
    const double2 *z = reinterpret_cast<const double2 *>(v.z);
    double2 *p = reinterpret_cast<double2 *>(v.p);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        const double2 zv = z[i];
        double2 pv = p[i];
        pv.x = zv.x + beta * pv.x;
        pv.y = zv.y + beta * pv.y;
        p[i] = pv;
    }
}

void launch_cg_direction(const DeviceMatrix &m, const CgVectors &v, hipStream_t st)
{
    const int64_t n2 = (int64_t)m.n_pad * 3;
    const int64_t blocks = (n2 + 255) / 256;
    hipLaunchKernelGGL(k_cg_direction, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, v, n2);
}

// Deterministic two-stage reduction of the per-workgroup partial sums followed by the scalar recurrence
// step, in one launch: kReduceGroups workgroups each sum a contiguous chunk (fixed order), publish their
// result and take a ticket; the workgroup that draws the last ticket adds the stage-1 sums in index order
// and updates alpha / beta / the convergence flag.  Hand-off without fences (an agent-scope release writes
// back the XCD's L2, an acquire invalidates the CU's L1: microseconds each): the stage-1 sums are stored and
// loaded with sc1 (agent-scope relaxed atomics, served by L2), the storing lane waits for its stores (vmcnt(0))
// before its agent-scope ticket add, and the last arriver loads after that add has returned and a workgroup
// barrier (MI355X_MICROARCH.md, hand-offs with sc1 loads in place of the acquire).  Which workgroup is last
// does not change the result: the final sum runs over the stage-1 sums in a fixed tree.
constexpr int kReduceGroups = 64;

constexpr double kRefineDrop = 1.0e-4; // residual reduction asked of a refinement pass (relative to its right-hand side) ...
// ... unless the pass knows better.  Its correction e is the displacement error of the iterate x it started from, and what the
// pass leaves of that error is about ||e|| / ||x|| times the drop of its residual (cg_amg).  With ||x||^2 at hand (pass_xx) the
// pass therefore stops when that estimate, with the ||e_k|| of the correction so far, is kRefineTarget of the tolerance: on the
// 4M panel (||e|| / ||x|| = 4.6e-8 behind a first phase to 1e-8) at a drop of 4.3e-4 instead of 1e-4 -- six iterations of 104 --
// and where the first phase left a larger error, deeper than 1e-4 instead of a second pass.  Never less than two digits, never
// more than six.
constexpr double kRefineTarget = 0.2, kRefineDropMin = 1.0e-6, kRefineDropMax = 1.0e-2;

__device__ __forceinline__ void cg_scalar_phase(const CgVectors &v, int phase, double rtol)
{
    CgScalars *s = v.s;
    if (phase == CG_PHASE_INIT) {
        s->rz = s->red[0];
        s->bb = s->red[1];
        s->rr = s->red[1];
        s->tol2 = rtol > 0.0 ? rtol * rtol * s->red[1] : 0.0;
        s->alpha = 0.0;
        s->beta = 0.0;
        s->iters = 0;
        s->done = (s->red[1] == 0.0) ? 1 : 0;
    } else if (phase == CG_PHASE_RESTART) {
        // explicit residual r = b - K x: red[0] = r.z, red[1] = r.r
        s->rz = s->red[0];
        s->rr = s->red[1];
        s->done = (s->red[1] <= s->tol2) ? 1 : 0;
    } else if (phase == CG_PHASE_ALPHA) {
        const double pq = s->red[0];
        if (!(pq > 0.0)) s->done = -1;
        else s->alpha = s->rz / pq;
    } else if (phase == CG_PHASE_FUSED_INIT) {
        // red = (r.z, r.r = b.b, z.Az) of the initial residual
        s->rz = s->red[0];
        s->bb = s->red[1];
        s->rr = s->red[1];
        s->tol2 = rtol > 0.0 ? rtol * rtol * s->red[1] : 0.0;
        s->beta = 0.0;
        s->alpha = 0.0;
        s->iters = 0;
        s->done = (s->red[1] == 0.0) ? 1 : 0;
        if (s->done == 0) {
            if (!(s->red[2] > 0.0)) s->done = -1;
            else s->alpha = s->red[0] / s->red[2];
        }
        s->ring_rz[0] = s->rz;
        s->ring_alpha[0] = s->alpha;
    } else if (phase == CG_PHASE_FUSED_STEP) {
        // red = (r.z, r.r, z.Az) of the new residual: beta = rz'/rz, alpha = rz' / (z.Az - beta rz'/alpha)
        const double rzn = s->red[0], rr = s->red[1], zaz = s->red[2];
        s->rr = rr;
        const int it = s->iters + 1;
        s->iters = it;
        if (v.hist != nullptr && it <= v.hist_cap) v.hist[it - 1] = rr / s->bb;
        if (rr <= s->tol2) s->done = 1;
        else {
            const double beta = rzn / s->rz;
            const double denom = zaz - beta * rzn / s->alpha;
            if (!(denom > 0.0)) s->done = -1;
            else {
                s->beta = beta;
                s->alpha = rzn / denom;
                s->rz = rzn;
            }
        }
    } else if (phase == CG_PHASE_FLEX_INIT) {
        s->pass_xx = 0.0;
        s->pass_rhs_rr = 0.0;
        s->bb = s->red[0];
        s->rr = s->red[0];
        s->tol2 = rtol > 0.0 ? rtol * rtol * s->red[0] : 0.0;
        s->alpha = 0.0;
        s->beta = 0.0;
        s->rz = 0.0;
        s->iters = 0;
        s->done = (s->red[0] == 0.0) ? 1 : 0;
    } else if (phase == CG_PHASE_FLEX_RESTART) {
        // a refinement pass starts: red[0] = r.r of the new right-hand side; b.b, the tolerance (relative to the
        // original right-hand side), the iteration count and the history carry on
        s->rr = s->red[0];
        s->alpha = 0.0;
        s->beta = 0.0;
        s->rz = 0.0;
        // (cg_amg passes rtol = 0: a pass stops on the drop of its own right-hand side alone; with rtol > 0 it would also
        //  stop at the tolerance of the solve as a whole)
        const double tol2_solve = rtol > 0.0 ? rtol * rtol * s->bb : 0.0;
        s->done = (s->red[0] <= tol2_solve) ? 1 : 0;
        // the correction equation needs four digits, not the full tolerance again: its solution is added to an iterate
        // whose error it reduces by that factor (2e-10 -> 1e-13 and below on the shell systems), and every further
        // digit costs iterations of the whole method
        s->tol2 = fmax(tol2_solve, kRefineDrop * kRefineDrop * s->red[0]);
        s->pass_rhs_rr = s->red[0];
    } else if (phase == CG_PHASE_FLEX_WARM) {
        s->rr = s->red[0];
        s->done = (s->red[0] <= s->tol2) ? 1 : 0;
    } else if (phase == CG_PHASE_FLEX_RZ0) {
        s->rz = s->red[0];
        if (!(s->red[0] > 0.0)) s->done = -1; // the preconditioner is not positive definite
    } else if (phase == CG_PHASE_FLEX_CONV) {
        const double rr = s->red[0];
        s->rr = rr;
        const int it = s->iters + 1;
        s->iters = it;
        if (v.hist != nullptr && it <= v.hist_cap) v.hist[it - 1] = rr / s->bb;
        if (s->pass_xx > 0.0 && s->pass_rhs_rr > 0.0 && s->red[1] > 0.0) {
            // a refinement pass with the adaptive rule: red[1] = e.e of the correction so far
            const double drop = kRefineTarget * s->pass_rtol * sqrt(s->pass_xx / s->red[1]);
            const double d = fmin(fmax(drop, kRefineDropMin), kRefineDropMax);
            s->tol2 = d * d * s->pass_rhs_rr;
        }
        if (rr <= s->tol2) s->done = 1;
    } else if (phase == CG_PHASE_FLEX_BETA) {
        const double rzn = s->red[0], zq = s->red[1];
        if (!(rzn > 0.0)) s->done = -1;
        else {
            s->beta = -s->alpha * zq / s->rz;
            s->rz = rzn;
        }
    } else if (phase == CG_PHASE_BETA) {
        const double rzn = s->red[0], rr = s->red[1];
        s->rr = rr;
        const int it = s->iters + 1;
        s->iters = it;
        if (v.hist != nullptr && it <= v.hist_cap) v.hist[it - 1] = rr / s->bb;
        if (rr <= s->tol2) s->done = 1;
        else {
            s->beta = rzn / s->rz;
            s->rz = rzn;
        }
    }
}

__global__ __launch_bounds__(256) void k_cg_scalar(CgVectors v, int G, int do_reduce, int nsums, int phase,
                                                   double rtol, int len3, int gate_phase)
{
    __shared__ double sh[4];
    CgScalars *s = v.s;
    // gate_phase: the phase this launch belongs to (a reduce-only launch in front of an all-reduce carries
    // phase NONE but must not be skipped when it serves an INIT / RESTART step on a finished solve)
    if (gate_phase != CG_PHASE_INIT && gate_phase != CG_PHASE_RESTART && gate_phase != CG_PHASE_FUSED_INIT &&
        gate_phase != CG_PHASE_FLEX_INIT && gate_phase != CG_PHASE_FLEX_RESTART && gate_phase != CG_PHASE_FLEX_WARM && s->done != 0)
        return; // same decision in every workgroup
    if (!do_reduce) {
        if (blockIdx.x == 0 && threadIdx.x == 0) cg_scalar_phase(v, phase, rtol);
        return;
    }
    const int nwg = gridDim.x;
    for (int a = 0; a < nsums; a++) {
        const int len = (a == 2) ? len3 : G; // the third array (single-reduction CG: the SpMV's) has its own length
        const int chunk = (len + nwg - 1) / nwg;
        const int lo = blockIdx.x * chunk, hi = min(len, lo + chunk);
        const double *pa = v.partials + (int64_t)a * G;
        double acc = 0.0;
        const int B = blockDim.x;
        for (int i0 = lo + threadIdx.x; i0 < hi; i0 += 4 * B) {
            double t[4];
#pragma unroll
            for (int q = 0; q < 4; q++) t[q] = (i0 + q * B < hi) ? pa[i0 + q * B] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) acc += t[q];
        }
        const double tot = block_sum(acc, sh);
        if (threadIdx.x == 0) __hip_atomic_store(&s->stage[a][blockIdx.x], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __shared__ int last_flag;
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t ticket = __hip_atomic_fetch_add(&s->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = (ticket == (uint32_t)nwg - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!last_flag) return;
    for (int a = 0; a < nsums; a++) {
        double part = 0.0;
        if ((int)threadIdx.x < nwg) part = __hip_atomic_load(&s->stage[a][threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double tot = block_sum(part, sh);
        if (threadIdx.x == 0) s->red[a] = tot;
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&s->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // ready for the next launch
        cg_scalar_phase(v, phase, rtol);
    }
}

void launch_cg_scalar(const DeviceMatrix &m, const CgVectors &v, bool reduce, int nsums, CgPhase phase,
                      double rtol, hipStream_t st, int n_partials, int len3, int gate_phase)
{
    const int G = n_partials > 0 ? n_partials : slice_grid(m);
    const int groups = reduce ? (G >= 4096 ? kReduceGroups : 1) : 1;
    hipLaunchKernelGGL(k_cg_scalar, dim3(groups), dim3(256), 0, st, v, G, reduce ? 1 : 0, nsums, (int)phase, rtol, len3,
                       gate_phase < 0 ? (int)phase : gate_phase);
}

__global__ void k_pack(const double *p, const int32_t *nodes, int32_t count, int32_t width, double *buf)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)count * width) return;
    buf[i] = p[(int64_t)nodes[i / width] * width + i % width];
}

void launch_pack(const double *p, const int32_t *send_nodes, int32_t count, double *sendbuf, hipStream_t st, int width)
{
    const int64_t n = (int64_t)count * width;
    if (n == 0) return;
    hipLaunchKernelGGL(k_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, send_nodes, count, (int32_t)width, sendbuf);
}

} // namespace femshell
