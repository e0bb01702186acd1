// cases.hip -- gfx950 kernels of the load cases (femshell_solve_cases, cases.hpp): the vector steps of a block-Jacobi CG that
// runs up to four right-hand sides in lockstep, and its scalar step.  One lane per node (device_common.hpp), 48 bytes per node and
// vector as three 16-byte words, no LDS in the vector kernels, no atomics; a node's inverse diagonal block is read once for all
// columns of the pass.  The scalars of a column (CaseScalars) are read through the kernel argument with a constant index: the
// same address in every lane, a scalar load.  A column whose done flag is set is skipped whole -- no load, no store, no partial
// sum -- so what it holds does not depend on how long its neighbours run.
#include "cases.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

int cases_grid(const DeviceMatrix &m) { return node_grid(m); }

// writes the sums of the lanes' d0[j], d1[j] (kSums == 2) or d0[j] alone: partials[(2 j + q) * G + workgroup]
template <int kB, int kSums>
__device__ __forceinline__ void cases_store_sums(const bool live[kB], const double d0[kB], const double d1[kB], double *__restrict__ partials)
{
    const int G = gridDim.x;
#pragma unroll
    for (int j = 0; j < kB; j++) {
        if (!live[j]) continue;
        const double t0 = wave_sum(d0[j]);
        const double t1 = kSums == 2 ? wave_sum(d1[j]) : 0.0;
        if (threadIdx.x == 0) {
            partials[(int64_t)(2 * j) * G + blockIdx.x] = t0;
            if (kSums == 2) partials[(int64_t)(2 * j + 1) * G + blockIdx.x] = t1;
        }
    }
}

// x = 0, z = D^-1 r, p = z; sums (r.z, r.r).  R holds the masked loads (zero on padding rows and fixed dofs).
template <int kB>
__global__ __launch_bounds__(64) void k_cases_init(DeviceMatrix m, double *__restrict__ X, const double *__restrict__ R, double *__restrict__ Z,
                                                   double *__restrict__ P, int64_t ld, double *__restrict__ partials)
{
    const int half = threadIdx.x >> 5, n = threadIdx.x & 31;
    bool live[kB];
    double d0[kB], d1[kB];
#pragma unroll
    for (int j = 0; j < kB; j++) {
        live[j] = true;
        d0[j] = 0.0;
        d1[j] = 0.0;
    }
    for (SliceWalk w(node_pairs(m.n_slices)); w.valid(); w.next()) {
        const int sl = 2 * w.s + half;
        if (sl >= m.n_slices) continue;
        const int64_t node = (int64_t)sl * kSliceNodes + n;
        double mv[kMinvWords];
        node_minv(m, sl, n, false, mv);
#pragma unroll
        for (int j = 0; j < kB; j++) {
            double rv[6], z[6];
            const double zero[6] = {0, 0, 0, 0, 0, 0};
            load_node6(R + j * ld, node, false, rv);
            node_minv_apply(mv, rv, z);
            store_node6(X + j * ld, node, false, zero);
            store_node6(Z + j * ld, node, false, z);
            store_node6(P + j * ld, node, false, z);
#pragma unroll
            for (int i = 0; i < 6; i++) {
                d0[j] += rv[i] * z[i];
                d1[j] += rv[i] * rv[i];
            }
        }
    }
    cases_store_sums<kB, 2>(live, d0, d1, partials);
}

// sum p.q
template <int kB>
__global__ __launch_bounds__(64) void k_cases_dot(DeviceMatrix m, const CaseScalars *__restrict__ s, const double *__restrict__ P,
                                                  const double *__restrict__ Q, int64_t ld, double *__restrict__ partials)
{
    const int half = threadIdx.x >> 5, n = threadIdx.x & 31;
    bool live[kB];
    double d0[kB];
#pragma unroll
    for (int j = 0; j < kB; j++) {
        live[j] = s[j].done == 0;
        d0[j] = 0.0;
    }
    for (SliceWalk w(node_pairs(m.n_slices)); w.valid(); w.next()) {
        const int sl = 2 * w.s + half;
        if (sl >= m.n_slices) continue;
        const int64_t node = (int64_t)sl * kSliceNodes + n;
#pragma unroll
        for (int j = 0; j < kB; j++) {
            if (!live[j]) continue;
            double pv[6], qv[6];
            load_node6(P + j * ld, node, false, pv);
            load_node6(Q + j * ld, node, false, qv);
#pragma unroll
            for (int i = 0; i < 6; i++) d0[j] += pv[i] * qv[i];
        }
    }
    cases_store_sums<kB, 1>(live, d0, d0, partials);
}

// x += alpha_j p ; r -= alpha_j q ; z = D^-1 r ; sums (r.z, r.r) -- per column the arithmetic of k_cg_update_node<false>
template <int kB>
__global__ __launch_bounds__(64) void k_cases_update(DeviceMatrix m, const CaseScalars *__restrict__ s, const double *__restrict__ P,
                                                     const double *__restrict__ Q, double *__restrict__ X, double *__restrict__ R,
                                                     double *__restrict__ Z, int64_t ld, double *__restrict__ partials)
{
    const int half = threadIdx.x >> 5, n = threadIdx.x & 31;
    bool live[kB];
    double alpha[kB], d0[kB], d1[kB];
    bool any = false;
#pragma unroll
    for (int j = 0; j < kB; j++) {
        live[j] = s[j].done == 0;
        alpha[j] = s[j].alpha;
        any = any || live[j];
        d0[j] = 0.0;
        d1[j] = 0.0;
    }
    if (!any) return;
    for (SliceWalk w(node_pairs(m.n_slices)); w.valid(); w.next()) {
        const int sl = 2 * w.s + half;
        if (sl >= m.n_slices) continue;
        const int64_t node = (int64_t)sl * kSliceNodes + n;
        double mv[kMinvWords];
        node_minv(m, sl, n, false, mv);
#pragma unroll
        for (int j = 0; j < kB; j++) {
            if (!live[j]) continue;
            double pv[6], qv[6], xv[6], rv[6], z[6];
            load_node6(P + j * ld, node, false, pv);
            load_node6(X + j * ld, node, false, xv);
            load_node6(R + j * ld, node, false, rv);
            load_node6(Q + j * ld, node, false, qv);
#pragma unroll
            for (int i = 0; i < 6; i++) {
                xv[i] = xv[i] + alpha[j] * pv[i];
                rv[i] = rv[i] - alpha[j] * qv[i];
            }
            store_node6(X + j * ld, node, false, xv);
            store_node6(R + j * ld, node, false, rv);
            node_minv_apply(mv, rv, z);
            store_node6(Z + j * ld, node, false, z);
#pragma unroll
            for (int i = 0; i < 6; i++) {
                d0[j] += rv[i] * z[i];
                d1[j] += rv[i] * rv[i];
            }
        }
    }
    cases_store_sums<kB, 2>(live, d0, d1, partials);
}

// p = z + beta_j p over the owned (padded) rows, 16 bytes per lane (k_cg_direction for every running column)
template <int kB>
__global__ __launch_bounds__(256) void k_cases_direction(const CaseScalars *__restrict__ s, const double *__restrict__ Z, double *__restrict__ P,
                                                         int64_t ld, int64_t n2)
{
#pragma unroll
    for (int j = 0; j < kB; j++) {
        if (s[j].done != 0) continue;
        const double beta = s[j].beta;
        const double2 *z = reinterpret_cast<const double2 *>(Z + j * ld);
        double2 *p = reinterpret_cast<double2 *>(P + j * ld);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
            const double2 zv = z[i];
            double2 pv = p[i];
            pv.x = zv.x + beta * pv.x;
            pv.y = zv.y + beta * pv.y;
            p[i] = pv;
        }
    }
}

// The scalar step of column j = blockIdx.x.  Wave q adds the partial sums of quantity q: lane l its stretch [l ch, (l + 1) ch),
// ch = ceil(G / 64), in index order, then lane 0 the 64 stretch sums in index order.  Thread 0 takes the step: the arithmetic of
// cg_scalar_phase (cg_kernels.hip) for CG_PHASE_INIT / _ALPHA / _BETA, on the column's own scalars.
__global__ __launch_bounds__(128) void k_cases_scalar(CaseScalars *__restrict__ s_all, const double *__restrict__ partials, int G, int phase,
                                                      double rtol)
{
    __shared__ double stretch[2][64];
    __shared__ double red[2];
    const int j = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    CaseScalars *s = s_all + j;
    if (phase != CASES_PHASE_INIT && s->done != 0) return; // (the same decision in both waves)
    const int nsums = phase == CASES_PHASE_ALPHA ? 1 : 2;
    if (q < nsums) {
        const double *pa = partials + (int64_t)(2 * j + q) * G;
        const int ch = (G + 63) >> 6, lo = lane * ch, hi = min(G, lo + ch);
        double acc = 0.0;
        for (int i = lo; i < hi; i++) acc += pa[i];
        stretch[q][lane] = acc;
    }
    __syncthreads();
    if (q < nsums && lane == 0) {
        double tot = 0.0;
        for (int l = 0; l < 64; l++) tot += stretch[q][l];
        red[q] = tot;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (phase == CASES_PHASE_INIT) {
        s->rz = red[0];
        s->bb = red[1];
        s->rr = red[1];
        s->tol2 = rtol > 0.0 ? rtol * rtol * red[1] : 0.0;
        s->alpha = 0.0;
        s->beta = 0.0;
        s->pq = 0.0;
        s->iters = 0;
        s->done = (red[1] == 0.0) ? 1 : 0;
    } else if (phase == CASES_PHASE_ALPHA) {
        const double pq = red[0];
        s->pq = pq;
        if (!(pq > 0.0)) s->done = -1;
        else s->alpha = s->rz / pq;
    } else if (phase == CASES_PHASE_BETA) {
        const double rzn = red[0], rr = red[1];
        s->rr = rr;
        s->iters = s->iters + 1;
        if (rr <= s->tol2) s->done = 1;
        else {
            s->beta = rzn / s->rz;
            s->rz = rzn;
        }
    }
}

#define CASES_BY_WIDTH(nb, CALL)    \
    switch (nb) {                   \
    case 4: { constexpr int kB = 4; CALL; } break; \
    case 3: { constexpr int kB = 3; CALL; } break; \
    case 2: { constexpr int kB = 2; CALL; } break; \
    default: { constexpr int kB = 1; CALL; } break; \
    }

void launch_cases_init(const DeviceMatrix &m, int nb, double *X, const double *R, double *Z, double *P, int64_t ld, double *partials,
                       hipStream_t st)
{
    if (nb < 1 || nb > kSpmmMaxCols || m.n_slices == 0) return;
    CASES_BY_WIDTH(nb, hipLaunchKernelGGL((k_cases_init<kB>), dim3(cases_grid(m)), dim3(64), 0, st, m, X, R, Z, P, ld, partials));
}

void launch_cases_dot(const DeviceMatrix &m, int nb, const CaseScalars *s, const double *P, const double *Q, int64_t ld, double *partials,
                      hipStream_t st)
{
    if (nb < 1 || nb > kSpmmMaxCols || m.n_slices == 0) return;
    CASES_BY_WIDTH(nb, hipLaunchKernelGGL((k_cases_dot<kB>), dim3(cases_grid(m)), dim3(64), 0, st, m, s, P, Q, ld, partials));
}

void launch_cases_update(const DeviceMatrix &m, int nb, const CaseScalars *s, const double *P, const double *Q, double *X, double *R, double *Z,
                         int64_t ld, double *partials, hipStream_t st)
{
    if (nb < 1 || nb > kSpmmMaxCols || m.n_slices == 0) return;
    CASES_BY_WIDTH(nb, hipLaunchKernelGGL((k_cases_update<kB>), dim3(cases_grid(m)), dim3(64), 0, st, m, s, P, Q, X, R, Z, ld, partials));
}

void launch_cases_direction(const DeviceMatrix &m, int nb, const CaseScalars *s, const double *Z, double *P, int64_t ld, hipStream_t st)
{
    if (nb < 1 || nb > kSpmmMaxCols || m.n_pad == 0) return;
    const int64_t n2 = (int64_t)m.n_pad * 3;
    const int64_t blocks = (n2 + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    CASES_BY_WIDTH(nb, hipLaunchKernelGGL((k_cases_direction<kB>), dim3(grid), dim3(256), 0, st, s, Z, P, ld, n2));
}

void launch_cases_scalar(int nb, CaseScalars *s, const double *partials, int G, CasesPhase phase, double rtol, hipStream_t st)
{
    if (nb < 1 || nb > kSpmmMaxCols || G < 1) return;
    hipLaunchKernelGGL(k_cases_scalar, dim3((unsigned)nb), dim3(128), 0, st, s, partials, G, (int)phase, rtol);
}

} // namespace femshell
