// device_common.hpp -- device helpers shared by the kernel translation units (kernels.hip, spmv_kernels.hip, cg_kernels.hip,
// amg_kernels.hip, ...):
// the XCD-aware slice walk, the pieces of a slice's row sums in list order, workgroup sums, the packed block-Jacobi inverse.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "plan.hpp"

namespace femshell {

// first failure wins: the status word (HBM, or host memory mapped into the device: context.hpp status_word) gets `value` if it
// still holds zero -- a system-scope compare-and-swap, executed on failures only
__device__ __forceinline__ void report_status(int32_t *status, int32_t value)
{
    int32_t expected = 0;
    (void)__hip_atomic_compare_exchange_strong(status, &expected, value, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}


// Workgroup b belongs to XCD group x = b%8 and walks the slices x*per + j, j = b/8, b/8 + G/8, ...
// of that group's contiguous eighth of the rows (per = ceil(S/8), G = gridDim.x).
struct SliceWalk {
    int per, first, last, step, s;
    __device__ __forceinline__ SliceWalk(int n_slices)
    {
        per = (n_slices + 7) >> 3;
        const int x = blockIdx.x & 7;
        first = x * per;
        last = min(first + per, n_slices);
        step = gridDim.x >> 3;
        s = first + (blockIdx.x >> 3);
    }
    __device__ __forceinline__ bool valid() const { return s < last; }
    __device__ __forceinline__ void next() { s += step; }
};

// ---- row sums of a slice over its element list, in list order (k_element_loads, k_element_thermal, k_geometric_product) ----------
// A kernel walks the list in tiles.  Whole waves take 64 consecutive entries each; a lane leaves what its entry contributes in LDS,
// and one ballot per row turns the entries' membership round: per wave of entries and row a 64-bit word, bit b = the wave's entry
// b contains the row.  A lane that sums a row then visits the words of its row wave after wave and the set bits of a word from
// the lowest -- the list order whatever the tile and the grid are, no atomics, the same bits from every launch.
//
// Node j of an entry: if it is a row of the slice (a triangle's fourth node, -1, and ghosts fall outside), its bit joins `rows`
// (bit r: node row0 + r belongs to the entry) and its row becomes byte j of `word`.  `word` starts as 0xFFFFFFFF: 0xFF means none.
// (One node per call, the loop over the nodes stays in the kernel: with the loop in here the compiler allots the instantiations
// of k_geometric_product two to seven more vector registers for the same work.)
__device__ __forceinline__ void entry_node(int j, int node, int row0, uint32_t &rows, uint32_t &word)
{
    const uint32_t r = (uint32_t)(node - row0);
    if (r < (uint32_t)kSliceNodes) {
        rows |= 1u << r;
        word = (word & ~(0xFFu << (8 * j))) | (r << (8 * j));
    }
}
// the row bit alone, for a kernel that does not ask where in the entry a row is (k_element_loads: with the unused word in
// the source its triangle instantiation is allotted another register count)
__device__ __forceinline__ void entry_row_bit(int node, int row0, uint32_t &rows)
{
    const uint32_t r = (uint32_t)(node - row0);
    if (r < (uint32_t)kSliceNodes) rows |= 1u << r;
}
// which node of the entry the row is (a node occurs once in an element)
__device__ __forceinline__ int entry_node_of_row(uint32_t word, uint32_t row)
{
    return (word & 0xFFu) == row ? 0 : (((word >> 8) & 0xFFu) == row ? 1 : (((word >> 16) & 0xFFu) == row ? 2 : 3));
}
// The wave's ballots into its words, wave_rows[kSliceNodes].  Every lane of the wave must call it (rows = 0 past the tile's end):
// the wave's 64 entries are 64 consecutive entries of the list, so bit b of the ballot for row r is the wave's entry b.
__device__ __forceinline__ void publish_rows(uint32_t rows, int lane, unsigned long long *wave_rows)
{
    for (int r = 0; r < kSliceNodes; r++) {
        const unsigned long long has = __ballot((rows >> r) & 1u);
        if (lane == r) wave_rows[r] = has;
    }
}
// body(i) for the entries i < nt of the tile that contain `row`, in list order
template <class Body>
__device__ __forceinline__ void for_entries_of_row(const unsigned long long (*s_rows)[kSliceNodes], int nt, int row, Body body)
{
    for (int c0 = 0; c0 < nt; c0 += 64) {
        unsigned long long has = s_rows[c0 >> 6][row];
        while (has) {
            body(c0 + __ffsll(has) - 1);
            has &= has - 1;
        }
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sum over the workgroup, valid in thread 0; sh must hold blockDim.x/64 doubles
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < nw; i++) t += sh[i];
    __syncthreads();
    return t;
}

// minv layout: per slice 21 words (upper triangle of the symmetric 6x6 inverse, row-major) x 32 nodes, nodes fastest
constexpr int kMinvWords = 21;
__host__ __device__ __forceinline__ int minv_word(int i, int j) { return (i * (11 - i)) / 2 + j; } // i <= j

// z_row = sum_j Minv[row][j] * r[node*6+j].  The six Minv entries of the row are fetched before the
// residual of the slice is exchanged through LDS, so their latency overlaps the barrier.
struct MinvRow {
    double a[6];
};
__device__ __forceinline__ MinvRow load_minv(const DeviceMatrix &m, int sl, int t)
{
    const int n = t / 6, i = t % 6;
    const double *mi = m.minv + (int64_t)sl * kMinvWords * kSliceNodes + n;
    MinvRow r;
#pragma unroll
    for (int j = 0; j < 6; j++) r.a[j] = mi[minv_word(i < j ? i : j, i < j ? j : i) * kSliceNodes];
    return r;
}
__device__ __forceinline__ double apply_minv(const MinvRow &mr, int t, const double *rs)
{
    const int nb = (t / 6) * 6;
    double z = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) z += mr.a[j] * rs[nb + j];
    return z;
}

// ---- one lane per NODE (round 5) ---------------------------------------------------------------------------------------
// The vector kernels that apply the 6x6 block-Jacobi inverse used one lane per scalar row and exchanged the residual of a node
// through LDS; their 4-byte loads of the inverse (21 words, nodes fastest) scatter over six words per wave instruction and two
// barriers per slice keep few loads in flight: 3.8-4.4 TB/s where the plain vector passes reach 6 (round 5, PMC).  With a lane
// per node -- the mapping of k_spmv_sym -- a half-wave reads one word of the inverse for its 32 nodes as one 128/256-byte
// segment, the six entries of a vector as three 16-byte words, and the apply is lane-local: no LDS, no barrier.
__device__ __forceinline__ void load_node6(const double *x, int64_t node, bool as_float, double out[6])
{
    if (as_float) {
        const float2 *xf = reinterpret_cast<const float2 *>(x) + 3 * node;
        const float2 a0 = xf[0], a1 = xf[1], a2 = xf[2];
        out[0] = a0.x; out[1] = a0.y; out[2] = a1.x; out[3] = a1.y; out[4] = a2.x; out[5] = a2.y;
    } else {
        const double2 *xd = reinterpret_cast<const double2 *>(x) + 3 * node;
        const double2 a0 = xd[0], a1 = xd[1], a2 = xd[2];
        out[0] = a0.x; out[1] = a0.y; out[2] = a1.x; out[3] = a1.y; out[4] = a2.x; out[5] = a2.y;
    }
}
__device__ __forceinline__ void store_node6(double *x, int64_t node, bool as_float, const double v[6])
{
    if (as_float) {
        float2 *xf = reinterpret_cast<float2 *>(x) + 3 * node;
        xf[0] = make_float2((float)v[0], (float)v[1]);
        xf[1] = make_float2((float)v[2], (float)v[3]);
        xf[2] = make_float2((float)v[4], (float)v[5]);
    } else {
        double2 *xd = reinterpret_cast<double2 *>(x) + 3 * node;
        xd[0] = make_double2(v[0], v[1]);
        xd[1] = make_double2(v[2], v[3]);
        xd[2] = make_double2(v[4], v[5]);
    }
}
// the 21 words of node n's inverse diagonal block (smoother: from the single-precision copy when the level has one)
__device__ __forceinline__ void node_minv(const DeviceMatrix &m, int sl, int n, bool smoother, double mv[kMinvWords])
{
    if (smoother && m.minv32 != nullptr) {
        const float *mi = m.minv32 + (int64_t)sl * kMinvWords * kSliceNodes + n;
#pragma unroll
        for (int w = 0; w < kMinvWords; w++) mv[w] = (double)mi[w * kSliceNodes];
    } else {
        const double *mi = m.minv + (int64_t)sl * kMinvWords * kSliceNodes + n;
#pragma unroll
        for (int w = 0; w < kMinvWords; w++) mv[w] = mi[w * kSliceNodes];
    }
}
// z = D^-1 r for one node; per row the order of apply_minv (j ascending from zero)
__device__ __forceinline__ void node_minv_apply(const double mv[kMinvWords], const double r[6], double z[6])
{
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) s += mv[minv_word(i < j ? i : j, i < j ? j : i)] * r[j];
        z[i] = s;
    }
}
// symmetric storage, second phase of a product for the six rows of node n of slice sl: acc += the transposed products of the
// node's in-list in the plan's fixed order (per row the additions of k_cgcg_update<true>, entry after entry); two entries' loads
// in flight together.  kT32: the products were stored as floats (DeviceMatrix::vec32)
template <bool kT32> __device__ __forceinline__ void node_gather(const DeviceMatrix &m, int sl, int n, double acc[6])
{
    const int Wi = m.in_width[sl];
    const int64_t ib = m.in_base[sl];
    for (int k0 = 0; k0 < Wi; k0 += 2) {
        const int32_t s0 = m.gat_slots[ib + (int64_t)k0 * kSliceNodes + n];
        const int32_t s1 = k0 + 1 < Wi ? m.gat_slots[ib + (int64_t)(k0 + 1) * kSliceNodes + n] : -1;
        double t0[6], t1[6];
        if (s0 >= 0) load_node6(m.tbuf, s0, kT32, t0);
        if (s1 >= 0) load_node6(m.tbuf, s1, kT32, t1);
        if (s0 >= 0) {
#pragma unroll
            for (int j = 0; j < 6; j++) acc[j] += t0[j];
        }
        if (s1 >= 0) {
#pragma unroll
            for (int j = 0; j < 6; j++) acc[j] += t1[j];
        }
    }
}
// (MEASURED, round 5, and dropped: the vectors of k_cheb_step_node moved by the whole wave -- fully coalesced 16-byte accesses of the
//  3 KB two adjacent slices occupy, turned into the node-per-lane view through LDS -- instead of three 16-byte words per lane at a
//  stride of 48 bytes: 0.6393 -> 0.6350 s and 0.6319 -> 0.6308 s per solve of the 4M-triangle panel, alternating on one box.  The
//  partial-line stores the counters show -- 312 MB written where 240 MB are due -- are not what bounds these kernels.)
// the slices a 64-lane workgroup of a node kernel walks: pairs of slices, one per half-wave (the walk of k_spmv_sym)
__host__ __device__ __forceinline__ int node_pairs(int n_slices) { return (n_slices + 1) >> 1; }
// workgroups of a node kernel: 64 lanes = two slices; never more than the per-slice kernels of the same matrix launch
inline int node_grid(const DeviceMatrix &m)
{
    const int g = 8 * ((node_pairs(m.n_slices) + 7) / 8), cap = slice_grid(m);
    return g < cap ? g : cap;
}

} // namespace femshell
