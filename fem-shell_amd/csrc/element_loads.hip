// element_loads.hip -- nodal equivalents of per-element pressure and traction (femshell_set_element_loads; gfx950, wave64).
//
// Per element four doubles (p, qx, qy, qz): p along the element's own +ez (the normal K is built with), q per area in global
// axes.  Lumped with the shares of the lumped mass: every node of a TRI3 gets p (b-a)x(c-a)/6 + q A/3, every node of a QUAD4
// p (d1 x d2)/8 + q A/4 (diagonals d1 = c-a, d2 = d-b), A = |cross|/2; the rotational rows get nothing (include/femshell.h).
//
// One workgroup per slice (32 node rows), over the slice's element list in tiles of kElTile entries:
//   A  one lane per list entry gathers the element's node ids, coordinates and load words (two 16-byte loads, through the
//      entry's local element index) and leaves the share vector -- the same three doubles for every node of the element -- in
//      LDS.  What it leaves of the node ids is which rows of the slice contain the entry, turned round by one ballot per row:
//      per wave of 64 consecutive entries and per row a 64-bit word, bit b = the wave's entry b contains the row;
//   B  one lane per (row, translation), 96 lanes, walks the tile IN LIST ORDER -- the words of its row wave after wave, the set
//      bits of a word from the lowest -- and adds the share of every element that contains its row: about six additions on a
//      structured slice, where a walk over all entries would compare 130 times.  The row sum stays in the lane's register from
//      tile to tile (the pattern of k_element_product): the order of the additions is the list order whatever the tile is,
//      there are no atomics, and two launches give the same bits.
// Then one lane per row writes base + S on the translations and base on the rotations (base == nullptr: zero); padding rows
// write zero.  A degenerate element contributes the zero its cross product gives and reports nothing.
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "k_element_loads assumes 32-node slices");

constexpr int kElThreads = 128;
constexpr int kElTile = 256; // entries per tile: 24 bytes of LDS each (share vector), 6 KB + the rows' words + the row sums per workgroup
static_assert(kElTile % kElThreads == 0 && kElThreads % 64 == 0, "phase A of k_element_loads: whole waves, whole rounds of the workgroup");

template <bool kHasQuads>
__global__ __launch_bounds__(kElThreads) void k_element_loads(DeviceMatrix m, const int32_t *__restrict__ slice_elem_local,
                                                              const double2 *__restrict__ elem_load, const double *__restrict__ base,
                                                              double *__restrict__ out)
{
    __shared__ double s_share[kElTile * 3];
    __shared__ unsigned long long s_rows[kElTile / 64][kSliceNodes]; // per wave of entries and row: the entries that contain the row
    __shared__ double s_sum[kSliceNodes * 3];
    const int tid = threadIdx.x, lane = tid & 63;
    SliceWalk w(m.n_slices);
    for (; w.valid(); w.next()) {
        const int s = w.s;
        const int e0 = m.slice_elem_ptr[s], ne = m.slice_elem_ptr[s + 1] - e0;
        const int row0 = s * kSliceNodes;
        const int my_row = tid / 3, my_v = tid % 3; // phase B: lanes 0 .. 95
        double sum = 0.0;
        for (int t0 = 0; t0 < ne; t0 += kElTile) {
            const int nt = min(kElTile, ne - t0);
            // ---- A: share vectors, and which rows of the slice every entry contains.  (Whole waves walk the tile, so that every
            //      lane takes part in the ballots below; a wave whose 64 entries lie past the tile's end skips them.)
            for (int i0 = tid - lane; i0 < nt; i0 += kElThreads) {
                const int i = i0 + lane;
                uint32_t rows = 0; // bit r: node row0 + r belongs to the entry
                if (i < nt) {
                    const int4 c = m.slice_elem_nodes[e0 + t0 + i];
                    const int le = slice_elem_local[e0 + t0 + i];
                    const double2 l0 = elem_load[2 * (int64_t)le], l1 = elem_load[2 * (int64_t)le + 1]; // (p, qx), (qy, qz)
                    const double *pa = m.xyz + 3 * (int64_t)c.x, *pb = m.xyz + 3 * (int64_t)c.y, *pc = m.xyz + 3 * (int64_t)c.z;
                    double d1[3], d2[3], part, pdiv;
                    if (!kHasQuads || c.w < 0) { // TRI3: (b - a) x (c - a), a third of the area to each node
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            d1[d] = pb[d] - pa[d];
                            d2[d] = pc[d] - pa[d];
                        }
                        part = 3.0;
                        pdiv = 6.0;
                    } else { // QUAD4: the diagonals d1 = c - a, d2 = d - b, a quarter to each node
                        const double *pd = m.xyz + 3 * (int64_t)c.w;
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            d1[d] = pc[d] - pa[d];
                            d2[d] = pd[d] - pb[d];
                        }
                        part = 4.0;
                        pdiv = 8.0;
                    }
                    const double cx = d1[1] * d2[2] - d1[2] * d2[1], cy = d1[2] * d2[0] - d1[0] * d2[2], cz = d1[0] * d2[1] - d1[1] * d2[0];
                    const double share = 0.5 * sqrt(cx * cx + cy * cy + cz * cz) / part; // (as k_lumped_mass forms it)
                    s_share[3 * i + 0] = l0.x * cx / pdiv + l0.y * share;
                    s_share[3 * i + 1] = l0.x * cy / pdiv + l1.x * share;
                    s_share[3 * i + 2] = l0.x * cz / pdiv + l1.y * share;
                    const int nid[4] = {c.x, c.y, c.z, kHasQuads ? c.w : -1};
#pragma unroll
                    for (int j = 0; j < 4; j++) entry_row_bit(nid[j], row0, rows); // (every node of the element gets the same share)
                }
                publish_rows(rows, lane, s_rows[i0 >> 6]);
            }
            __syncthreads();
            // ---- B: row sums in list order: waves of entries ascending, within one the set bits ascending
            if (tid < kSliceNodes * 3) for_entries_of_row(s_rows, nt, my_row, [&](int i) { sum += s_share[3 * i + my_v]; });
            __syncthreads(); // (the next tile overwrites the shares)
        }
        if (tid < kSliceNodes * 3) s_sum[tid] = sum;
        __syncthreads();
        if (tid < kSliceNodes) {
            const int a = row0 + tid;
            double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (a < m.n_own) {
                if (base != nullptr) load_node6(base, a, false, v);
#pragma unroll
                for (int d = 0; d < 3; d++) v[d] = base != nullptr ? v[d] + s_sum[3 * tid + d] : s_sum[3 * tid + d];
            }
            store_node6(out, a, false, v);
        }
        __syncthreads(); // (the next slice overwrites the row sums)
    }
}

void launch_element_loads(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *elem_load, const double *base, double *out,
                          hipStream_t st)
{
    if (m.n_slices == 0) return;
    const int g = slice_grid(m);
    const double2 *el = reinterpret_cast<const double2 *>(elem_load);
    if (m.n_lquad > 0) hipLaunchKernelGGL(k_element_loads<true>, dim3(g), dim3(kElThreads), 0, st, m, slice_elem_local, el, base, out);
    else hipLaunchKernelGGL(k_element_loads<false>, dim3(g), dim3(kElThreads), 0, st, m, slice_elem_local, el, base, out);
}

} // namespace femshell
