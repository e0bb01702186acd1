// elastic_support.hip -- elastic supports: element foundations and nodal springs (femshell_set_foundation, femshell_set_springs;
// gfx950, wave64).
//
// Per element two doubles (kn, kt), force per volume: kn along the element's own +ez (the normal of the element loads: TRI3
// c = (b-a) x (c-a), QUAD4 c = d1 x d2), kt in the element's plane.  Lumped with the shares of the lumped mass: every node of
// element e gets the symmetric 3 x 3 block  B_e = share_e [kt I + (kn - kt) n n^T],  share_e = A_e / 3 (TRI3), A_e / 4 (QUAD4),
// A_e = |c| / 2, n = c / |c|; the rotational rows get nothing.  Per node six doubles of springs in global axes.  The support table
// holds per node nine words: the tensor T_a = sum of the B_e in the project's order xx yy zz xy yz zx with the translational
// springs added to the first three, then the three rotational springs (include/femshell.h).
//
// k_support_rows: one workgroup per slice (32 node rows), over the slice's element list in tiles of kSupTile entries -- the walk of
// k_element_loads with a tensor where that kernel sums a vector:
//   A  one lane per list entry gathers the element's node ids, coordinates and (kn, kt) (one 16-byte load, through the entry's
//      local element index) and leaves the six words of B_e -- the same for every node of the element -- in LDS, and the ballots
//      that say which rows of the slice contain the entry (device_common.hpp);
//   B  one lane per (row, word), 192 lanes, walks the tile IN LIST ORDER and adds the word of every element that contains its
//      row.  The sum stays in the lane's register from tile to tile: the order of the additions is the list order whatever the
//      tile and the grid are, there are no atomics, and two launches give the same bits.
// Then one lane per row adds the springs (one addition per diagonal word, after the row sum) and writes the nine words; padding
// rows write zeros.  A degenerate element contributes zero and reports nothing.
// k_support_add: one lane per owned node adds the table into the diagonal block of K behind the assembly.
// k_support_apply: one lane per node, y = base + s K_sup (x + xp).
// k_support_words: the table as two node vectors of six, for the transfers of node_io.
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "k_support_rows assumes 32-node slices");

constexpr int kSupThreads = 256;
constexpr int kSupTile = 256; // entries per tile: 48 bytes of LDS each (the six words of B_e), 12 KB + the rows' words + the row sums
constexpr int kSupWords = 6;
static_assert(kSupTile % kSupThreads == 0 && kSupThreads % 64 == 0, "phase A of k_support_rows: whole waves, whole rounds of the workgroup");
static_assert(kSliceNodes * kSupWords <= kSupThreads, "phase B of k_support_rows: a lane per (row, word)");

template <bool kHasQuads>
__global__ __launch_bounds__(kSupThreads) void k_support_rows(DeviceMatrix m, const int32_t *__restrict__ slice_elem_local,
                                                              const double2 *__restrict__ elem_found, const double *__restrict__ spring,
                                                              double *__restrict__ table)
{
    __shared__ double s_b[kSupTile * kSupWords];
    __shared__ unsigned long long s_rows[kSupTile / 64][kSliceNodes]; // per wave of entries and row: the entries that contain the row
    __shared__ double s_sum[kSliceNodes * kSupWords];
    const int tid = threadIdx.x, lane = tid & 63;
    SliceWalk w(m.n_slices);
    for (; w.valid(); w.next()) {
        const int s = w.s;
        const int e0 = m.slice_elem_ptr[s], ne = elem_found != nullptr ? m.slice_elem_ptr[s + 1] - e0 : 0; // (springs alone: no walk)
        const int row0 = s * kSliceNodes;
        const int my_row = tid / kSupWords, my_w = tid % kSupWords; // phase B: lanes 0 .. 191
        double sum = 0.0;
        for (int t0 = 0; t0 < ne; t0 += kSupTile) {
            const int nt = min(kSupTile, ne - t0);
            // ---- A: the words of B_e, and which rows of the slice every entry contains.  (Whole waves walk the tile, so that every
            //      lane takes part in the ballots below; a wave whose 64 entries lie past the tile's end skips them.)
            for (int i0 = tid - lane; i0 < nt; i0 += kSupThreads) {
                const int i = i0 + lane;
                uint32_t rows = 0; // bit r: node row0 + r belongs to the entry
                if (i < nt) {
                    const int4 c = m.slice_elem_nodes[e0 + t0 + i];
                    const int le = slice_elem_local[e0 + t0 + i];
                    const double2 k = elem_found[le]; // (kn, kt)
                    const double *pa = m.xyz + 3 * (int64_t)c.x, *pb = m.xyz + 3 * (int64_t)c.y, *pc = m.xyz + 3 * (int64_t)c.z;
                    double d1[3], d2[3], part;
                    if (!kHasQuads || c.w < 0) { // TRI3: (b - a) x (c - a), a third of the area to each node
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            d1[d] = pb[d] - pa[d];
                            d2[d] = pc[d] - pa[d];
                        }
                        part = 3.0;
                    } else { // QUAD4: the diagonals d1 = c - a, d2 = d - b, a quarter to each node
                        const double *pd = m.xyz + 3 * (int64_t)c.w;
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            d1[d] = pc[d] - pa[d];
                            d2[d] = pd[d] - pb[d];
                        }
                        part = 4.0;
                    }
                    const double cx = d1[1] * d2[2] - d1[2] * d2[1], cy = d1[2] * d2[0] - d1[0] * d2[2], cz = d1[0] * d2[1] - d1[1] * d2[0];
                    const double len = sqrt(cx * cx + cy * cy + cz * cz);
                    const double share = 0.5 * len / part;                           // (as k_lumped_mass forms it)
                    const double inv = len > 0.0 ? 1.0 / (2.0 * part * len) : 0.0; // n n^T share = c c^T / (2 part |c|)
                    const double iso = k.y * share, dk = k.x - k.y;
                    double *b = s_b + kSupWords * i;
                    b[0] = iso + dk * (cx * cx * inv);
                    b[1] = iso + dk * (cy * cy * inv);
                    b[2] = iso + dk * (cz * cz * inv);
                    b[3] = dk * (cx * cy * inv);
                    b[4] = dk * (cy * cz * inv);
                    b[5] = dk * (cz * cx * inv);
                    const int nid[4] = {c.x, c.y, c.z, kHasQuads ? c.w : -1};
#pragma unroll
                    for (int j = 0; j < 4; j++) entry_row_bit(nid[j], row0, rows); // (every node of the element gets the same block)
                }
                publish_rows(rows, lane, s_rows[i0 >> 6]);
            }
            __syncthreads();
            // ---- B: row sums in list order: waves of entries ascending, within one the set bits ascending
            if (tid < kSliceNodes * kSupWords) for_entries_of_row(s_rows, nt, my_row, [&](int i) { sum += s_b[kSupWords * i + my_w]; });
            __syncthreads(); // (the next tile overwrites the blocks)
        }
        if (tid < kSliceNodes * kSupWords) s_sum[tid] = sum;
        __syncthreads();
        if (tid < kSliceNodes) {
            const int a = row0 + tid;
            double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (a < m.n_own) {
#pragma unroll
                for (int d = 0; d < kSupWords; d++) v[d] = s_sum[kSupWords * tid + d];
                if (spring != nullptr) {
                    double k6[6];
                    load_node6(spring, a, false, k6);
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        v[d] += k6[d];
                        v[6 + d] = k6[3 + d];
                    }
                }
            }
            double *out = table + 9 * (int64_t)a;
#pragma unroll
            for (int d = 0; d < 9; d++) out[d] = v[d];
        }
        __syncthreads(); // (the next slice overwrites the row sums)
    }
}

void launch_support_rows(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *elem_found, const double *spring, double *table,
                         hipStream_t st)
{
    if (m.n_slices == 0) return;
    const int g = slice_grid(m);
    const double2 *ef = reinterpret_cast<const double2 *>(elem_found);
    if (m.n_lquad > 0) hipLaunchKernelGGL(k_support_rows<true>, dim3(g), dim3(kSupThreads), 0, st, m, slice_elem_local, ef, spring, table);
    else hipLaunchKernelGGL(k_support_rows<false>, dim3(g), dim3(kSupThreads), 0, st, m, slice_elem_local, ef, spring, table);
}

// the nine words of a row as the symmetric 3 x 3 block of the translations and the three rotational stiffnesses
struct SupportRow {
    double t[3][3], r[3];
};
__device__ __forceinline__ SupportRow load_support_row(const double *__restrict__ table, int a)
{
    const double *w = table + 9 * (int64_t)a;
    SupportRow s;
    s.t[0][0] = w[0];
    s.t[1][1] = w[1];
    s.t[2][2] = w[2];
    s.t[0][1] = s.t[1][0] = w[3];
    s.t[1][2] = s.t[2][1] = w[4];
    s.t[0][2] = s.t[2][0] = w[5];
    s.r[0] = w[6];
    s.r[1] = w[7];
    s.r[2] = w[8];
    return s;
}

// K + mask(K_sup): entry (i, j) of the row's diagonal block (slot 0 of the row) is component j & 1 of word (j / 2, i) -- the
// layout k_mass_shift and the assembly kernels write -- and receives one addition where neither dof i nor dof j of the node is
// fixed.  An off-diagonal entry has two images, (i, j) and (j, i): with full storage both are read and both get the addition;
// under DeviceMatrix::diag_upper the image below the diagonal gets it where it lies in a word that the assembly writes (entry
// (1, 0), beside (1, 1)), so that such a word stays the mirror of its image, and not in the never-written words.
__global__ __launch_bounds__(64) void k_support_add(DeviceMatrix m, const double *__restrict__ table)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= m.n_own) return;
    const int s = a / kSliceNodes, n = a % kSliceNodes;
    double *blk = m.vals + m.slice_base[s] * 36;
    const uint32_t fixed = m.dmask[a];
    const SupportRow sr = load_support_row(table, a);
    auto entry = [&](int i, int j) -> double * { return blk + (((j >> 1) * 6 + i) * kSliceNodes + n) * 2 + (j & 1); };
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) {
            if (((fixed >> i) | (fixed >> j)) & 1u) continue;
            *entry(i, j) += sr.t[i][j];
            if (j > i && (!m.diag_upper || 2 * (i >> 1) + 1 >= j)) *entry(j, i) += sr.t[i][j];
        }
#pragma unroll
    for (int i = 3; i < 6; i++)
        if (!((fixed >> i) & 1u)) *entry(i, i) += sr.r[i - 3];
}

void launch_support_add(const DeviceMatrix &m, const double *table, hipStream_t st)
{
    if (m.n_own == 0) return;
    hipLaunchKernelGGL(k_support_add, dim3((unsigned)((m.n_own + 63) / 64)), dim3(64), 0, st, m, table);
}

// y = base + s K_sup (x + xp) on the owned rows, zero on padding rows; base and xp may be nullptr.  Not masked.
__global__ __launch_bounds__(256) void k_support_apply(DeviceMatrix m, const double *__restrict__ table, const double *__restrict__ x,
                                                       const double *__restrict__ xp, const double *__restrict__ base, double s,
                                                       double *__restrict__ y)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    double out[6] = {0, 0, 0, 0, 0, 0};
    if (node < m.n_own) {
        const SupportRow sr = load_support_row(table, node);
        double u[6];
        load_node6(x, node, false, u);
        if (xp != nullptr) {
            double up[6];
            load_node6(xp, node, false, up);
#pragma unroll
            for (int i = 0; i < 6; i++) u[i] += up[i];
        }
        if (base != nullptr) load_node6(base, node, false, out);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double f = sr.t[i][0] * u[0] + sr.t[i][1] * u[1] + sr.t[i][2] * u[2];
            out[i] += s * f;
            out[3 + i] += s * (sr.r[i] * u[3 + i]);
        }
    }
    store_node6(y, node, false, out);
}

void launch_support_apply(const DeviceMatrix &m, const double *table, const double *x, const double *xp, const double *base, double s,
                          double *y, hipStream_t st)
{
    if (m.n_pad == 0) return;
    hipLaunchKernelGGL(k_support_apply, dim3((unsigned)((m.n_pad + 255) / 256)), dim3(256), 0, st, m, table, x, xp, base, s, y);
}

// lo[n_pad][6] = words 0-5 of every row, hi[n_pad][6] = words 6-8 and three zeros
__global__ __launch_bounds__(256) void k_support_words(DeviceMatrix m, const double *__restrict__ table, double *__restrict__ lo,
                                                       double *__restrict__ hi)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    double a[6] = {0, 0, 0, 0, 0, 0}, b[6] = {0, 0, 0, 0, 0, 0};
    if (node < m.n_own) {
        const double *w = table + 9 * (int64_t)node;
#pragma unroll
        for (int d = 0; d < 6; d++) a[d] = w[d];
#pragma unroll
        for (int d = 0; d < 3; d++) b[d] = w[6 + d];
    }
    store_node6(lo, node, false, a);
    store_node6(hi, node, false, b);
}

void launch_support_words(const DeviceMatrix &m, const double *table, double *lo, double *hi, hipStream_t st)
{
    if (m.n_pad == 0) return;
    hipLaunchKernelGGL(k_support_words, dim3((unsigned)((m.n_pad + 255) / 256)), dim3(256), 0, st, m, table, lo, hi);
}

} // namespace femshell
