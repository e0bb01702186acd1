// modal.hip -- gfx950 kernels of the modal analysis (femshell_modes, modal.hpp): K times a block of vectors with symmetric
// storage, Gram matrices of two blocks, the Rayleigh-Ritz rotation, block residuals, block-Jacobi on a block, start vectors.
// All FP64, HBM-bound streaming kernels like those of spmv_kernels.hip; no atomics, no device-side waiting, every loop bounded by plan
// data or by an argument.
#include "modal.hpp"
#include "plan.hpp"
#include "device_common.hpp"

#include <cstdlib>

namespace femshell {

typedef double v2d __attribute__((ext_vector_type(2)));

// the 18 words (jp, i) of block slot k, non-temporal (spmv_kernels.hip load_block_words: wd[jp * 6 + i] = columns 2jp, 2jp+1 of row i;
// kDiag: only the words of the upper triangle, the others stay unset)
// v: the 16-byte words of m.vals; slot = slot_base + k * 32 + n, so word e of the block lies at (slot_base + k * 32) * 18 + e * 32 + n
template <bool kDiag> __device__ __forceinline__ void load_block_words_nt(const v2d *v, int64_t slot, int n, v2d wd[18])
{
    const v2d *b = v + (slot * 18 - 17 * n);
#pragma unroll
    for (int e = 0; e < 18; e++)
        if (!kDiag || 2 * (e / 6) + 1 >= e % 6) wd[e] = __builtin_nontemporal_load(b + e * kSliceNodes);
}

// =====================================================================================
// Y = K X for kB columns, symmetric storage.  The mapping of k_spmv_sym: one wave per slice pair, one lane per node row, the
// diagonal slot read as its upper triangle.  The 18 words of a block are loaded once and used for every column: ya[j] += K_ac xc[j]
// for the lane's own row, u = K_ac^T xa[j] for row c -- into plane j of the transposed-product buffer, or into LDS when row c lies
// in the lane's own slice.  Registers: 72 for the block, 24 kB for xa / ya, xc and u per column.
// =====================================================================================
template <int kB>
__global__ __launch_bounds__(64) void k_spmm_sym(DeviceMatrix m, const double *__restrict__ X, double *__restrict__ Y, int64_t ld,
                                                 double *__restrict__ tbuf, int64_t plane)
{
    const int lane = threadIdx.x, half = lane >> 5, n = lane & 31;
    extern __shared__ double2 lds_block_products[]; // [half][kB][max_loc][3]
    const bool has_local = m.loc_index != nullptr;
    double2 *lu = lds_block_products + (size_t)half * kB * m.max_loc * 3;
    const int count = m.n_slices, n_pairs = (count + 1) >> 1;
    for (SliceWalk w(n_pairs); w.valid(); w.next()) {
        const int q = 2 * w.s + half;
        const bool live = q < count;
        const int sl = live ? q : 0;
        const int64_t base = m.slice_base[sl];
        const int W = live ? m.slice_width[sl] : 0;
        const int a = sl * kSliceNodes + n;
        double xa[kB][6], ya[kB][6];
#pragma unroll
        for (int j = 0; j < kB; j++) {
            load_node6(X + j * ld, a, false, xa[j]);
#pragma unroll
            for (int i = 0; i < 6; i++) ya[j][i] = 0.0;
        }
        const v2d *v = reinterpret_cast<const v2d *>(m.vals);
        if (W > 0) {
            v2d wd[18];
            load_block_words_nt<true>(v, base + n, n, wd);
#pragma unroll
            for (int j = 0; j < kB; j++)
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) {
                        const int r = jj >= i ? i : jj, cl = jj >= i ? jj : i; // (r, cl): the element of the upper triangle
                        const v2d kw = wd[(cl >> 1) * 6 + r];
                        ya[j][i] += ((cl & 1) ? kw.y : kw.x) * xa[j][jj];
                    }
        }
        for (int k = 1; k < W; k++) {
            const int64_t slot = base + (int64_t)k * kSliceNodes + n;
            const int c = m.cols[slot];
            v2d wd[18];
            load_block_words_nt<false>(v, slot, n, wd);
            // the transpose acts on row c when c is another owned row (ghost columns belong to another rank, padding slots point
            // at the own row)
            const bool transposed = c != a && c < m.n_pad;
            const int local = (transposed && has_local) ? (int)m.loc_index[slot] : 255;
#pragma unroll
            for (int j = 0; j < kB; j++) {
                double xc[6], u[6];
                load_node6(X + j * ld, c, false, xc);
#pragma unroll
                for (int jj = 0; jj < 6; jj++) u[jj] = 0.0;
#pragma unroll
                for (int jp = 0; jp < 3; jp++)
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const v2d kw = wd[jp * 6 + i];
                        ya[j][i] += kw.x * xc[2 * jp];
                        ya[j][i] += kw.y * xc[2 * jp + 1];
                        u[2 * jp] += kw.x * xa[j][i];
                        u[2 * jp + 1] += kw.y * xa[j][i];
                    }
                // (row c is a row of this slice: the product waits in LDS for the end of the slice, else next to the slot)
                if (transposed && local != 255) {
                    double2 *t = lu + (j * m.max_loc + local) * 3;
                    t[0] = make_double2(u[0], u[1]);
                    t[1] = make_double2(u[2], u[3]);
                    t[2] = make_double2(u[4], u[5]);
                } else if (transposed) {
                    double2 *t = reinterpret_cast<double2 *>(tbuf + j * plane) + slot * 3;
                    t[0] = make_double2(u[0], u[1]);
                    t[1] = make_double2(u[2], u[3]);
                    t[2] = make_double2(u[4], u[5]);
                }
            }
        }
        if (has_local) {
            // the transposed products of this slice's own rows, in the order of the in-list
            __syncthreads(); // (one wave per workgroup)
            const int Wi = live ? m.in_width[sl] : 0;
            const uint8_t *ll = m.loc_list + m.in_base[sl] + n;
            for (int k = 0; k < Wi; k++) {
                const int idx = ll[(size_t)k * kSliceNodes];
                if (idx != 255) {
#pragma unroll
                    for (int j = 0; j < kB; j++) {
                        const double2 *t = lu + (j * m.max_loc + idx) * 3;
                        const double2 t0 = t[0], t1 = t[1], t2 = t[2];
                        ya[j][0] += t0.x; ya[j][1] += t0.y; ya[j][2] += t1.x; ya[j][3] += t1.y; ya[j][4] += t2.x; ya[j][5] += t2.y;
                    }
                }
            }
            __syncthreads(); // the next slice overwrites the products
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < kB; j++) store_node6(Y + j * ld, a, false, ya[j]);
        }
    }
}

// second phase: every node row adds the transposed products of its in-list, in the plan's fixed order, for all columns
template <int kB>
__global__ __launch_bounds__(64) void k_spmm_gather(DeviceMatrix m, double *__restrict__ Y, int64_t ld, const double *__restrict__ tbuf,
                                                    int64_t plane)
{
    const int half = threadIdx.x >> 5, n = threadIdx.x & 31;
    for (SliceWalk w(node_pairs(m.n_slices)); w.valid(); w.next()) {
        const int sl = 2 * w.s + half;
        if (sl >= m.n_slices) continue;
        const int64_t node = (int64_t)sl * kSliceNodes + n;
        double acc[kB][6];
#pragma unroll
        for (int j = 0; j < kB; j++) load_node6(Y + j * ld, node, false, acc[j]);
        const int Wi = m.in_width[sl];
        const int64_t ib = m.in_base[sl];
        for (int k = 0; k < Wi; k++) {
            const int32_t slot = m.gat_slots[ib + (int64_t)k * kSliceNodes + n];
            if (slot < 0) continue;
#pragma unroll
            for (int j = 0; j < kB; j++) {
                double t[6];
                load_node6(tbuf + j * plane, slot, false, t);
#pragma unroll
                for (int i = 0; i < 6; i++) acc[j][i] += t[i];
            }
        }
#pragma unroll
        for (int j = 0; j < kB; j++) store_node6(Y + j * ld, node, false, acc[j]);
    }
}

constexpr size_t kSpmmLdsLimit = 64 * 1024; // dynamic LDS of a workgroup without raising the kernel's limit

int spmm_pass_cols(const DeviceMatrix &m)
{
    const size_t per_col = m.loc_index != nullptr ? (size_t)2 * m.max_loc * 48 : 0;
    int kb = kSpmmMaxCols;
    while (kb > 1 && per_col * kb > kSpmmLdsLimit) kb >>= 1;
    return kb;
}

template <int kB>
static void spmm_pass(const DeviceMatrix &m, const double *X, double *Y, int64_t ld, double *tbuf, int64_t plane, hipStream_t st)
{
    const size_t lds = m.loc_index != nullptr ? (size_t)2 * m.max_loc * 48 * kB : 0;
    const int pairs_grid = 8 * ((node_pairs(m.n_slices) + 7) / 8), cap = slice_grid(m);
    hipLaunchKernelGGL((k_spmm_sym<kB>), dim3(slice_grid(m)), dim3(64), lds, st, m, X, Y, ld, tbuf, plane);
    hipLaunchKernelGGL((k_spmm_gather<kB>), dim3(pairs_grid < cap ? pairs_grid : cap), dim3(64), 0, st, m, Y, ld, tbuf, plane);
}

bool launch_spmm_sym(const DeviceMatrix &m, const double *X, double *Y, int64_t ld, int n_cols, double *tbuf, int64_t plane, hipStream_t st)
{
    if (!m.symmetric || m.n_slices == 0) return false;
    const int kb = spmm_pass_cols(m);
    for (int j0 = 0; j0 < n_cols;) {
        const int left = n_cols - j0, nb = left < kb ? left : kb;
        const double *x = X + (int64_t)j0 * ld;
        double *y = Y + (int64_t)j0 * ld;
        switch (nb) {
        case 4: spmm_pass<4>(m, x, y, ld, tbuf, plane, st); break;
        case 3: spmm_pass<3>(m, x, y, ld, tbuf, plane, st); break;
        case 2: spmm_pass<2>(m, x, y, ld, tbuf, plane, st); break;
        default: spmm_pass<1>(m, x, y, ld, tbuf, plane, st); break;
        }
        j0 += nb;
    }
    return true;
}

void block_product(const DeviceMatrix &m, const double *X, double *Y, int64_t ld, int n_cols, double *tbuf, int64_t plane, hipStream_t st,
                   int *fused)
{
    // (FEMSHELL_SPMM_FUSED=0: the column-by-column path with symmetric storage too -- the yardstick of A/B measurements)
    if (knob_flag("FEMSHELL_SPMM_FUSED", true) && launch_spmm_sym(m, X, Y, ld, n_cols, tbuf, plane, st)) {
        if (fused) *fused = 1;
        return;
    }
    // full storage: the existing product, column by column
    for (int j = 0; j < n_cols; j++) launch_spmv(m, X + (int64_t)j * ld, Y + (int64_t)j * ld, SpmvEpilogue(), nullptr, st);
}

// =====================================================================================
// Gram matrices.  A workgroup walks its stretch of the rows in tiles of kGramTile rows; the tile of both operands (A times w) goes
// through LDS, every thread keeps a 6 x 6 tile of G in registers.  With few columns the 256 threads split the rows of a tile among
// nrg row groups (thread = (row group, tile of G)); their sums are added in the order of the row groups at the end.
// =====================================================================================
constexpr int kGramTile = 32, kGramStride = kModalMaxCols + 1; // (+1: the rows of a tile fall into different banks)

__global__ __launch_bounds__(256) void k_gram_partials(int64_t n_rows, int qa, const double *__restrict__ A, int qb, const double *__restrict__ B,
                                                       int64_t ld, const double *__restrict__ w, double *__restrict__ partials)
{
    __shared__ double tiles[2 * kGramTile * kGramStride];
    double *As = tiles, *Bs = tiles + kGramTile * kGramStride;
    const int t = threadIdx.x;
    const int nti = (qa + 5) / 6, ntj = (qb + 5) / 6, nt = nti * ntj;
    int nrg = 256 / nt;
    nrg = nrg > kGramTile ? kGramTile : nrg;
    const bool worker = t < nt * nrg;
    const int rg = worker ? t / nt : 0, tile = t % nt, ti = tile % nti, tj = tile / nti;
    const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x, r_begin = (int64_t)blockIdx.x * per;
    const int64_t r_end = r_begin + per < n_rows ? r_begin + per : n_rows;
    double acc[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) acc[i][j] = 0.0;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += kGramTile) {
        const int rows = r_end - r0 < kGramTile ? (int)(r_end - r0) : kGramTile;
        __syncthreads();
        for (int idx = t; idx < kGramTile * qa; idx += 256) {
            const int r = idx % kGramTile, c = idx / kGramTile;
            double v = 0.0;
            if (r < rows) {
                v = A[(int64_t)c * ld + r0 + r];
                if (w != nullptr) v *= w[r0 + r];
            }
            As[r * kGramStride + c] = v;
        }
        for (int idx = t; idx < kGramTile * qb; idx += 256) {
            const int r = idx % kGramTile, c = idx / kGramTile;
            Bs[r * kGramStride + c] = r < rows ? B[(int64_t)c * ld + r0 + r] : 0.0;
        }
        __syncthreads();
        if (worker) {
            for (int r = rg; r < rows; r += nrg) {
                double a[6], b[6];
#pragma unroll
                for (int e = 0; e < 6; e++) {
                    a[e] = ti * 6 + e < qa ? As[r * kGramStride + ti * 6 + e] : 0.0;
                    b[e] = tj * 6 + e < qb ? Bs[r * kGramStride + tj * 6 + e] : 0.0;
                }
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int j = 0; j < 6; j++) acc[i][j] += a[i] * b[j];
            }
        }
    }
    // the row groups' sums, added in their order (nrg >= 2 means nt <= 128: 36 nt doubles fit into the two tiles)
    for (int g = 1; g < nrg; g++) {
        __syncthreads();
        if (worker && rg == g) {
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) tiles[tile * 36 + i * 6 + j] = acc[i][j];
        }
        __syncthreads();
        if (worker && rg == 0) {
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) acc[i][j] += tiles[tile * 36 + i * 6 + j];
        }
    }
    if (worker && rg == 0) {
        double *out = partials + (int64_t)blockIdx.x * qa * qb;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++)
                if (ti * 6 + i < qa && tj * 6 + j < qb) out[(ti * 6 + i) * qb + tj * 6 + j] = acc[i][j];
    }
}

// G[e] = partials[0][e] + partials[1][e] + ... in index order
__global__ __launch_bounds__(256) void k_gram_sums(const double *__restrict__ partials, int n_partials, int n_entries, double *__restrict__ G)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    double s = 0.0;
    for (int g = 0; g < n_partials; g++) s += partials[(int64_t)g * n_entries + e];
    G[e] = s;
}

void launch_gram(const DeviceMatrix &m, int qa, const double *A, int qb, const double *B, int64_t ld, const double *w, double *partials,
                 double *G, hipStream_t st)
{
    if (qa <= 0 || qb <= 0 || qa > kModalMaxCols || qb > kModalMaxCols) return;
    static_assert(2 * kGramTile * kGramStride >= 128 * 36, "the row groups' sums go through the tiles");
    hipLaunchKernelGGL(k_gram_partials, dim3(kGramGrid), dim3(256), 0, st, (int64_t)m.n_own * 6, qa, A, qb, B, ld, w, partials);
    hipLaunchKernelGGL(k_gram_sums, dim3((unsigned)((qa * qb + 255) / 256)), dim3(256), 0, st, partials, kGramGrid, qa * qb, G);
}

// =====================================================================================
// Y = sum_k S_k C_k.  A workgroup of four waves takes tiles of 128 rows; a lane holds two consecutive rows (16-byte accesses), wave
// v the output columns v, v + 4, ... (at most 16: 64 output columns).  The source columns of a tile pass through LDS in chunks of
// 32, each read from HBM once; the coefficients are uniform in a wave.
// =====================================================================================
constexpr int kCombineChunk = 32, kCombineOutPerWave = 16;

__global__ __launch_bounds__(256) void k_block_combine(int64_t n_rows, CombineSources src, int ldc, int n_out, double *__restrict__ Y, int64_t ld)
{
    __shared__ double2 tile[kCombineChunk * 64];
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t n_tiles = (n_rows + 127) / 128;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t row0 = tl * 128;
        double2 acc[kCombineOutPerWave];
#pragma unroll
        for (int e = 0; e < kCombineOutPerWave; e++) acc[e] = make_double2(0.0, 0.0);
        for (int k = 0; k < 3; k++) {
            const double *S = src.S[k], *Cm = src.C[k];
            const int qk = src.q[k];
            for (int s0 = 0; s0 < qk; s0 += kCombineChunk) {
                const int ns = qk - s0 < kCombineChunk ? qk - s0 : kCombineChunk;
                __syncthreads();
                for (int idx = t; idx < ns * 64; idx += 256) {
                    const int rp = idx & 63, c = idx >> 6;
                    const int64_t row = row0 + 2 * rp;
                    tile[c * 64 + rp] = row < n_rows ? *reinterpret_cast<const double2 *>(S + (int64_t)(s0 + c) * ld + row) : make_double2(0.0, 0.0);
                }
                __syncthreads();
                for (int c = 0; c < ns; c++) {
                    const double2 v = tile[c * 64 + lane];
                    const double *crow = Cm + (int64_t)(s0 + c) * ldc;
#pragma unroll
                    for (int e = 0; e < kCombineOutPerWave; e++) {
                        const int o = wv + 4 * e;
                        if (o < n_out) {
                            const double cf = crow[o];
                            acc[e].x += v.x * cf;
                            acc[e].y += v.y * cf;
                        }
                    }
                }
            }
        }
        const int64_t row = row0 + 2 * lane;
        if (row < n_rows) {
#pragma unroll
            for (int e = 0; e < kCombineOutPerWave; e++) {
                const int o = wv + 4 * e;
                if (o < n_out) *reinterpret_cast<double2 *>(Y + (int64_t)o * ld + row) = acc[e];
            }
        }
    }
}

void launch_block_combine(const DeviceMatrix &m, const CombineSources &src, int ldc, int n_out, double *Y, int64_t ld, hipStream_t st)
{
    const int64_t n_rows = (int64_t)m.n_pad * 6; // (even: a multiple of 192)
    if (n_rows == 0 || n_out <= 0 || n_out > 4 * kCombineOutPerWave) return;
    const int64_t n_tiles = (n_rows + 127) / 128;
    hipLaunchKernelGGL(k_block_combine, dim3((unsigned)(n_tiles < 8192 ? n_tiles : 8192)), dim3(256), 0, st, n_rows, src, ldc, n_out, Y, ld);
}

// =====================================================================================
// residuals, block-Jacobi, mask, start vectors: one lane per node, 48 bytes per node and column
// =====================================================================================
__global__ __launch_bounds__(256) void k_block_residual(DeviceMatrix m, const double *__restrict__ KX, const double *__restrict__ X,
                                                        const double *__restrict__ mass, const double *__restrict__ theta,
                                                        const int32_t *__restrict__ cols, double *__restrict__ R, int64_t ld,
                                                        double *__restrict__ partials)
{
    __shared__ double sh[4];
    const int col = cols[blockIdx.y];
    const double th = theta[col];
    const int per = (m.n_pad + gridDim.x - 1) / gridDim.x, b = blockIdx.x * per, e = min(b + per, m.n_pad);
    double sum = 0.0;
    for (int node = b + threadIdx.x; node < e; node += blockDim.x) {
        double r[6] = {0, 0, 0, 0, 0, 0};
        if (node < m.n_own) {
            const uint32_t fixed = m.dmask[node];
            double kx[6], x[6], mv[6];
            load_node6(KX + (int64_t)col * ld, node, false, kx);
            load_node6(X + (int64_t)col * ld, node, false, x);
            load_node6(mass, node, false, mv);
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const bool free_dof = !((fixed >> i) & 1u);
                r[i] = free_dof ? kx[i] - th * (mv[i] * x[i]) : 0.0;
                if (free_dof && mv[i] > 0.0) sum += r[i] * r[i] / mv[i];
            }
        }
        store_node6(R + (int64_t)blockIdx.y * ld, node, false, r);
    }
    sum = block_sum(sum, sh);
    if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}
// norms[i] = the partial sums of column i in index order
__global__ __launch_bounds__(64) void k_block_residual_sums(const double *__restrict__ partials, int G, int n, double *__restrict__ norms)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int g = 0; g < G; g++) s += partials[(int64_t)i * G + g];
    norms[i] = s;
}

void launch_block_residual(const DeviceMatrix &m, const double *KX, const double *X, const double *mass, const double *theta,
                           const int32_t *cols, int n, double *R, int64_t ld, double *partials, double *norms, hipStream_t st)
{
    if (n <= 0 || m.n_pad == 0) return;
    hipLaunchKernelGGL(k_block_residual, dim3(kGramGrid, (unsigned)n), dim3(256), 0, st, m, KX, X, mass, theta, cols, R, ld, partials);
    hipLaunchKernelGGL(k_block_residual_sums, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, partials, kGramGrid, n, norms);
}

__global__ __launch_bounds__(64) void k_block_bj(DeviceMatrix m, const double *__restrict__ R, double *__restrict__ Z, int64_t ld, int n)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    const bool owned = node < m.n_own;
    const uint32_t fixed = owned ? m.dmask[node] : 0x3Fu;
    double mv[kMinvWords];
    if (owned) node_minv(m, node / kSliceNodes, node % kSliceNodes, false, mv);
    for (int j = 0; j < n; j++) {
        double z[6] = {0, 0, 0, 0, 0, 0};
        if (owned) {
            double r[6];
            load_node6(R + (int64_t)j * ld, node, false, r);
            node_minv_apply(mv, r, z);
#pragma unroll
            for (int i = 0; i < 6; i++) z[i] = ((fixed >> i) & 1u) ? 0.0 : z[i];
        }
        store_node6(Z + (int64_t)j * ld, node, false, z);
    }
}

void launch_block_bj(const DeviceMatrix &m, const double *R, double *Z, int64_t ld, int n, hipStream_t st)
{
    if (n <= 0 || m.n_pad == 0) return;
    hipLaunchKernelGGL(k_block_bj, dim3((unsigned)((m.n_pad + 63) / 64)), dim3(64), 0, st, m, R, Z, ld, n);
}

__global__ __launch_bounds__(256) void k_block_mask(DeviceMatrix m, double *__restrict__ X, int64_t ld)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    const uint32_t fixed = node < m.n_own ? m.dmask[node] : 0x3Fu;
    if (fixed == 0u) return;
    double x[6];
    load_node6(X + (int64_t)blockIdx.y * ld, node, false, x);
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = ((fixed >> i) & 1u) ? 0.0 : x[i];
    store_node6(X + (int64_t)blockIdx.y * ld, node, false, x);
}

void launch_block_mask(const DeviceMatrix &m, double *X, int64_t ld, int n, hipStream_t st)
{
    if (n <= 0 || m.n_pad == 0) return;
    hipLaunchKernelGGL(k_block_mask, dim3((unsigned)((m.n_pad + 255) / 256), (unsigned)n), dim3(256), 0, st, m, X, ld);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void k_modal_init(DeviceMatrix m, const int32_t *__restrict__ node_ids, double *__restrict__ X, int64_t ld)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    const int col = blockIdx.y;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (node < m.n_own) {
        const uint32_t fixed = m.dmask[node];
        const uint64_t id = (uint64_t)(node_ids != nullptr ? node_ids[node] : node);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const uint64_t h = splitmix64(splitmix64(id * 6ull + (uint64_t)i) ^ ((uint64_t)col * 0xD1B54A32D192ED03ull));
            // the upper 53 bits, centred in their cell: (0, 1), then (-1, 1) with both ends excluded
            const double u01 = ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);
            x[i] = ((fixed >> i) & 1u) ? 0.0 : 2.0 * u01 - 1.0;
        }
    }
    store_node6(X + (int64_t)col * ld, node, false, x);
}

void launch_modal_init(const DeviceMatrix &m, const int32_t *node_ids, int n_cols, double *X, int64_t ld, hipStream_t st)
{
    if (n_cols <= 0 || m.n_pad == 0) return;
    hipLaunchKernelGGL(k_modal_init, dim3((unsigned)((m.n_pad + 255) / 256), (unsigned)n_cols), dim3(256), 0, st, m, node_ids, X, ld);
}

} // namespace femshell
