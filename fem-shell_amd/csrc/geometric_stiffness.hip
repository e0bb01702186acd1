// geometric_stiffness.hip -- the geometric (initial-stress) stiffness K_G(N) of linear buckling, matrix-free (gfx950, wave64).
// DESIGN.md 8g has the definition:
//     g_ab = sum_gp w_gp grad phi_a(gp)^T [[Nxx, Nxy], [Nxy, Nyy]] grad phi_b(gp),   K_G,e[a, b] = g_ab I3 on the translations,
// N the element-mean membrane force of k_element_resultants, phi the membrane shape functions (TRI3: linear, one point of weight
// A; QUAD4: bilinear at the stiffness's 2 x 2 Gauss points, weight det J).
//
// k_geometric_coeff: one lane per local element (the mapping and grid of k_element_resultants, which runs in front and leaves N in
// global axes).  TRI3 needs no frame: the in-plane gradient of phi_a is n x e_a / 2A (e_a the side opposite node a), so with
// cr = (b - a) x (c - a) and h_a = cr x e_a, g_ab = h_a^T N h_b / (2 |cr|^3).  QUAD4 builds the frame of the stiffness, takes N
// back into it (ex.N ex, ey.N ey, ex.N ey) and sums the four points.  The unique g_ab of an element go to HBM in the local element
// order: 6 doubles on a mesh of triangles, 10 where the mesh has quadrilaterals (a triangle's fourth row and column zero).
//
// k_geometric_product: Y = K_G X for kCols columns.  One workgroup per slice (32 node rows), over the slice's element list in
// tiles of kGpTile entries:
//   A  one lane per list entry loads the node ids, the entry's coefficient row (16-byte loads, through its local element index)
//      and the translations of its nodes, forms for every node a of the entry the 3-vector sum_b g_ab x_b per column and leaves it
//      in LDS; beside it which rows of the slice the entry contains, turned round by one ballot per row (the incidence words of
//      k_element_loads), and at which of its nodes;
//   B  one lane per (row, translation, column) walks the tile IN LIST ORDER over the set bits of its row's words and adds.
// The row sum stays in the lane's register from tile to tile: the order of the additions is the list order whatever the tile
// is, there are no atomics, and two launches give the same bits.  The products of a column are the same chain of fma whatever
// kCols is: column j of a block product is bitwise the single-column product.
#include "geometric_stiffness.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "k_geometric_product assumes 32-node slices");

constexpr int kGcThreads = 256; // k_geometric_coeff: one lane per element
constexpr int kGpTile = 128;    // entries per tile of k_geometric_product: at most 4 nodes x 3 x 4 columns doubles of LDS each, 48 KB
// lanes of a workgroup: phase B wants 96 kCols, whole waves, and phase A at least one wave per 64 entries of a tile
__host__ __device__ constexpr int geo_threads(int cols) { return cols == 1 ? 128 : 64 * ((96 * cols + 63) / 64); }

namespace {

// index of g_ab, a <= b, in the row-by-row upper triangle of an n x n matrix
__host__ __device__ constexpr int tri_index(int n, int a, int b) { return a * n - (a * (a - 1)) / 2 + (b - a); }
__host__ __device__ constexpr int sym_index(int n, int a, int b) { return a <= b ? tri_index(n, a, b) : tri_index(n, b, a); }

// N (xx yy zz xy yz zx) times a vector
__device__ __forceinline__ void sym_apply(const double N[6], const double h[3], double out[3])
{
    out[0] = N[0] * h[0] + N[3] * h[1] + N[5] * h[2];
    out[1] = N[3] * h[0] + N[1] * h[1] + N[4] * h[2];
    out[2] = N[5] * h[0] + N[4] * h[1] + N[2] * h[2];
}

template <int kN> __device__ __forceinline__ bool tri3_coeff(const double X[9], const double N[6], double g[])
{
    double e[3][3], cr[3]; // e[a]: the side opposite node a
#pragma unroll
    for (int d = 0; d < 3; d++) {
        e[0][d] = X[6 + d] - X[3 + d];
        e[1][d] = X[d] - X[6 + d];
        e[2][d] = X[3 + d] - X[d];
    }
    // (b - a) x (c - a) = e2 x (-e1)
    cr[0] = e[1][1] * e[2][2] - e[1][2] * e[2][1];
    cr[1] = e[1][2] * e[2][0] - e[1][0] * e[2][2];
    cr[2] = e[1][0] * e[2][1] - e[1][1] * e[2][0];
    const double c2 = cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2];
    const bool ok = c2 > 0.0;
    const double s = ok ? 0.5 / (c2 * sqrt(c2)) : 0.0;
    double h[3][3], Nh[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        h[a][0] = cr[1] * e[a][2] - cr[2] * e[a][1];
        h[a][1] = cr[2] * e[a][0] - cr[0] * e[a][2];
        h[a][2] = cr[0] * e[a][1] - cr[1] * e[a][0];
        sym_apply(N, h[a], Nh[a]);
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++) g[tri_index(kN, a, b)] = ok ? s * (h[a][0] * Nh[b][0] + h[a][1] * Nh[b][1] + h[a][2] * Nh[b][2]) : 0.0;
    return ok;
}

__device__ __forceinline__ bool quad4_coeff(const double X[12], const double N[6], double g[10])
{
    QuadFrame f;
    bool ok = quad4_frame(X, f);
    const double *ex = f.ex, *ey = f.ey;
    // N in the element frame
    double Nx[3], Ny[3];
    sym_apply(N, ex, Nx);
    sym_apply(N, ey, Ny);
    const double nxx = ex[0] * Nx[0] + ex[1] * Nx[1] + ex[2] * Nx[2], nyy = ey[0] * Ny[0] + ey[1] * Ny[1] + ey[2] * Ny[2];
    const double nxy = ex[0] * Ny[0] + ex[1] * Ny[1] + ex[2] * Ny[2];
#pragma unroll
    for (int q = 0; q < 10; q++) g[q] = 0.0;
#pragma unroll
    for (int gp = 0; gp < 4; gp++) {
        const QuadGauss gq = quad4_gauss(f, gp, ok);
        ok = ok && gq.det != 0.0; // (a vanishing determinant at one Gauss point rejects the element)
        double bx[4], by[4], sx[4], sy[4];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            bilinear_grad(n, gq.r, gq.s, gq.Ji, bx[n], by[n]);
            sx[n] = gq.det * (nxx * bx[n] + nxy * by[n]); // w N grad phi_b
            sy[n] = gq.det * (nxy * bx[n] + nyy * by[n]);
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = a; b < 4; b++) g[tri_index(4, a, b)] += bx[a] * sx[b] + by[a] * sy[b];
    }
#pragma unroll
    for (int q = 0; q < 10; q++) g[q] = ok ? g[q] : 0.0; // (selects: a degenerate element's values may be Inf / NaN)
    return ok;
}

} // namespace

template <bool kHasQuads>
__global__ __launch_bounds__(kGcThreads) void k_geometric_coeff(DeviceMatrix m, const double *__restrict__ res, double *__restrict__ coeff)
{
    constexpr int kN = kHasQuads ? 4 : 3, kW = kHasQuads ? 10 : 6;
    const int n = m.n_ltri + (kHasQuads ? m.n_lquad : 0);
    const int64_t e64 = (int64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (e64 >= n) return;
    const int e = (int)e64;
    double N[6];
    {
        const double2 *r = reinterpret_cast<const double2 *>(res + 14 * e64); // (112 bytes per row: 16-byte aligned)
        const double2 a0 = r[0], a1 = r[1], a2 = r[2];
        N[0] = a0.x; N[1] = a0.y; N[2] = a1.x; N[3] = a1.y; N[4] = a2.x; N[5] = a2.y;
    }
    double g[kW];
#pragma unroll
    for (int q = 0; q < kW; q++) g[q] = 0.0;
    bool ok;
    if (!kHasQuads || e < m.n_ltri) {
        const int32_t *c = m.tri + 3 * e64;
        const int nid[3] = {c[0], c[1], c[2]};
        double X[9];
        load_xyz<3>(m.xyz, nid, X);
        ok = tri3_coeff<kN>(X, N, g);
    } else {
        const int4 c = reinterpret_cast<const int4 *>(m.quad)[e - m.n_ltri];
        const int nid[4] = {c.x, c.y, c.z, c.w};
        double X[12];
        load_xyz<4>(m.xyz, nid, X);
        relative_to_first(X);
        ok = quad4_coeff(X, N, g);
    }
    if (!ok) report_status(m.status, kStatusDirect + e);
    double2 *row = reinterpret_cast<double2 *>(coeff + (int64_t)kW * e64);
#pragma unroll
    for (int q = 0; q < kW / 2; q++) row[q] = make_double2(g[2 * q], g[2 * q + 1]);
}

template <bool kHasQuads, int kCols>
__global__ __launch_bounds__(geo_threads(kCols)) void k_geometric_product(DeviceMatrix m, const int32_t *__restrict__ slice_elem_local,
                                                                          const double2 *__restrict__ coeff, const double *__restrict__ X,
                                                                          double *__restrict__ Y, int64_t ld, int solver)
{
    constexpr int kThreads = geo_threads(kCols);
    constexpr int kN = kHasQuads ? 4 : 3, kW = kHasQuads ? 10 : 6;
    constexpr int kRowItems = 3 * kCols;    // (translation, column) of a row
    constexpr int kEntry = kN * kRowItems;  // doubles of LDS per list entry
    static_assert(kGpTile % 64 == 0 && kThreads % 64 == 0 && kThreads >= kSliceNodes * kRowItems, "whole waves; a lane per (row, translation, column)");
    __shared__ double s_y[kGpTile * kEntry];
    __shared__ unsigned long long s_rows[kGpTile / 64][kSliceNodes]; // per wave of entries and row: the entries that contain the row
    __shared__ uint32_t s_node[kGpTile];                             // per entry: byte j = the slice row of its node j (0xFF: none)
    __shared__ double s_sum[kSliceNodes * kRowItems];
    const int tid = threadIdx.x, lane = tid & 63;
    SliceWalk w(m.n_slices);
    for (; w.valid(); w.next()) {
        const int s = w.s;
        const int e0 = m.slice_elem_ptr[s], ne = m.slice_elem_ptr[s + 1] - e0;
        const int row0 = s * kSliceNodes;
        const int my_row = tid / kRowItems, my_item = tid % kRowItems; // phase B: lanes 0 .. 96 kCols - 1
        double sum = 0.0;
        for (int t0 = 0; t0 < ne; t0 += kGpTile) {
            const int nt = min(kGpTile, ne - t0);
            // ---- A: the entries' products, and which rows of the slice every entry contains.  (Whole waves walk the tile, so
            //      that every lane takes part in the ballots below.)
            for (int i0 = tid - lane; i0 < nt; i0 += kThreads) {
                const int i = i0 + lane;
                uint32_t rows = 0; // bit r: node row0 + r belongs to the entry
                if (i < nt) {
                    const int4 c = m.slice_elem_nodes[e0 + t0 + i];
                    const int le = slice_elem_local[e0 + t0 + i];
                    const double2 *cg = coeff + (kW / 2) * (int64_t)le;
                    double g[kW];
#pragma unroll
                    for (int q = 0; q < kW / 2; q++) {
                        const double2 v = cg[q];
                        g[2 * q] = v.x;
                        g[2 * q + 1] = v.y;
                    }
                    const int nid[4] = {c.x, c.y, c.z, kHasQuads ? c.w : -1};
                    uint32_t word = 0xFFFFFFFFu;
#pragma unroll
                    for (int j = 0; j < kN; j++) entry_node(j, nid[j], row0, rows, word);
                    s_node[i] = word;
#pragma unroll
                    for (int col = 0; col < kCols; col++) {
                        const double *xc = X + (int64_t)col * ld;
                        double x[kN][3];
#pragma unroll
                        for (int b = 0; b < kN; b++) {
                            if (nid[b] >= 0) { // (the fourth node of a triangle on a mesh with quadrilaterals: its g row is zero)
                                const double *px = xc + 6 * (int64_t)nid[b];
                                const double2 x01 = *reinterpret_cast<const double2 *>(px);
                                x[b][0] = x01.x;
                                x[b][1] = x01.y;
                                x[b][2] = px[2];
                            } else {
                                x[b][0] = x[b][1] = x[b][2] = 0.0;
                            }
                        }
#pragma unroll
                        for (int a = 0; a < kN; a++)
#pragma unroll
                            for (int v = 0; v < 3; v++) {
                                double acc = g[sym_index(kN, a, 0)] * x[0][v]; // one chain of fma per value, the same for every kCols
#pragma unroll
                                for (int b = 1; b < kN; b++) acc = fma(g[sym_index(kN, a, b)], x[b][v], acc);
                                s_y[i * kEntry + a * kRowItems + v * kCols + col] = acc;
                            }
                    }
                }
                publish_rows(rows, lane, s_rows[i0 >> 6]);
            }
            __syncthreads();
            // ---- B: row sums in list order: waves of entries ascending, within one the set bits ascending
            if (tid < kSliceNodes * kRowItems)
                for_entries_of_row(s_rows, nt, my_row, [&](int i) {
                    sum += s_y[i * kEntry + entry_node_of_row(s_node[i], (uint32_t)my_row) * kRowItems + my_item];
                });
            __syncthreads(); // (the next tile overwrites the products)
        }
        if (tid < kSliceNodes * kRowItems) s_sum[tid] = sum;
        __syncthreads();
        if (tid < kSliceNodes * kCols) {
            const int col = tid / kSliceNodes, r = tid % kSliceNodes;
            const int a = row0 + r;
            double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (a < m.n_own) {
                const uint32_t fixed = solver ? m.dmask[a] : 0u;
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const double t = s_sum[r * kRowItems + d * kCols + col];
                    v[d] = solver ? (((fixed >> d) & 1u) ? 0.0 : -t) : t;
                }
            }
            store_node6(Y + (int64_t)col * ld, a, false, v);
        }
        __syncthreads(); // (the next slice overwrites the row sums)
    }
}

void launch_geometric_coeff(const DeviceMatrix &m, const double *res, double *coeff, hipStream_t st)
{
    const int64_t n = (int64_t)m.n_ltri + m.n_lquad;
    if (n == 0) return;
    const unsigned g = (unsigned)((n + kGcThreads - 1) / kGcThreads);
    if (m.n_lquad > 0) hipLaunchKernelGGL(k_geometric_coeff<true>, dim3(g), dim3(kGcThreads), 0, st, m, res, coeff);
    else hipLaunchKernelGGL(k_geometric_coeff<false>, dim3(g), dim3(kGcThreads), 0, st, m, res, coeff);
}

namespace {

template <bool kHasQuads>
void geometric_pass(const DeviceMatrix &m, const int32_t *slice_elem_local, const double2 *coeff, const double *X, double *Y, int64_t ld, int nc,
                    int solver, int g, hipStream_t st)
{
    switch (nc) {
    case 1: hipLaunchKernelGGL((k_geometric_product<kHasQuads, 1>), dim3(g), dim3(geo_threads(1)), 0, st, m, slice_elem_local, coeff, X, Y, ld, solver); break;
    case 2: hipLaunchKernelGGL((k_geometric_product<kHasQuads, 2>), dim3(g), dim3(geo_threads(2)), 0, st, m, slice_elem_local, coeff, X, Y, ld, solver); break;
    case 3: hipLaunchKernelGGL((k_geometric_product<kHasQuads, 3>), dim3(g), dim3(geo_threads(3)), 0, st, m, slice_elem_local, coeff, X, Y, ld, solver); break;
    default: hipLaunchKernelGGL((k_geometric_product<kHasQuads, 4>), dim3(g), dim3(geo_threads(4)), 0, st, m, slice_elem_local, coeff, X, Y, ld, solver); break;
    }
}

} // namespace

void launch_geometric_product(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *coeff, const double *X, double *Y,
                              int64_t ld, int n_cols, bool solver, hipStream_t st)
{
    if (m.n_slices == 0 || n_cols < 1) return;
    const int g = slice_grid(m);
    const double2 *cg = reinterpret_cast<const double2 *>(coeff);
    for (int c0 = 0; c0 < n_cols; c0 += kGeoMaxCols) {
        const int nc = n_cols - c0 < kGeoMaxCols ? n_cols - c0 : kGeoMaxCols;
        const double *x = X + (int64_t)c0 * ld;
        double *y = Y + (int64_t)c0 * ld;
        if (m.n_lquad > 0) geometric_pass<true>(m, slice_elem_local, cg, x, y, ld, nc, solver ? 1 : 0, g, st);
        else geometric_pass<false>(m, slice_elem_local, cg, x, y, ld, nc, solver ? 1 : 0, g, st);
    }
    if (m.n_ghost > 0) // the ghost space of every column
        for (int j = 0; j < n_cols; j++)
            (void)hipMemsetAsync(Y + (int64_t)j * ld + (int64_t)m.n_pad * 6, 0, (size_t)m.n_ghost * 6 * sizeof(double), st);
}

} // namespace femshell
