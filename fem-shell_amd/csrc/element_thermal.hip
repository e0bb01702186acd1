// element_thermal.hip -- nodal equivalents of per-element temperatures (femshell_set_thermal; gfx950, wave64).  DESIGN.md 8j.
//
// Per element two doubles (Tm, Tg): the temperature change of the mid-surface and the difference top - bottom, top at z = +t/2
// along the element's own ez.  The free thermal state is eps0 = alpha Tm (1,1,0), kappa0 = -(alpha Tg / t) (1,1,0); the loads are
// work-equivalent, with the element's own strain operators and the quadrature of its stiffness:
//     f_m = N_T sum_g w_g Bm_g^T (1,1,0),  N_T = E t alpha Tm / (1 - nu),
//     f_p = -M_T sum_g w_g Bp_g^T (1,1,0), M_T = E t^2 alpha Tg / (12 (1 - nu)).
//   TRI3   f_m of node i is N_T / 2 times (y, -x) of the opposite side (the CST operator times the area: no division by it);
//          f_p takes the Gauss-point sum of Specht's operator as element_resultants.hip forms it -- through sQ_n = sum_g Q_n(g) --
//          TRANSPOSED and applied to Y^T (1,1,0), whose third component is what Y's row 2 multiplies: the kRefY21 switch of the
//          stiffness's Y does not reach it.
//   QUAD4  the det-J-weighted sums over the 2 x 2 Gauss points of the bilinear membrane operator and of MINUS the DKQ operator.
// Local (u, v, w) and (tx, ty) go to global axes with the element frame; the drilling row gets nothing.
//
// One workgroup per slice (32 node rows), over the slice's element list in tiles of kThTile entries:
//   A  one lane per list entry gathers the element's node ids, coordinates, (Tm, Tg) as one 16-byte load through the entry's
//      local element index, and the section's two constants; it builds the frame and leaves the element's per-node 6-vectors --
//      they differ from node to node and fill the rotational rows: 18 doubles for a triangle, 24 for a quadrilateral -- in LDS,
//      beside a word that says which row of the slice each of its nodes is.  One ballot per row turns the membership round, as in
//      k_element_loads;
//   B  one lane per (row, component), 192 lanes, walks the tile IN LIST ORDER and adds, of every entry that contains its row, the
//      6-vector of the node that IS the row.  The row sum stays in the lane's register from tile to tile: the order of the
//      additions is the list order whatever the tile and the grid are, there are no atomics, two launches give the same bits.
// Then one lane per row writes base + T on all six components (base == nullptr: zero); padding rows write zero.  A degenerate
// element contributes the finite zeros its zero scale factors give and reports nothing (the assembly reports it).
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "k_element_thermal assumes 32-node slices");

constexpr int kThThreads = 192; // phase B: one lane per (row, component)
constexpr int kThTile = 192;    // entries per tile: one round of the workgroup in phase A
static_assert(kThTile % kThThreads == 0 && kThThreads % 64 == 0 && kThThreads >= kSliceRows, "k_element_thermal: whole waves, whole rounds");
// doubles per entry in LDS: 18 / 24 and one of padding -- an odd count, so that the lanes of a wave, which write the same field
// of consecutive entries, spread over all banks (24 doubles = 48 dwords would leave them four)
template <bool kHasQuads> constexpr int th_stride() { return kHasQuads ? 25 : 19; }
static_assert(kThTile * 25 * 8 + kThTile * 4 + (kThTile / 64) * kSliceNodes * 8 + kSliceRows * 8 < 64 * 1024, "static LDS of k_element_thermal");

namespace {

// global 6-vector of one node from its local (fu, fv, fw) and (ftx, fty)
__device__ __forceinline__ void put_node(double *dst, const double ex[3], const double ey[3], const double ez[3], double fu, double fv, double fw,
                                         double ftx, double fty)
{
#pragma clang fp reassociate(on) contract(fast)
#pragma unroll
    for (int d = 0; d < 3; d++) {
        dst[d] = ex[d] * fu + ey[d] * fv + ez[d] * fw;
        dst[3 + d] = ex[d] * ftx + ey[d] * fty;
    }
}

// the three 6-vectors of a triangle: nt = N_T, mt = M_T
__device__ __forceinline__ void tri3_thermal(const double X[9], double nt, double mt, double *dst)
{
#pragma clang fp reassociate(on) contract(fast) // element math only; parity bar is 1e-12, not bitwise
    constexpr SpechtSums kS = specht_sums();
    constexpr double kC[3][3] = SPECHT_C456_INIT;
    TriFrame f;
    const bool ok = tri3_frame(X, f); // degenerate: zero scale factors, everything below is a finite zero
    double mu[3];
    specht_mu(f, ok, mu);
    // -M_T A Y^T (1,1,0): rows 0 and 1 of Y (SA:578-588), A / (4 A^2) = inv2a / 2
    const double x31 = f.xs[1], y31 = f.ys[1], x23 = f.xs[2], y23 = f.ys[2];
    const double sp = -mt * (0.5 * f.inv2a);
    const double yv[3] = {sp * (y23 * y23 + x23 * x23), sp * (y31 * y31 + x31 * x31), sp * (y23 * y31 + x31 * x23)};
    double aQ[3], aC[3]; // mean Q_n and C_n against it
#pragma unroll
    for (int n = 0; n < 3; n++) {
        aQ[n] = 0.0;
        aC[n] = 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            aQ[n] += ((kS.a[n][r] + mu[(n + 2) % 3] * kS.b[n][r]) * (1.0 / 3.0)) * yv[r];
            aC[n] += kC[n][r] * yv[r];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int k = tri_prev(i);
        const double xki = f.xs[tri_row_ki(i)], yki = f.ys[tri_row_ki(i)], xji = -f.xs[tri_row_ji(i)], yji = -f.ys[tri_row_ji(i)];
        // the transposes of u_i = (2, y_ji, -x_ji), v_i = (-2, -y_ki, x_ki), e0 + w_i = (1, y_ki, -x_ki), -e0
        const double a = aQ[i], b = aQ[k], ck = aC[k], ci = aC[i];
        const double fw = 2.0 * (a - b) + (ck - ci);
        const double ftx = yji * a + yki * (ck - b);
        const double fty = -(xji * a + xki * (ck - b));
        // membrane: N_T A (beta_i, gamma_i) / (2A), beta_i = y of row 2 - i, gamma_i = -x of that row
        put_node(dst + 6 * i, f.ex, f.ey, f.ez, 0.5 * nt * f.ys[2 - i], -0.5 * nt * f.xs[2 - i], fw, ftx, fty);
    }
}

// the four 6-vectors of a quadrilateral; X relative to its first node (as k_element_resultants hands it to quad4_means)
__device__ __forceinline__ void quad4_thermal(const double X[12], double nt, double mt, double *dst)
{
#pragma clang fp reassociate(on) contract(fast) // element math only; parity bar is 1e-12, not bitwise
    QuadFrame f;
    const bool ok = quad4_frame(X, f);
    DkqSide sd[4];
    dkq_sides(f, ok, sd);
    double fm[4][2], fp[4][3];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        fm[n][0] = fm[n][1] = 0.0;
        fp[n][0] = fp[n][1] = fp[n][2] = 0.0;
    }
#pragma unroll 1 // (one copy of the Gauss-point code: the register budget, as in quad4_means)
    for (int gp = 0; gp < 4; gp++) {
        const QuadGauss g = quad4_gauss(f, gp, ok);
        const double wdet = ok ? g.det : 0.0;
#pragma unroll
        for (int n = 0; n < 4; n++) {
            double bx, by; // Bm^T (1,1,0) = (dN/dx, dN/dy)
            bilinear_grad(n, g.r, g.s, g.Ji, bx, by);
            fm[n][0] += wdet * bx;
            fm[n][1] += wdet * by;
            const int np = (n + 3) & 3;
            const double rn = quad_corner_r(n), sn = quad_corner_s(n);
            double B[3][3];
            dkq_node_block(sd[n], sd[np], dkq_corner_x(g.r, g.s, rn, sn), dkq_corner_e(g.r, g.s, rn, sn), dkq_mid_x(g.r, g.s, n),
                           dkq_mid_e(g.r, g.s, n), dkq_mid_x(g.r, g.s, np), dkq_mid_e(g.r, g.s, np), g.Ji, B);
#pragma unroll
            for (int c = 0; c < 3; c++) fp[n][c] += wdet * (B[0][c] + B[1][c]);
        }
    }
    // f_p = -M_T sum w (-B)^T (1,1,0): the curvature operator is minus the DKQ operator
#pragma unroll
    for (int n = 0; n < 4; n++) put_node(dst + 6 * n, f.ex, f.ey, f.ez, nt * fm[n][0], nt * fm[n][1], mt * fp[n][0], mt * fp[n][1], mt * fp[n][2]);
}

} // namespace

template <bool kHasQuads, bool kSections>
__global__ __launch_bounds__(kThThreads) void k_element_thermal(DeviceMatrix m, const int32_t *__restrict__ slice_elem_local,
                                                                const int32_t *__restrict__ slice_elem_section, ThermalView tv,
                                                                const double *__restrict__ base, double *__restrict__ out)
{
    constexpr int kStride = th_stride<kHasQuads>();
    __shared__ double s_vec[kThTile * kStride];
    __shared__ uint32_t s_node[kThTile]; // byte j: the row of the slice that node j of the entry is (0xFF: none of them)
    __shared__ unsigned long long s_rows[kThTile / 64][kSliceNodes]; // per wave of entries and row: the entries that contain the row
    __shared__ double s_sum[kSliceRows];
    const int tid = threadIdx.x, lane = tid & 63;
    SliceWalk w(m.n_slices);
    for (; w.valid(); w.next()) {
        const int s = w.s;
        const int e0 = m.slice_elem_ptr[s], ne = m.slice_elem_ptr[s + 1] - e0;
        const int row0 = s * kSliceNodes;
        const uint32_t my_row = (uint32_t)(tid / 6);
        const int my_v = tid % 6; // phase B: all 192 lanes
        double sum = 0.0;
        for (int t0 = 0; t0 < ne; t0 += kThTile) {
            const int nt = min(kThTile, ne - t0);
            // ---- A: the entries' per-node vectors, and which rows of the slice every entry contains.  (Whole waves walk the tile, so
            //      that every lane takes part in the ballots below; a wave whose 64 entries lie past the tile's end skips them.)
            for (int i0 = tid - lane; i0 < nt; i0 += kThThreads) {
                const int i = i0 + lane;
                uint32_t rows = 0; // bit r: node row0 + r belongs to the entry
                if (i < nt) {
                    const int4 c = m.slice_elem_nodes[e0 + t0 + i];
                    const int le = slice_elem_local[e0 + t0 + i];
                    const double2 tmp = tv.elem_temp[le]; // (Tm, Tg)
                    double2 coef = make_double2(tv.uni.nt, tv.uni.mt);
                    if (kSections) coef = *reinterpret_cast<const double2 *>(tv.sec + slice_elem_section[e0 + t0 + i]);
                    const double nT = coef.x * tmp.x, mT = coef.y * tmp.y;
                    const int nid[4] = {c.x, c.y, c.z, kHasQuads ? c.w : -1};
                    double *dst = s_vec + i * kStride;
                    if (!kHasQuads || c.w < 0) {
                        double X[9];
                        load_xyz<3>(m.xyz, nid, X);
                        tri3_thermal(X, nT, mT, dst);
                    } else {
                        double X[12];
                        load_xyz<4>(m.xyz, nid, X);
                        relative_to_first(X);
                        quad4_thermal(X, nT, mT, dst);
                    }
                    uint32_t word = 0xFFFFFFFFu;
#pragma unroll
                    for (int j = 0; j < 4; j++) entry_node(j, nid[j], row0, rows, word);
                    s_node[i] = word;
                }
                publish_rows(rows, lane, s_rows[i0 >> 6]);
            }
            __syncthreads();
            // ---- B: row sums in list order: waves of entries ascending, within one the set bits ascending
            if (tid < kSliceRows)
                for_entries_of_row(s_rows, nt, (int)my_row, [&](int i) { sum += s_vec[i * kStride + 6 * entry_node_of_row(s_node[i], my_row) + my_v]; });
            __syncthreads(); // (the next tile overwrites the vectors)
        }
        if (tid < kSliceRows) s_sum[tid] = sum;
        __syncthreads();
        if (tid < kSliceNodes) {
            const int a = row0 + tid;
            double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (a < m.n_own) {
                if (base != nullptr) load_node6(base, a, false, v);
#pragma unroll
                for (int d = 0; d < 6; d++) v[d] = base != nullptr ? v[d] + s_sum[6 * tid + d] : s_sum[6 * tid + d];
            }
            store_node6(out, a, false, v);
        }
        __syncthreads(); // (the next slice overwrites the row sums)
    }
}

void launch_element_thermal(const DeviceMatrix &m, const int32_t *slice_elem_local, const int32_t *slice_elem_section, const ThermalView &tv,
                            const double *base, double *out, hipStream_t st)
{
    if (m.n_slices == 0) return;
    const int g = slice_grid(m);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(g), dim3(kThThreads), 0, st, m, slice_elem_local, slice_elem_section, tv, base, out); };
    if (tv.sec != nullptr) { // (the instantiations with sections: contexts without never launch them)
        if (m.n_lquad > 0) launch(k_element_thermal<true, true>);
        else launch(k_element_thermal<false, true>);
    } else if (m.n_lquad > 0) {
        launch(k_element_thermal<true, false>);
    } else {
        launch(k_element_thermal<false, false>);
    }
}

} // namespace femshell
