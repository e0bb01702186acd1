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

// sum over the three Gauss points of Specht's tables (as element_resultants.hip): sQ_n[r] = a[n][r] + mu_{(n+2)%3} b[n][r]
struct SpechtSumsT {
    double a[3][3], b[3][3];
};
constexpr SpechtSumsT specht_sums_t()
{
    constexpr double QA[3][3][3] = SPECHT_QA_INIT;
    constexpr double QB[3][3][3] = SPECHT_QB_INIT;
    SpechtSumsT s{};
    for (int n = 0; n < 3; n++)
        for (int r = 0; r < 3; r++) {
            s.a[n][r] = QA[n][0][r] + QA[n][1][r] + QA[n][2][r];
            s.b[n][r] = QB[n][0][r] + QB[n][1][r] + QB[n][2][r];
        }
    return s;
}

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
    constexpr SpechtSumsT kS = specht_sums_t();
    constexpr double kC[3][3] = SPECHT_C456_INIT;
    TriFrame f;
    const bool ok = tri3_frame(X, f); // degenerate: zero scale factors, everything below is a finite zero
    double C[3], mu[3];
#pragma unroll
    for (int e = 0; e < 3; e++) C[e] = f.xs[e] * f.xs[e] + f.ys[e] * f.ys[e];
    {
        const double c01 = C[0] * C[1], rall = ok ? 1.0 / (c01 * C[2]) : 0.0; // as tri3_record
        mu[0] = (C[0] - C[1]) * (c01 * rall);
        mu[1] = (C[2] - C[0]) * (C[0] * C[2] * rall);
        mu[2] = (C[1] - C[2]) * (C[1] * C[2] * rall);
    }
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
        constexpr int kPrev[3] = {2, 0, 1}, kRowKi[3] = {1, 0, 2}, kRowJi[3] = {0, 2, 1};
        const int k = kPrev[i];
        const double xki = f.xs[kRowKi[i]], yki = f.ys[kRowKi[i]], xji = -f.xs[kRowJi[i]], yji = -f.ys[kRowJi[i]];
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
    // frame from the mid-side points (SA:342-375), as quad4_record
    double ex[3], ey[3], ez[3], vr[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double mI = X[d] + 0.5 * (X[3 + d] - X[d]);
        const double mJ = X[3 + d] + 0.5 * (X[6 + d] - X[3 + d]);
        const double mK = X[6 + d] + 0.5 * (X[9 + d] - X[6 + d]);
        const double mL = X[9 + d] + 0.5 * (X[d] - X[9 + d]);
        ex[d] = mJ - mL;
        vr[d] = mK - mI;
    }
    const double lx2 = ex[0] * ex[0] + ex[1] * ex[1] + ex[2] * ex[2];
    bool ok = lx2 > 0.0;
    const double ilx = ok ? 1.0 / sqrt(lx2) : 0.0;
#pragma unroll
    for (int d = 0; d < 3; d++) ex[d] *= ilx;
    ez[0] = ex[1] * vr[2] - ex[2] * vr[1];
    ez[1] = ex[2] * vr[0] - ex[0] * vr[2];
    ez[2] = ex[0] * vr[1] - ex[1] * vr[0];
    const double lz2 = ez[0] * ez[0] + ez[1] * ez[1] + ez[2] * ez[2];
    ok = ok && lz2 > 0.0;
    const double ilz = ok ? 1.0 / sqrt(lz2) : 0.0;
#pragma unroll
    for (int d = 0; d < 3; d++) ez[d] *= ilz;
    ey[0] = ez[1] * ex[2] - ez[2] * ex[1];
    ey[1] = ez[2] * ex[0] - ez[0] * ex[2];
    ey[2] = ez[0] * ex[1] - ez[1] * ex[0];
    double x[4], y[4];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        x[n] = ex[0] * X[3 * n] + ex[1] * X[3 * n + 1] + ex[2] * X[3 * n + 2];
        y[n] = ey[0] * X[3 * n] + ey[1] * X[3 * n + 1] + ey[2] * X[3 * n + 2];
    }
    double a2 = 0.0;
#pragma unroll
    for (int n = 0; n < 4; n++) a2 += x[n] * y[(n + 1) % 4] - x[(n + 1) % 4] * y[n];
    ok = ok && fabs(a2) > 0.0;
    DkqSide sd[4]; // SA:613-621, side s from node s to node s + 1
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const double dx = x[s] - x[(s + 1) % 4], dy = y[s] - y[(s + 1) % 4];
        const double l2 = dx * dx + dy * dy;
        const double l = (ok && l2 > 0.0) ? 1.0 / l2 : 0.0;
        sd[s].a = -dx * l;
        sd[s].b = 0.75 * dx * dy * l;
        sd[s].c = (0.25 * dx * dx - 0.5 * dy * dy) * l;
        sd[s].d = -dy * l;
        sd[s].e = (0.25 * dy * dy - 0.5 * dx * dx) * l;
    }
    const double x12 = x[0] - x[1], y12 = y[0] - y[1], x23 = x[1] - x[2], y23 = y[1] - y[2];
    const double x34 = x[2] - x[3], y34 = y[2] - y[3], x41 = x[3] - x[0], y41 = y[3] - y[0];
    const double root = 0.57735026918962576451; // sqrt(1/3)
    double fm[4][2], fp[4][3];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        fm[n][0] = fm[n][1] = 0.0;
        fp[n][0] = fp[n][1] = fp[n][2] = 0.0;
    }
#pragma unroll 1 // (one copy of the Gauss-point code: the register budget, as in quad4_means)
    for (int gp = 0; gp < 4; gp++) {
        const double r = (gp & 2) ? -root : root, s = (gp & 1) ? -root : root; // SA:482-487 order
        const double J00 = 0.25 * ((x12 + x34) * s - x12 + x34), J01 = 0.25 * ((y12 + y34) * s - y12 + y34);
        const double J10 = 0.25 * ((x12 + x34) * r - x23 + x41), J11 = 0.25 * ((y12 + y34) * r - y23 + y41);
        const double det = J00 * J11 - J01 * J10, idet = (ok && det != 0.0) ? 1.0 / det : 0.0;
        const double wdet = ok ? det : 0.0;
        const double Ji[4] = {J11 * idet, -J01 * idet, -J10 * idet, J00 * idet};
        auto corner_x = [&](double rr, double ss) { return 0.25 * rr * (1.0 + s * ss) * (2.0 * r * rr + s * ss); };
        auto corner_e = [&](double rr, double ss) { return 0.25 * ss * (1.0 + r * rr) * (2.0 * s * ss + r * rr); };
        const double mid_x[4] = {-r * (1.0 - s), 0.5 * (1.0 - s * s), -r * (1.0 + s), -0.5 * (1.0 - s * s)};
        const double mid_e[4] = {-0.5 * (1.0 - r * r), -s * (1.0 + r), 0.5 * (1.0 - r * r), -s * (1.0 - r)};
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const double rn = (n == 1 || n == 2) ? 1.0 : -1.0, sn = (n >= 2) ? 1.0 : -1.0;
            const double dr = 0.25 * rn * (1.0 + sn * s), ds = 0.25 * sn * (1.0 + rn * r);
            fm[n][0] += wdet * (Ji[0] * dr + Ji[1] * ds); // dN/dx: Bm^T (1,1,0) = (dN/dx, dN/dy)
            fm[n][1] += wdet * (Ji[2] * dr + Ji[3] * ds);
            const int np = (n + 3) & 3;
            double B[3][3];
            dkq_node_block(sd[n], sd[np], corner_x(rn, sn), corner_e(rn, sn), mid_x[n], mid_e[n], mid_x[np], mid_e[np], Ji, B);
#pragma unroll
            for (int c = 0; c < 3; c++) fp[n][c] += wdet * (B[0][c] + B[1][c]);
        }
    }
    // f_p = -M_T sum w (-B)^T (1,1,0): the curvature operator is minus the DKQ operator
#pragma unroll
    for (int n = 0; n < 4; n++) put_node(dst + 6 * n, ex, ey, ez, nt * fm[n][0], nt * fm[n][1], mt * fp[n][0], mt * fp[n][1], mt * fp[n][2]);
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
#pragma unroll
                        for (int j = 0; j < 3; j++) {
                            const double *pt = m.xyz + 3 * (int64_t)nid[j];
                            X[3 * j + 0] = pt[0];
                            X[3 * j + 1] = pt[1];
                            X[3 * j + 2] = pt[2];
                        }
                        tri3_thermal(X, nT, mT, dst);
                    } else {
                        double X[12];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const double *pt = m.xyz + 3 * (int64_t)nid[j];
                            X[3 * j + 0] = pt[0];
                            X[3 * j + 1] = pt[1];
                            X[3 * j + 2] = pt[2];
                        }
                        // coordinates relative to the first node, each difference rounded once (as k_element_resultants)
#pragma unroll
                        for (int j = 3; j >= 0; j--)
#pragma unroll
                            for (int d = 0; d < 3; d++) X[3 * j + d] -= X[d];
                        quad4_thermal(X, nT, mT, dst);
                    }
                    uint32_t word = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t r = (uint32_t)(nid[j] - row0); // (a triangle's fourth node, -1, and ghosts fall outside)
                        const bool in = r < (uint32_t)kSliceNodes;
                        if (in) rows |= 1u << r;
                        word |= (in ? r : 0xFFu) << (8 * j);
                    }
                    s_node[i] = word;
                }
                // the wave's 64 entries are 64 consecutive entries of the list: bit b of the ballot for row r is entry i0 + b
                for (int r = 0; r < kSliceNodes; r++) {
                    const unsigned long long has = __ballot((rows >> r) & 1u);
                    if (lane == r) s_rows[i0 >> 6][r] = has;
                }
            }
            __syncthreads();
            // ---- B: row sums in list order: waves of entries ascending, within one the set bits ascending
            if (tid < kSliceRows) {
                for (int c0 = 0; c0 < nt; c0 += 64) {
                    unsigned long long has = s_rows[c0 >> 6][my_row];
                    while (has) {
                        const int i = c0 + __ffsll(has) - 1;
                        const uint32_t word = s_node[i];
                        // which node of the entry the row is (a node occurs once in an element)
                        const int j = (word & 0xFFu) == my_row ? 0 : (((word >> 8) & 0xFFu) == my_row ? 1 : (((word >> 16) & 0xFFu) == my_row ? 2 : 3));
                        sum += s_vec[i * kStride + 6 * j + my_v];
                        has &= has - 1;
                    }
                }
            }
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
