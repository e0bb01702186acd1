// envelope.hip -- load combinations: the stress envelope of every element over factored sums of load cases
// (femshell_combination_envelope; gfx950, wave64, FP64).  DESIGN.md 8n has the definition; include/femshell.h states it for the caller.
//
// N_loc and M_loc of an element are affine in a case's own data, so a combination's row is the factored sum of the cases' rows and
// only the last step -- von Mises, principal values -- is not linear.  Two kernels:
//
// k_case_resultants (stage 1): one lane per local element, triangles then quadrilaterals (the mapping of k_element_resultants).  The
//   lane gathers its nodes' coordinates ONCE, builds the frame and the element's mean strain operators once:
//     TRI3   the frame, the side differences and (1/3) sum_g Q_n(g) of Specht's factorisation (specht_mu, specht_sums) -- 25 doubles;
//     QUAD4  the frame and, from one walk over the 2 x 2 Gauss points (quad4_gauss, dkq_sides, dkq_node_block), the det-J-weighted
//            mean gradients of the bilinear functions (8) and the mean DKQ operator (36), divided by the sum of the weights.
//   Then it applies them to the case vectors, kB columns at a time: the loads of a block are issued together, the arithmetic of a
//   column is one function with explicit fused multiply-adds and no contraction or reassociation left to the compiler, so a
//   column's six words do not depend on its position in the block, on the block, or on the other columns.  The words go into a
//   table in HBM laid out as planes [case][word][element]: a wave's store of one word is 512 contiguous bytes.
// k_envelope (stage 2): one lane per local element.  For kC combinations at a time it sums the table rows over the cases in index
//   order (one fused multiply-add per word, case and combination, from +0), the factors read with a wave-uniform index (scalar
//   loads); then q0..q5 of each combination and the six running extremes with strict comparisons, so the lowest index governs.
//   The table is left to the caches: it is read once per kC combinations (DESIGN.md 8n has the byte model).  A lane's six doubles
//   and six indices go through LDS and leave as the wave's contiguous 16-byte words.
// No atomics, no sums across lanes: two calls give the same bits.  A degenerate element writes zero rows in stage 1 and reports
// kStatusDirect + its index.  Rows are in the LOCAL element order; the host maps them to the caller's (api_envelope.cpp).
#include <type_traits>

#include "kernels.hpp"
#include "device_common.hpp"

namespace femshell {

constexpr int kEnvThreads = 256;
constexpr int kEnvWords = 6;    // table words per case and element: Nxx Nyy Nxy Mxx Myy Mxy in the element frame
constexpr int kEnvColsTri = 4;  // kB: columns per pass of a TRI3 lane
constexpr int kEnvColsQuad = 2; //     of a QUAD4 lane (the mean operator holds 44 doubles)
static_assert(kEnvCombosPerPass >= 1 && kEnvCombosPerPass <= 8, "k_envelope keeps 6 sums per combination of a pass in registers");

namespace {

// ---- arithmetic whose bits do not depend on the code around it: explicit fused multiply-adds, nothing contracted or reassociated
__device__ __forceinline__ double dot3(const double a[3], double x, double y, double z)
{
#pragma clang fp contract(off)
    return __builtin_fma(a[2], z, __builtin_fma(a[1], y, a[0] * x));
}

// the material of one element as stage 1 applies it
struct EnvMat {
    double tcm, cp, nu, g;
    double e0, k0; // the free thermal state: eps0 = e0 (1, 1, 0), kappa0 = k0 (1, 1, 0); zero without temperatures
};

// eps, kap -> the six table words of a column; tau: the multiple of the free thermal state the case was loaded with
template <bool kThermal> __device__ __forceinline__ void finish_column(const EnvMat &m, double tau, double eps[3], double kap[3], double w[kEnvWords])
{
#pragma clang fp contract(off)
    if (kThermal) {
        eps[0] = __builtin_fma(-tau, m.e0, eps[0]);
        eps[1] = __builtin_fma(-tau, m.e0, eps[1]);
        kap[0] = __builtin_fma(-tau, m.k0, kap[0]);
        kap[1] = __builtin_fma(-tau, m.k0, kap[1]);
    }
    w[0] = m.tcm * __builtin_fma(m.nu, eps[1], eps[0]);
    w[1] = m.tcm * __builtin_fma(m.nu, eps[0], eps[1]);
    w[2] = (m.tcm * m.g) * eps[2];
    w[3] = -m.cp * __builtin_fma(m.nu, kap[1], kap[0]);
    w[4] = -m.cp * __builtin_fma(m.nu, kap[0], kap[1]);
    w[5] = (-m.cp * m.g) * kap[2];
}

// ---- TRI3: what of the element the columns need
struct TriOp {
    double ex[3], ey[3], ez[3];
    double xs[3], ys[3];
    double inv2a;
    double mQ[3][3]; // (1/3) sum_g Q_n(g)
    double Y[3][3];  // curvature from area coordinates, 1 / (4 A^2) included
};

__device__ __forceinline__ bool tri_op(const double X[9], uint32_t flags, TriOp &o)
{
#pragma clang fp reassociate(on) contract(fast) // element geometry, once per element: the bar is 1e-12, as in tri3_means
    constexpr SpechtSums kS = specht_sums();
    TriFrame f;
    const bool ok = tri3_frame(X, f);
    double mu[3];
    specht_mu(f, ok, mu);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        o.ex[d] = f.ex[d];
        o.ey[d] = f.ey[d];
        o.ez[d] = f.ez[d];
        o.xs[d] = f.xs[d];
        o.ys[d] = f.ys[d];
    }
    o.inv2a = f.inv2a;
#pragma unroll
    for (int n = 0; n < 3; n++)
#pragma unroll
        for (int r = 0; r < 3; r++) o.mQ[n][r] = (kS.a[n][r] + mu[(n + 2) % 3] * kS.b[n][r]) * (1.0 / 3.0);
    // Y (SA:578-588) as tri3_record forms it
    const double x31 = f.xs[1], y31 = f.ys[1], x23 = f.xs[2], y23 = f.ys[2];
    const double sY = f.inv2a * f.inv2a;
    const double y21 = (flags & kRefY21) ? -2.0 * x31 * x31 : -2.0 * x31 * y31;
    o.Y[0][0] = sY * (y23 * y23);
    o.Y[0][1] = sY * (y31 * y31);
    o.Y[0][2] = sY * (y23 * y31);
    o.Y[1][0] = sY * (x23 * x23);
    o.Y[1][1] = sY * (x31 * x31);
    o.Y[1][2] = sY * (x31 * x23);
    o.Y[2][0] = sY * (-2.0 * x23 * y23);
    o.Y[2][1] = sY * y21;
    o.Y[2][2] = sY * (-x23 * y31 - x31 * y23);
    return ok;
}

// one column of a triangle: U = the global nodal values of its three nodes
__device__ __forceinline__ void tri_column(const TriOp &o, const double U[3][6], double eps[3], double kap[3])
{
#pragma clang fp contract(off)
    constexpr double kC[3][3] = SPECHT_C456_INIT;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    double c[3] = {0.0, 0.0, 0.0}; // mean curvature in area coordinates
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double ux = dot3(o.ex, U[i][0], U[i][1], U[i][2]), uy = dot3(o.ey, U[i][0], U[i][1], U[i][2]);
        const double w = dot3(o.ez, U[i][0], U[i][1], U[i][2]);
        const double tx = dot3(o.ex, U[i][3], U[i][4], U[i][5]), ty = dot3(o.ey, U[i][3], U[i][4], U[i][5]);
        // membrane (SA:443-468): beta_i = y of row 2 - i, gamma_i = -x of that row
        const double bi = o.ys[2 - i], gi = -o.xs[2 - i];
        e0 = __builtin_fma(bi, ux, e0);
        e1 = __builtin_fma(gi, uy, e1);
        e2 = __builtin_fma(bi, uy, __builtin_fma(gi, ux, e2));
        // plate: rows seen from node i (tri_row_ki, tri_row_ji), d_i = (w, tx, ty)
        const int k = tri_prev(i);
        const double xki = o.xs[tri_row_ki(i)], yki = o.ys[tri_row_ki(i)], xji = -o.xs[tri_row_ji(i)], yji = -o.ys[tri_row_ji(i)];
        const double ud = __builtin_fma(-xji, ty, __builtin_fma(yji, tx, 2.0 * w));  // u_i . d_i
        const double vd = __builtin_fma(xki, ty, __builtin_fma(-yki, tx, -2.0 * w)); // v_i . d_i
        const double wd = __builtin_fma(-xki, ty, __builtin_fma(yki, tx, w));        // (e0 + w_i) . d_i
#pragma unroll
        for (int r = 0; r < 3; r++)
            c[r] = __builtin_fma(-kC[i][r], w, __builtin_fma(kC[k][r], wd, __builtin_fma(o.mQ[k][r], vd, __builtin_fma(o.mQ[i][r], ud, c[r]))));
    }
    eps[0] = e0 * o.inv2a;
    eps[1] = e1 * o.inv2a;
    eps[2] = e2 * o.inv2a;
#pragma unroll
    for (int r = 0; r < 3; r++) kap[r] = dot3(o.Y[r], c[0], c[1], c[2]);
}

// ---- QUAD4: the frame and the mean operators
struct QuadOp {
    double ex[3], ey[3], ez[3];
    double gx[4], gy[4];  // det-J-weighted means of dN/dx, dN/dy
    double Bk[3][4][3];   // the mean curvature operator (w,xx, w,yy, 2 w,xy) of node n's (w, tx, ty): MINUS the mean DKQ operator
};

__device__ __forceinline__ bool quad_op(const double X[12], QuadOp &o)
{
#pragma clang fp reassociate(on) contract(fast) // element geometry, once per element: the bar is 1e-12, as in quad4_means
    QuadFrame q;
    const bool ok = quad4_frame(X, q); // (of X as given: the caller translates)
#pragma unroll
    for (int d = 0; d < 3; d++) {
        o.ex[d] = q.ex[d];
        o.ey[d] = q.ey[d];
        o.ez[d] = q.ez[d];
    }
    DkqSide sd[4];
    dkq_sides(q, ok, sd);
    double dsum = 0.0;
#pragma unroll
    for (int n = 0; n < 4; n++) {
        o.gx[n] = 0.0;
        o.gy[n] = 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) o.Bk[r][n][c] = 0.0;
    }
#pragma unroll 1 // (one copy of the Gauss-point code, as in quad4_means)
    for (int gp = 0; gp < 4; gp++) {
        const QuadGauss g = quad4_gauss(q, gp, ok);
#pragma unroll
        for (int n = 0; n < 4; n++) {
            double bx, by;
            bilinear_grad(n, g.r, g.s, g.Ji, bx, by);
            o.gx[n] += g.det * bx;
            o.gy[n] += g.det * by;
            const int np = (n + 3) & 3;
            const double rn = quad_corner_r(n), sn = quad_corner_s(n);
            double B[3][3];
            dkq_node_block(sd[n], sd[np], dkq_corner_x(g.r, g.s, rn, sn), dkq_corner_e(g.r, g.s, rn, sn), dkq_mid_x(g.r, g.s, n),
                           dkq_mid_e(g.r, g.s, n), dkq_mid_x(g.r, g.s, np), dkq_mid_e(g.r, g.s, np), g.Ji, B);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) o.Bk[r][n][c] += g.det * B[r][c];
        }
        dsum += g.det;
    }
    const double iw = (ok && dsum != 0.0) ? 1.0 / dsum : 0.0;
#pragma unroll
    for (int n = 0; n < 4; n++) {
        o.gx[n] *= iw;
        o.gy[n] *= iw;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) o.Bk[r][n][c] *= -iw; // the DKQ operator is in beta = -grad w
    }
    return ok;
}

__device__ __forceinline__ void quad_column(const QuadOp &o, const double U[4][6], double eps[3], double kap[3])
{
#pragma clang fp contract(off)
    double e[3] = {0.0, 0.0, 0.0}, k[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const double ux = dot3(o.ex, U[n][0], U[n][1], U[n][2]), uy = dot3(o.ey, U[n][0], U[n][1], U[n][2]);
        const double w = dot3(o.ez, U[n][0], U[n][1], U[n][2]);
        const double tx = dot3(o.ex, U[n][3], U[n][4], U[n][5]), ty = dot3(o.ey, U[n][3], U[n][4], U[n][5]);
        e[0] = __builtin_fma(o.gx[n], ux, e[0]);
        e[1] = __builtin_fma(o.gy[n], uy, e[1]);
        e[2] = __builtin_fma(o.gx[n], uy, __builtin_fma(o.gy[n], ux, e[2]));
#pragma unroll
        for (int r = 0; r < 3; r++) k[r] = __builtin_fma(o.Bk[r][n][2], ty, __builtin_fma(o.Bk[r][n][1], tx, __builtin_fma(o.Bk[r][n][0], w, k[r])));
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        eps[r] = e[r];
        kap[r] = k[r];
    }
}

// the columns of one element, kB at a time: the loads of a block first, then column after column.  The last block reads its
// missing columns from the last case again and stores nothing for them: one code path, whatever n_cases is.
template <int kNodes, int kB, bool kThermal, class Op, class Apply>
__device__ __forceinline__ void element_columns(const Op &op, const EnvMat &mat, bool ok, const int nid[], const double *__restrict__ u, int64_t ld,
                                                int n_cases, const double *__restrict__ case_tau, double *__restrict__ table, int64_t ne,
                                                int e, Apply apply)
{
#pragma unroll 1
    for (int j0 = 0; j0 < n_cases; j0 += kB) {
        double U[kB][kNodes][6];
#pragma unroll
        for (int b = 0; b < kB; b++) {
            const int j = min(j0 + b, n_cases - 1);
#pragma unroll
            for (int i = 0; i < kNodes; i++) load_node6(u + (int64_t)j * ld, nid[i], false, U[b][i]);
        }
#pragma unroll
        for (int b = 0; b < kB; b++) {
            const int j = j0 + b;
            if (j < n_cases) { // (wave-uniform)
                double eps[3], kap[3], w[kEnvWords];
                apply(op, U[b], eps, kap);
                finish_column<kThermal>(mat, kThermal ? case_tau[j] : 0.0, eps, kap, w);
                double *dst = table + (int64_t)j * kEnvWords * ne + e;
#pragma unroll
                for (int q = 0; q < kEnvWords; q++) dst[(int64_t)q * ne] = ok ? w[q] : 0.0; // (selects: a degenerate element's values may be Inf / NaN)
            }
        }
    }
}

} // namespace

// table: n_cases x 6 x (n_ltri + n_lquad), planes [case][word][element], LOCAL element order.  u: n_cases columns of
// (n_pad + n_ghost) x 6, column j at u + j * ld.  sec_t is not needed here: the table holds forces and moments.  kThermal:
// temperatures are in force and at least one case carries them -- case_tau[j] times the free thermal state leaves the means of
// case j before the material is applied; without, case_tau and tv are not looked at.
template <bool kHasQuads, bool kSections, bool kThermal>
__global__ __launch_bounds__(kEnvThreads) void k_case_resultants(DeviceMatrix m, MatConst mc, DeviceSections ds, ThermalView tv,
                                                                const double *__restrict__ u, int64_t ld, int n_cases,
                                                                const double *__restrict__ case_tau, double *__restrict__ table)
{
    const int n = m.n_ltri + (kHasQuads ? m.n_lquad : 0);
    const int64_t e64 = (int64_t)blockIdx.x * kEnvThreads + threadIdx.x;
    if (e64 >= n) return;
    const int e = (int)e64;
    EnvMat mat;
    mat.tcm = mc.t * mc.cm;
    mat.cp = mc.cp;
    mat.nu = mc.nu;
    mat.g = mc.g;
    mat.e0 = 0.0;
    mat.k0 = 0.0;
    if (kSections) { // the element's own material
        const SecConst sc = fetch_section(ds.table, ds.elem_section[e]);
        mat.tcm = sc.tcm;
        mat.cp = sc.cp;
        mat.nu = sc.nu;
        mat.g = sc.g;
    }
    if (kThermal) { // the free thermal state: eps0 = alpha Tm (1,1,0), kappa0 = -(alpha Tg / t) (1,1,0)
        const double2 tmp = tv.elem_temp[e];
        double2 al = make_double2(tv.uni.alpha, tv.uni.alpha_t);
        if (kSections) al = reinterpret_cast<const double2 *>(tv.sec + ds.elem_section[e])[1];
        mat.e0 = al.x * tmp.x;
        mat.k0 = -al.y * tmp.y;
    }
    if (!kHasQuads || e < m.n_ltri) {
        const int32_t *c = m.tri + 3 * (int64_t)e;
        const int nid[3] = {c[0], c[1], c[2]};
        double X[9];
        load_xyz<3>(m.xyz, nid, X);
        TriOp op;
        const bool ok = tri_op(X, mc.flags, op);
        element_columns<3, kEnvColsTri, kThermal>(op, mat, ok, nid, u, ld, n_cases, case_tau, table, (int64_t)n, e,
                                                  [](const TriOp &o, const double U[3][6], double eps[3], double kap[3]) { tri_column(o, U, eps, kap); });
        if (!ok) report_status(m.status, kStatusDirect + e);
    } else {
        const int4 c = reinterpret_cast<const int4 *>(m.quad)[e - m.n_ltri];
        const int nid[4] = {c.x, c.y, c.z, c.w};
        double X[12];
        load_xyz<4>(m.xyz, nid, X);
        relative_to_first(X);
        QuadOp op;
        const bool ok = quad_op(X, op);
        element_columns<4, kEnvColsQuad, kThermal>(op, mat, ok, nid, u, ld, n_cases, case_tau, table, (int64_t)n, e,
                                                   [](const QuadOp &o, const double U[4][6], double eps[3], double kap[3]) { quad_column(o, U, eps, kap); });
        if (!ok) report_status(m.status, kStatusDirect + e);
    }
}

void launch_case_resultants(const DeviceMatrix &m, const MatConst &mc, const DeviceSections *sections, const ThermalView *thermal, const double *u,
                            int64_t ld, int n_cases, const double *case_tau, double *table, hipStream_t st)
{
    const int64_t n = (int64_t)m.n_ltri + m.n_lquad;
    if (n == 0 || n_cases <= 0) return;
    const DeviceSections ds = sections ? *sections : DeviceSections();
    const ThermalView tv = thermal ? *thermal : ThermalView();
    const unsigned g = (unsigned)((n + kEnvThreads - 1) / kEnvThreads);
    // one instantiation per (quadrilaterals, sections, temperatures): a context launches only those of what it holds
    auto with = [](bool on, auto f) { on ? f(std::true_type()) : f(std::false_type()); };
    with(m.n_lquad > 0, [&](auto quads) {
        with(sections != nullptr, [&](auto sec) {
            with(thermal != nullptr, [&](auto th) {
                hipLaunchKernelGGL((k_case_resultants<decltype(quads)::value, decltype(sec)::value, decltype(th)::value>), dim3(g),
                                   dim3(kEnvThreads), 0, st, m, mc, ds, tv, u, ld, n_cases, case_tau, table);
            });
        });
    });
}

namespace {

// q0..q5 of a combined row (the definition of DESIGN.md 8n): von Mises at the two surfaces, principal membrane forces, principal moments
__device__ __forceinline__ void envelope_values(const double T[kEnvWords], double it, double b, double q[6])
{
#pragma clang fp contract(off)
    double top[3], bot[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double n = T[r] * it, mm = b * T[3 + r];
        top[r] = n + mm;
        bot[r] = n - mm;
    }
    q[0] = sqrt(__builtin_fma(3.0 * top[2], top[2], __builtin_fma(-top[0], top[1], __builtin_fma(top[1], top[1], top[0] * top[0]))));
    q[1] = sqrt(__builtin_fma(3.0 * bot[2], bot[2], __builtin_fma(-bot[0], bot[1], __builtin_fma(bot[1], bot[1], bot[0] * bot[0]))));
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const double xx = T[3 * p], yy = T[3 * p + 1], xy = T[3 * p + 2];
        const double c = 0.5 * (xx + yy), h = 0.5 * (xx - yy);
        const double r = sqrt(__builtin_fma(h, h, xy * xy));
        q[2 + 2 * p] = c + r;
        q[3 + 2 * p] = c - r;
    }
}

} // namespace

// table as k_case_resultants left it; factors: n_combos x n_cases, row-major.  env: (n_ltri + n_lquad) x 6 doubles, gov: the same
// count of int32 (padded to whole 16-byte words: the last wave stores its final word whole), LOCAL element order.
template <bool kSections>
__global__ __launch_bounds__(kEnvThreads) void k_envelope(int n, MatConst mc, const int32_t *__restrict__ elem_section,
                                                         const double *__restrict__ sec_t, const double *__restrict__ table, int n_cases,
                                                         const double *__restrict__ factors, int n_combos, double *__restrict__ env,
                                                         int32_t *__restrict__ gov)
{
    constexpr int kC = kEnvCombosPerPass;
    __shared__ __attribute__((aligned(16))) double s_env[kEnvThreads * 6];
    __shared__ __attribute__((aligned(16))) int32_t s_gov[kEnvThreads * 6];
    const int64_t e64 = (int64_t)blockIdx.x * kEnvThreads + threadIdx.x;
    double best[6];
    int32_t who[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        best[k] = 0.0;
        who[k] = 0;
    }
    if (e64 < n) {
        const int e = (int)e64;
        double t = mc.t;
        if (kSections) t = sec_t[elem_section[e]];
        const double it = 1.0 / t, b = 6.0 * it * it;
        const double *row = table + e;
#pragma unroll 1
        for (int c0 = 0; c0 < n_combos; c0 += kC) {
            double T[kC][kEnvWords];
#pragma unroll
            for (int i = 0; i < kC; i++)
#pragma unroll
                for (int q = 0; q < kEnvWords; q++) T[i][q] = 0.0;
#pragma unroll 1
            for (int j = 0; j < n_cases; j++) {
                double w[kEnvWords];
#pragma unroll
                for (int q = 0; q < kEnvWords; q++) w[q] = row[((int64_t)j * kEnvWords + q) * n];
#pragma unroll
                for (int i = 0; i < kC; i++) { // (the last pass reads its missing combinations from the last one again and drops them below)
                    const double f = factors[(int64_t)min(c0 + i, n_combos - 1) * n_cases + j];
#pragma unroll
                    for (int q = 0; q < kEnvWords; q++) T[i][q] = __builtin_fma(f, w[q], T[i][q]);
                }
            }
#pragma unroll
            for (int i = 0; i < kC; i++) {
                const int c = c0 + i;
                if (c < n_combos) { // (wave-uniform)
                    double q[6];
                    envelope_values(T[i], it, b, q);
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        const bool is_min = (k == 3 || k == 5);
                        const bool take = c == 0 || (is_min ? q[k] < best[k] : q[k] > best[k]);
                        best[k] = take ? q[k] : best[k];
                        who[k] = take ? c : who[k];
                    }
                }
            }
        }
    }
    // the lane's rows into LDS, then the wave's rows out as contiguous 16-byte words
    {
        double2 *r = reinterpret_cast<double2 *>(s_env + (size_t)threadIdx.x * 6);
#pragma unroll
        for (int k = 0; k < 3; k++) r[k] = make_double2(best[2 * k], best[2 * k + 1]);
        int2 *g = reinterpret_cast<int2 *>(s_gov + (size_t)threadIdx.x * 6);
#pragma unroll
        for (int k = 0; k < 3; k++) g[k] = make_int2(who[2 * k], who[2 * k + 1]);
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * kEnvThreads + 64 * wave; // first element of this wave
    const int64_t left = (int64_t)n - first;
    const int rows = (int)(left < 0 ? 0 : (left > 64 ? 64 : left));
    {
        const int words = rows * 3; // 48 bytes per row
        const double2 *src = reinterpret_cast<const double2 *>(s_env + (size_t)wave * 64 * 6);
        double2 *dst = reinterpret_cast<double2 *>(env + first * 6);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int w = 64 * k + lane;
            if (w < words) dst[w] = src[w];
        }
    }
    {
        const int words = (rows * 3 + 1) / 2; // 24 bytes per row; an odd count of rows ends in half a word of the next lane's zeros
        const int4 *src = reinterpret_cast<const int4 *>(s_gov + (size_t)wave * 64 * 6);
        int4 *dst = reinterpret_cast<int4 *>(gov + first * 6);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int w = 64 * k + lane;
            if (w < words) dst[w] = src[w];
        }
    }
}

void launch_envelope(const DeviceMatrix &m, const MatConst &mc, const int32_t *elem_section, const double *sec_t, const double *table, int n_cases,
                     const double *factors, int n_combos, double *env, int32_t *gov, hipStream_t st)
{
    const int64_t n = (int64_t)m.n_ltri + m.n_lquad;
    if (n == 0 || n_cases <= 0 || n_combos <= 0) return;
    const unsigned g = (unsigned)((n + kEnvThreads - 1) / kEnvThreads);
    if (sec_t != nullptr)
        hipLaunchKernelGGL(k_envelope<true>, dim3(g), dim3(kEnvThreads), 0, st, (int)n, mc, elem_section, sec_t, table, n_cases, factors, n_combos, env, gov);
    else
        hipLaunchKernelGGL(k_envelope<false>, dim3(g), dim3(kEnvThreads), 0, st, (int)n, mc, elem_section, sec_t, table, n_cases, factors, n_combos, env, gov);
}

} // namespace femshell
