// element_resultants.hip -- what the shell carries: per element the membrane force tensor N, the moment tensor M (global axes) and the
// von Mises stress at the two surfaces, from a displacement vector (gfx950, wave64).  DESIGN.md 8d has the definition.
//
// One lane per local element, triangles then quadrilaterals (DeviceMatrix::tri, ::quad, the order k_element_matrices indexes).  The
// lane gathers its 3 or 4 nodes' coordinates and displacements, builds the element frame and forms the element MEANS of the
// element's own strain operators directly -- no 38/66-double record, no Gram table:
//   TRI3   eps = the CST strain; kappa = Y * (1/3) sum_g B~(g) d, and with Specht's factorisation (shell_element.hpp, tri3_record)
//          B~_i(g) = Q_i(g) u_i^T + Q_k(g) v_i^T + C_k (e0 + w_i)^T - C_i e0^T the Gauss-point sum touches Q alone: sQ_n = sum_g Q_n(g),
//          three constants and three multiples of a side ratio per n.  Y is the stiffness's, kRefY21 switch included.
//   QUAD4  the det-J-weighted means over the 2 x 2 Gauss points of the bilinear membrane strain and of MINUS the DKQ operator
//          (dkq_node_block is written in the section rotations beta = -grad w; kappa here is (w,xx, w,yy, 2 w,xy)).
// Then N_loc = t Dm eps, M_loc = -Dp kappa (M = integral of sigma z dz), both rotated as R^T [[a_xx, a_xy, 0], [a_xy, a_yy, 0], 0] R,
// sigma_top/bot = N_loc / t +- 6 M_loc / t^2 and their plane-stress von Mises values: 14 doubles per element.
//
// A lane's 14 doubles lie 112 bytes from its neighbour's: stored by the lane they would split every line.  The lanes of a wave put
// them into LDS and the wave writes its 64 rows -- 7168 contiguous bytes -- as 16-byte words, lane after lane.  No atomics, no sum
// across lanes: two launches give the same bits.  A degenerate element writes zeros and reports kStatusDirect + its index.
// Rows are in the LOCAL element order; the host maps them to the caller's (api_resultants.cpp).
#include <type_traits>

#include "kernels.hpp"
#include "device_common.hpp"

namespace femshell {

constexpr int kErThreads = 256;
constexpr int kErWords = 14; // doubles per element

namespace {

// what the element math hands on: local membrane strain and curvature means and the frame
struct ElemMeans {
    double ex[3], ey[3], ez[3];
    double eps[3], kap[3];
};

// local nodal values of node n: translations (ul) and rotations (rl) in the element frame; the drilling rotation carries nothing
__device__ __forceinline__ void to_local(const ElemMeans &f, const double u6[6], double ul[3], double rl[2])
{
#pragma clang fp reassociate(on) contract(fast)
    ul[0] = f.ex[0] * u6[0] + f.ex[1] * u6[1] + f.ex[2] * u6[2];
    ul[1] = f.ey[0] * u6[0] + f.ey[1] * u6[1] + f.ey[2] * u6[2];
    ul[2] = f.ez[0] * u6[0] + f.ez[1] * u6[1] + f.ez[2] * u6[2];
    rl[0] = f.ex[0] * u6[3] + f.ex[1] * u6[4] + f.ex[2] * u6[5];
    rl[1] = f.ey[0] * u6[3] + f.ey[1] * u6[4] + f.ey[2] * u6[5];
}

__device__ __forceinline__ bool tri3_means(const double X[9], const double U[3][6], uint32_t flags, ElemMeans &o)
{
#pragma clang fp reassociate(on) contract(fast) // element math only; parity bar is 1e-12, not bitwise
    constexpr SpechtSums kS = specht_sums();
    constexpr double kC[3][3] = SPECHT_C456_INIT;
    TriFrame f;
    const bool ok = tri3_frame(X, f); // degenerate: zero scale factors, everything below is a finite zero
#pragma unroll
    for (int d = 0; d < 3; d++) {
        o.ex[d] = f.ex[d];
        o.ey[d] = f.ey[d];
        o.ez[d] = f.ez[d];
    }
    double mu[3];
    specht_mu(f, ok, mu);
    double mQ[3][3]; // (1/3) sum_g Q_n(g)
#pragma unroll
    for (int n = 0; n < 3; n++)
#pragma unroll
        for (int r = 0; r < 3; r++) mQ[n][r] = (kS.a[n][r] + mu[(n + 2) % 3] * kS.b[n][r]) * (1.0 / 3.0);
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    double c[3] = {0.0, 0.0, 0.0}; // mean curvature in area coordinates
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double ul[3], rl[2];
        to_local(o, U[i], ul, rl);
        // membrane (SA:443-468): beta_i = y of row 2 - i, gamma_i = -x of that row
        const double bi = f.ys[2 - i], gi = -f.xs[2 - i];
        e0 += bi * ul[0];
        e1 += gi * ul[1];
        e2 += gi * ul[0] + bi * ul[1];
        // plate: rows seen from node i (tri_row_ki, tri_row_ji), d_i = (w, tx, ty)
        const int k = tri_prev(i);
        const double xki = f.xs[tri_row_ki(i)], yki = f.ys[tri_row_ki(i)], xji = -f.xs[tri_row_ji(i)], yji = -f.ys[tri_row_ji(i)];
        const double w = ul[2], tx = rl[0], ty = rl[1];
        const double ud = 2.0 * w + yji * tx - xji * ty;  // u_i . d_i
        const double vd = -2.0 * w - yki * tx + xki * ty; // v_i . d_i
        const double wd = w + yki * tx - xki * ty;        // (e0 + w_i) . d_i
#pragma unroll
        for (int r = 0; r < 3; r++) c[r] += mQ[i][r] * ud + mQ[k][r] * vd + kC[k][r] * wd - kC[i][r] * w;
    }
    o.eps[0] = e0 * f.inv2a;
    o.eps[1] = e1 * f.inv2a;
    o.eps[2] = e2 * f.inv2a;
    // Y (SA:578-588) as tri3_record forms it
    const double x31 = f.xs[1], y31 = f.ys[1], x23 = f.xs[2], y23 = f.ys[2];
    const double sY = f.inv2a * f.inv2a;
    const double y21 = (flags & kRefY21) ? -2.0 * x31 * x31 : -2.0 * x31 * y31;
    o.kap[0] = sY * (y23 * y23 * c[0] + y31 * y31 * c[1] + y23 * y31 * c[2]);
    o.kap[1] = sY * (x23 * x23 * c[0] + x31 * x31 * c[1] + x31 * x23 * c[2]);
    o.kap[2] = sY * (-2.0 * x23 * y23 * c[0] + y21 * c[1] + (-x23 * y31 - x31 * y23) * c[2]);
    return ok;
}

__device__ __forceinline__ bool quad4_means(const double X[12], const double U[4][6], ElemMeans &o)
{
#pragma clang fp reassociate(on) contract(fast) // element math only; parity bar is 1e-12, not bitwise
    QuadFrame q;
    const bool ok = quad4_frame(X, q); // (of X as given: the caller translates)
#pragma unroll
    for (int d = 0; d < 3; d++) {
        o.ex[d] = q.ex[d];
        o.ey[d] = q.ey[d];
        o.ez[d] = q.ez[d];
    }
    double um[4][2], dp[4][3]; // local (u, v) and (w, tx, ty) of the nodes
#pragma unroll
    for (int n = 0; n < 4; n++) {
        double ul[3], rl[2];
        to_local(o, U[n], ul, rl);
        um[n][0] = ul[0];
        um[n][1] = ul[1];
        dp[n][0] = ul[2];
        dp[n][1] = rl[0];
        dp[n][2] = rl[1];
    }
    DkqSide sd[4];
    dkq_sides(q, ok, sd);
    double es[3] = {0.0, 0.0, 0.0}, ks[3] = {0.0, 0.0, 0.0}, dsum = 0.0;
#pragma unroll 1 // (one copy of the Gauss-point code: the register budget, as in quad4_block_add_rec)
    for (int gp = 0; gp < 4; gp++) {
        const QuadGauss g = quad4_gauss(q, gp, ok);
        double eg[3] = {0.0, 0.0, 0.0}, kg[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int n = 0; n < 4; n++) {
            double bx, by; // dN/dx, dN/dy
            bilinear_grad(n, g.r, g.s, g.Ji, bx, by);
            eg[0] += bx * um[n][0];
            eg[1] += by * um[n][1];
            eg[2] += by * um[n][0] + bx * um[n][1];
            const int np = (n + 3) & 3;
            const double rn = quad_corner_r(n), sn = quad_corner_s(n);
            double B[3][3];
            dkq_node_block(sd[n], sd[np], dkq_corner_x(g.r, g.s, rn, sn), dkq_corner_e(g.r, g.s, rn, sn), dkq_mid_x(g.r, g.s, n),
                           dkq_mid_e(g.r, g.s, n), dkq_mid_x(g.r, g.s, np), dkq_mid_e(g.r, g.s, np), g.Ji, B);
#pragma unroll
            for (int c = 0; c < 3; c++) kg[c] += B[c][0] * dp[n][0] + B[c][1] * dp[n][1] + B[c][2] * dp[n][2];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            es[c] += g.det * eg[c];
            ks[c] += g.det * kg[c];
        }
        dsum += g.det;
    }
    const double iw = (ok && dsum != 0.0) ? 1.0 / dsum : 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o.eps[c] = es[c] * iw;
        o.kap[c] = -ks[c] * iw; // the DKQ operator is in beta = -grad w
    }
    return ok;
}

// material, rotation, surface stresses: the 14 doubles of one element
__device__ __forceinline__ void finish_element(const ElemMeans &f, double tcm, double cp, double nu, double g, double t, double out[kErWords])
{
#pragma clang fp reassociate(on) contract(fast)
    const double N[3] = {tcm * (f.eps[0] + nu * f.eps[1]), tcm * (nu * f.eps[0] + f.eps[1]), tcm * g * f.eps[2]};
    const double M[3] = {-cp * (f.kap[0] + nu * f.kap[1]), -cp * (nu * f.kap[0] + f.kap[1]), -cp * g * f.kap[2]};
    // R^T [[a_xx, a_xy, 0], [a_xy, a_yy, 0], [0, 0, 0]] R, rows of R = ex, ey, ez; components xx yy zz xy yz zx
    constexpr int kP[6] = {0, 1, 2, 0, 1, 2}, kQ[6] = {0, 1, 2, 1, 2, 0};
#pragma unroll
    for (int v = 0; v < 6; v++) {
        const int p = kP[v], q = kQ[v];
        const double xx = f.ex[p] * f.ex[q], yy = f.ey[p] * f.ey[q], xy = f.ex[p] * f.ey[q] + f.ey[p] * f.ex[q];
        out[v] = N[0] * xx + N[1] * yy + N[2] * xy;
        out[6 + v] = M[0] * xx + M[1] * yy + M[2] * xy;
    }
    const double it = 1.0 / t, b = 6.0 * it * it;
    double top[3], bot[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        top[q] = N[q] * it + b * M[q];
        bot[q] = N[q] * it - b * M[q];
    }
    out[12] = sqrt(top[0] * top[0] + top[1] * top[1] - top[0] * top[1] + 3.0 * top[2] * top[2]);
    out[13] = sqrt(bot[0] * bot[0] + bot[1] * bot[1] - bot[0] * bot[1] + 3.0 * bot[2] * bot[2]);
}

// displacements of one node: u, and up (the prescribed part of a solution that lies in HBM as its homogeneous part) added entry by entry
__device__ __forceinline__ void gather_u(const double *u, const double *up, int node, double v[6])
{
    load_node6(u, node, false, v);
    if (up != nullptr) {
        double w[6];
        load_node6(up, node, false, w);
#pragma unroll
        for (int q = 0; q < 6; q++) v[q] += w[q];
    }
}

} // namespace

// out: (n_ltri + n_lquad) x 14, local element order.  u, up: (n_pad + n_ghost) x 6, up may be nullptr.  sec_t: thickness per section
// (kSections only: the table in HBM keeps products of it).  kThermal: temperatures are in force -- the element means
// lose the free thermal state before the material is applied, N_loc = t Dm (eps - eps0), M_loc = -Dp (kappa - kappa0), from the
// element's (Tm, Tg) and the expansion of its section (tv).  Without, tv is not looked at: those instantiations are the only ones
// launched when nothing is set.
template <bool kHasQuads, bool kSections, bool kThermal>
__global__ __launch_bounds__(kErThreads) void k_element_resultants(DeviceMatrix m, MatConst mc, DeviceSections ds, const double *__restrict__ sec_t,
                                                                  const double *__restrict__ u, const double *__restrict__ up, ThermalView tv,
                                                                  double *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) double s_out[kErThreads * kErWords];
    const int n = m.n_ltri + (kHasQuads ? m.n_lquad : 0);
    const int64_t e64 = (int64_t)blockIdx.x * kErThreads + threadIdx.x;
    double res[kErWords];
#pragma unroll
    for (int q = 0; q < kErWords; q++) res[q] = 0.0;
    if (e64 < n) {
        const int e = (int)e64;
        ElemMeans f;
        bool ok;
        if (!kHasQuads || e < m.n_ltri) {
            const int32_t *c = m.tri + 3 * (int64_t)e;
            const int nid[3] = {c[0], c[1], c[2]};
            double X[9], U[3][6];
            load_xyz<3>(m.xyz, nid, X);
#pragma unroll
            for (int i = 0; i < 3; i++) gather_u(u, up, nid[i], U[i]);
            ok = tri3_means(X, U, mc.flags, f);
        } else {
            const int4 c = reinterpret_cast<const int4 *>(m.quad)[e - m.n_ltri];
            const int nid[4] = {c.x, c.y, c.z, c.w};
            double X[12], U[4][6];
            load_xyz<4>(m.xyz, nid, X);
#pragma unroll
            for (int i = 0; i < 4; i++) gather_u(u, up, nid[i], U[i]);
            relative_to_first(X);
            ok = quad4_means(X, U, f);
        }
        double tcm = mc.t * mc.cm, cp = mc.cp, nu = mc.nu, g = mc.g, t = mc.t;
        if (kSections) { // the element's own material
            const int si = ds.elem_section[e];
            const SecConst sc = fetch_section(ds.table, si);
            tcm = sc.tcm;
            cp = sc.cp;
            nu = sc.nu;
            g = sc.g;
            t = sec_t[si];
        }
        if (kThermal) { // the free thermal state leaves: eps0 = alpha Tm (1,1,0), kappa0 = -(alpha Tg / t) (1,1,0)
            const double2 tmp = tv.elem_temp[e];
            double2 al = make_double2(tv.uni.alpha, tv.uni.alpha_t);
            if (kSections) al = reinterpret_cast<const double2 *>(tv.sec + ds.elem_section[e])[1];
            const double e0 = al.x * tmp.x, k0 = -al.y * tmp.y;
            f.eps[0] -= e0;
            f.eps[1] -= e0;
            f.kap[0] -= k0;
            f.kap[1] -= k0;
        }
        double val[kErWords];
        finish_element(f, tcm, cp, nu, g, t, val);
#pragma unroll
        for (int q = 0; q < kErWords; q++) res[q] = ok ? val[q] : 0.0; // (selects: a degenerate element's values may be Inf / NaN)
        if (!ok) report_status(m.status, kStatusDirect + e);
    }
    // the lane's row into LDS, then the wave's rows out as contiguous 16-byte words
    {
        double2 *row = reinterpret_cast<double2 *>(s_out + (size_t)threadIdx.x * kErWords);
#pragma unroll
        for (int q = 0; q < kErWords / 2; q++) row[q] = make_double2(res[2 * q], res[2 * q + 1]);
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * kErThreads + 64 * wave; // first element of this wave
    const int64_t left = (int64_t)n - first;
    const int words = (int)(left < 0 ? 0 : (left > 64 ? 64 : left)) * (kErWords / 2); // 16-byte words of the wave's valid rows
    const double2 *src = reinterpret_cast<const double2 *>(s_out + (size_t)wave * 64 * kErWords);
    double2 *dst = reinterpret_cast<double2 *>(out + first * kErWords);
#pragma unroll
    for (int q = 0; q < kErWords / 2; q++) {
        const int w = 64 * q + lane;
        if (w < words) dst[w] = src[w];
    }
}

void launch_element_resultants(const DeviceMatrix &m, const MatConst &mc, const DeviceSections *sections, const double *sec_t, const double *u,
                               const double *up, double *out, hipStream_t st, const ThermalView *thermal)
{
    const int64_t n = (int64_t)m.n_ltri + m.n_lquad;
    if (n == 0) return;
    const DeviceSections ds = sections ? *sections : DeviceSections();
    const ThermalView tv = thermal ? *thermal : ThermalView();
    const unsigned g = (unsigned)((n + kErThreads - 1) / kErThreads);
    // one instantiation per (quadrilaterals, sections, temperatures): a context launches only those of what it holds
    auto with = [](bool on, auto f) { on ? f(std::true_type()) : f(std::false_type()); };
    with(m.n_lquad > 0, [&](auto quads) {
        with(sections != nullptr, [&](auto sec) {
            with(thermal != nullptr, [&](auto th) {
                hipLaunchKernelGGL((k_element_resultants<decltype(quads)::value, decltype(sec)::value, decltype(th)::value>), dim3(g),
                                   dim3(kErThreads), 0, st, m, mc, ds, sec_t, u, up, tv, out);
            });
        });
    });
}

} // namespace femshell
