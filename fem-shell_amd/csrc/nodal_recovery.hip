// nodal_recovery.hip -- nodal stress recovery and the Zienkiewicz-Zhu error indicator (femshell_nodal_resultants; gfx950, wave64).
// DESIGN.md 8k has the definitions; include/femshell.h states them for the caller.
//
// k_nodal_recovery: the area-weighted average of the element tensors at every node, N* = sum_e A_e N_e / W, M* alike, W = sum_e A_e,
// and the fold measure 1 - |sum_e a_e| / W with the vector areas a_e.  One workgroup of 512 lanes per slice (32 node rows), over the
// slice's element list in tiles of kNrTile entries -- the pattern of k_element_loads:
//   A  one lane per list entry gathers the element's node ids and coordinates (load_xyz, the element geometry every derived kernel
//      shares), forms a_e and A_e = |a_e| as k_lumped_mass and k_element_loads do, reads the 12 tensor words of its element from
//      the rows k_element_resultants left in HBM (six 16-byte loads through the entry's local element index: a row is 112 bytes)
//      and leaves 16 words in LDS: A N (6), A M (6), A, a_e (3).  The wave's ballots say which rows contain which entry.
//   B  one lane per (row, word), 32 x 16 = 512 lanes, adds the words of the entries that contain its row IN LIST ORDER
//      (for_entries_of_row); the sum stays in the lane's register from tile to tile.  No atomics: two launches give the same bits
//      at every grid size.
// Finish: the 16 sums of every row meet in LDS, one lane per (row, output word) divides or forms the fold measure, and the
// slice's 32 rows of 14 words -- 3584 contiguous bytes -- leave as whole 16-byte stores.  Padding rows and rows without area
// write zeros.
//
// k_recovery_error: one lane per local element (the mapping of k_element_resultants).  With d_i = (N*_i - N_e, M*_i - M_e) at the
// corners and c(S, T) = cN q(S_N, T_N) + cM q(S_M, T_M), q(S, T) = (1 + nu) S:T - nu tr S tr T, cN = 1 / (E t), cM = 12 / (E t^3):
//   e2    = A_e c(sigma_e, sigma_e)
//   eta^2 = A_e sum_ij w_ij c(d_i, d_j),  w the linear (TRI3) or bilinear (QUAD4, of a parallelogram) mass matrix over A_e.
// Both mass matrices are sums of outer products of 0/1 vectors, so the double sum is a sum of SQUARES, every term >= 0:
//   TRI3   12 w = I + 1 1^T:                    sum_i c(d_i, d_i) + c(s, s),  s = sum_i d_i
//   QUAD4  36 w = (I + J) x (I + J), J = 1 1^T: sum_i c(d_i, d_i) + the four sides' c(d_i + d_j, d_i + d_j) + c(s, s)
// (same corner 4, a shared side 2, the diagonal 1).  The lane writes one 16-byte (e2, eta^2).
#include <type_traits>

#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

static_assert(kSliceNodes == 32, "k_nodal_recovery assumes 32-node slices");

constexpr int kNrWords = 16;                        // words an entry leaves in LDS, sums per row
constexpr int kNrThreads = kSliceNodes * kNrWords;  // 512: phase B, one lane per (row, word)
constexpr int kNrTile = 256;                        // entries per tile
constexpr int kNrStride = kNrWords + 1;             // doubles between entries in LDS: 34 dwords, the 32 lanes of a half-wave hit 32 bank pairs
constexpr int kNrOut = 14;                          // doubles per node row in HBM
static_assert(kNrTile % 64 == 0 && kNrTile <= kNrThreads, "phase A of k_nodal_recovery: whole waves, one round of the workgroup");

constexpr int kReThreads = 256;

namespace {

// vector area of an element from its coordinates: TRI3 (b - a) x (c - a) / 2, QUAD4 d1 x d2 / 2 with the diagonals d1 = c - a, d2 = d - b
template <bool kQuad> __device__ __forceinline__ void vector_area(const double X[], double a[3])
{
    double d1[3], d2[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        d1[d] = kQuad ? X[6 + d] - X[d] : X[3 + d] - X[d];
        d2[d] = kQuad ? X[9 + d] - X[3 + d] : X[6 + d] - X[d];
    }
    a[0] = 0.5 * (d1[1] * d2[2] - d1[2] * d2[1]);
    a[1] = 0.5 * (d1[2] * d2[0] - d1[0] * d2[2]);
    a[2] = 0.5 * (d1[0] * d2[1] - d1[1] * d2[0]);
}

// the 12 tensor words of a 14-word row (element rows and node rows alike: 112 bytes apart, 16-byte aligned)
__device__ __forceinline__ void load_tensors(const double *rows, int64_t r, double v[12])
{
    const double2 *p = reinterpret_cast<const double2 *>(rows + kNrOut * r);
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const double2 w = p[q];
        v[2 * q] = w.x;
        v[2 * q + 1] = w.y;
    }
}

// q_nu(T, T) = (1 + nu) T:T - nu (tr T)^2 of a tensor xx yy zz xy yz zx
__device__ __forceinline__ double q_form(const double *t, double nu)
{
    const double tt = t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + 2.0 * (t[3] * t[3] + t[4] * t[4] + t[5] * t[5]);
    const double tr = t[0] + t[1] + t[2];
    return (1.0 + nu) * tt - nu * tr * tr;
}
// c(d, d) of a pair (N part, M part)
__device__ __forceinline__ double c_form(const double d[12], double cn, double cm, double nu)
{
    return cn * q_form(d, nu) + cm * q_form(d + 6, nu);
}

} // namespace

template <bool kHasQuads>
__global__ __launch_bounds__(kNrThreads) void k_nodal_recovery(DeviceMatrix m, const int32_t *__restrict__ slice_elem_local,
                                                               const double *__restrict__ res, double *__restrict__ out)
{
    __shared__ double s_part[kNrTile * kNrStride];
    __shared__ unsigned long long s_rows[kNrTile / 64][kSliceNodes]; // per wave of entries and row: the entries that contain the row
    __shared__ double s_sum[kSliceNodes * kNrWords];
    __shared__ __attribute__((aligned(16))) double s_out[kSliceNodes * kNrOut];
    const int tid = threadIdx.x, lane = tid & 63;
    const int my_row = tid / kNrWords, my_w = tid % kNrWords; // phase B
    SliceWalk w(m.n_slices);
    for (; w.valid(); w.next()) {
        const int s = w.s;
        const int e0 = m.slice_elem_ptr[s], ne = m.slice_elem_ptr[s + 1] - e0;
        const int row0 = s * kSliceNodes;
        double sum = 0.0;
        for (int t0 = 0; t0 < ne; t0 += kNrTile) {
            const int nt = min(kNrTile, ne - t0);
            // ---- A: the 16 words of every entry, and which rows of the slice it contains.  (Whole waves: every lane of a wave
            //      that has an entry below nt takes part in the ballots; the waves past the tile's end skip.)
            const int i0 = tid - lane;
            if (i0 < nt) {
                const int i = tid;
                uint32_t rows = 0; // bit r: node row0 + r belongs to the entry
                if (i < nt) {
                    const int4 c = m.slice_elem_nodes[e0 + t0 + i];
                    const int le = slice_elem_local[e0 + t0 + i];
                    double T[12], a[3];
                    load_tensors(res, le, T);
                    if (!kHasQuads || c.w < 0) {
                        const int nid[3] = {c.x, c.y, c.z};
                        double X[9];
                        load_xyz<3>(m.xyz, nid, X);
                        vector_area<false>(X, a);
                    } else {
                        const int nid[4] = {c.x, c.y, c.z, c.w};
                        double X[12];
                        load_xyz<4>(m.xyz, nid, X);
                        vector_area<true>(X, a);
                    }
                    const double A = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
                    double *p = s_part + i * kNrStride;
#pragma unroll
                    for (int q = 0; q < 12; q++) p[q] = A * T[q];
                    p[12] = A;
                    p[13] = a[0];
                    p[14] = a[1];
                    p[15] = a[2];
                    const int nid4[4] = {c.x, c.y, c.z, kHasQuads ? c.w : -1};
#pragma unroll
                    for (int j = 0; j < 4; j++) entry_row_bit(nid4[j], row0, rows);
                }
                publish_rows(rows, lane, s_rows[i0 >> 6]);
            }
            __syncthreads();
            // ---- B: row sums in list order: waves of entries ascending, within one the set bits ascending
            for_entries_of_row(s_rows, nt, my_row, [&](int i) { sum += s_part[i * kNrStride + my_w]; });
            __syncthreads(); // (the next tile overwrites the words)
        }
        s_sum[tid] = sum;
        __syncthreads();
        // ---- finish: one lane per (row, output word)
        if (my_w < kNrOut) {
            const double *r = s_sum + my_row * kNrWords;
            const double W = r[12];
            double v = 0.0;
            if (row0 + my_row < m.n_own && W > 0.0) {
                if (my_w < 12) v = r[my_w] / W;
                else if (my_w == 12) v = W;
                else v = 1.0 - sqrt(r[13] * r[13] + r[14] * r[14] + r[15] * r[15]) / W;
            }
            s_out[my_row * kNrOut + my_w] = v;
        }
        __syncthreads();
        if (tid < kSliceNodes * kNrOut / 2) // 224 16-byte words: the slice's 32 rows are contiguous in HBM
            reinterpret_cast<double2 *>(out + (int64_t)row0 * kNrOut)[tid] = reinterpret_cast<const double2 *>(s_out)[tid];
        // (the next slice writes s_sum and s_out only behind the barriers of its tiles -- or, with an empty list, behind the one
        //  below)
        __syncthreads();
    }
}

void launch_nodal_recovery(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *res, double *out, hipStream_t st)
{
    if (m.n_slices == 0) return;
    const int g = slice_grid(m);
    if (m.n_lquad > 0) hipLaunchKernelGGL(k_nodal_recovery<true>, dim3(g), dim3(kNrThreads), 0, st, m, slice_elem_local, res, out);
    else hipLaunchKernelGGL(k_nodal_recovery<false>, dim3(g), dim3(kNrThreads), 0, st, m, slice_elem_local, res, out);
}

// res: the rows of k_element_resultants (LOCAL element order); nodes: the rows of k_nodal_recovery; out: 2 doubles per local element.
// mat = (1 / (E t), 12 / (E t^3), nu) of the uniform material; kSections: sec_mat holds such a triple (and a zero) per section.
template <bool kHasQuads, bool kSections>
__global__ __launch_bounds__(kReThreads) void k_recovery_error(DeviceMatrix m, RecoveryMat mat, const RecoveryMat *__restrict__ sec_mat,
                                                               const int32_t *__restrict__ elem_section, const double *__restrict__ res,
                                                               const double *__restrict__ nodes, double *__restrict__ out)
{
    const int n = m.n_ltri + (kHasQuads ? m.n_lquad : 0);
    const int64_t e64 = (int64_t)blockIdx.x * kReThreads + threadIdx.x;
    if (e64 >= n) return;
    const int e = (int)e64;
    double cn = mat.cn, cm = mat.cm, nu = mat.nu;
    if (kSections) {
        const double2 *row = reinterpret_cast<const double2 *>(sec_mat + elem_section[e]);
        const double2 r0 = row[0], r1 = row[1];
        cn = r0.x;
        cm = r0.y;
        nu = r1.x;
    }
    double T[12], a[3], eta = 0.0;
    load_tensors(res, e, T);
    if (!kHasQuads || e < m.n_ltri) {
        const int32_t *c = m.tri + 3 * (int64_t)e;
        const int nid[3] = {c[0], c[1], c[2]};
        double X[9];
        load_xyz<3>(m.xyz, nid, X);
        vector_area<false>(X, a);
        double sd[12];
#pragma unroll
        for (int q = 0; q < 12; q++) sd[q] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double d[12];
            load_tensors(nodes, nid[i], d);
#pragma unroll
            for (int q = 0; q < 12; q++) {
                d[q] -= T[q];
                sd[q] += d[q];
            }
            eta += c_form(d, cn, cm, nu);
        }
        eta = (eta + c_form(sd, cn, cm, nu)) * (1.0 / 12.0);
    } else {
        const int4 c = reinterpret_cast<const int4 *>(m.quad)[e - m.n_ltri];
        const int nid[4] = {c.x, c.y, c.z, c.w};
        double X[12];
        load_xyz<4>(m.xyz, nid, X);
        vector_area<true>(X, a);
        double d[4][12];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            load_tensors(nodes, nid[i], d[i]);
#pragma unroll
            for (int q = 0; q < 12; q++) d[i][q] -= T[q];
            eta += c_form(d[i], cn, cm, nu);
        }
        double s01[12], s23[12], sd[12];
#pragma unroll
        for (int q = 0; q < 12; q++) {
            s01[q] = d[0][q] + d[1][q];
            s23[q] = d[2][q] + d[3][q];
            sd[q] = s01[q] + s23[q];
        }
        eta += c_form(s01, cn, cm, nu) + c_form(s23, cn, cm, nu) + c_form(sd, cn, cm, nu);
#pragma unroll
        for (int q = 0; q < 12; q++) {
            s01[q] = d[1][q] + d[2][q];
            s23[q] = d[3][q] + d[0][q];
        }
        eta = (eta + c_form(s01, cn, cm, nu) + c_form(s23, cn, cm, nu)) * (1.0 / 36.0);
    }
    const double A = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    reinterpret_cast<double2 *>(out)[e] = make_double2(A * c_form(T, cn, cm, nu), A * eta);
}

void launch_recovery_error(const DeviceMatrix &m, const RecoveryMat &mat, const RecoveryMat *sec_mat, const int32_t *elem_section,
                           const double *res, const double *nodes, double *out, hipStream_t st)
{
    const int64_t n = (int64_t)m.n_ltri + m.n_lquad;
    if (n == 0) return;
    const unsigned g = (unsigned)((n + kReThreads - 1) / kReThreads);
    auto with = [](bool on, auto f) { on ? f(std::true_type()) : f(std::false_type()); };
    with(m.n_lquad > 0, [&](auto quads) {
        with(sec_mat != nullptr, [&](auto sec) {
            hipLaunchKernelGGL((k_recovery_error<decltype(quads)::value, decltype(sec)::value>), dim3(g), dim3(kReThreads), 0, st, m, mat, sec_mat,
                               elem_section, res, nodes, out);
        });
    });
}

} // namespace femshell
