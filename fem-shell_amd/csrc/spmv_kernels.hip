// spmv_kernels.hip -- the sparse products of libfemshell on the sliced block ELL layout (plan.hpp): k_spmv (full storage, one
// lane per scalar row, optional epilogue), k_spmv_node (full storage, narrow rows, one lane per node), k_spmv_sym + k_sym_gather_node
// (symmetric storage, two phases), the double-double residual, and the three launchers kernels.hpp exports for them.
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

#include <type_traits>

#include <cstdlib>

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "kernels assume 32-node slices");

// =====================================================================================
// SpMV y = K x on the sliced block ELL layout, one lane per scalar row: lane t of a slice holds block row
// i = t / 32 of node n = t % 32, so that the words of K it needs are the t-th of every 192-word group and
// consecutive lanes read consecutive 16-byte words (1 KiB per wave instruction).  The x entries of the slice's
// block columns (48 bytes per slot and node) are staged through LDS once per slice -- the six lanes of a node sit
// in three different waves in this mapping -- and read back as broadcasts.  Optionally fuses the partial sums of
// x.y needed by CG (p.Ap).
// =====================================================================================
// kChunk block slots are handled together: all their K loads are issued back to back; the loads of the first
// chunk are issued before the x staging (spmv_load), so that their latency overlaps it.
// (kF32: the words come from a single-precision copy of the values in the same layout, v32 -- smoothing products of the
//  multigrid cycle only; the arithmetic stays FP64.  The chunk keeps the words AS LOADED and converts them where they are used:
//  until round 5 spmv_load converted to double on the spot, so the wave waited for its loads before it began to stage x -- the
//  float variant of the product took 16.3 us on the 584-slice level of the 4M hierarchy where the FP64 one took 11.4.)
template <int kChunk, bool kF32 = false> struct SpmvChunk {
    typedef float v2f_ __attribute__((ext_vector_type(2)));
    typedef double v2d_ __attribute__((ext_vector_type(2)));
    typedef typename std::conditional<kF32, v2f_, v2d_>::type Word;
    Word a[kChunk][3];
};
template <int kChunk, bool kF32 = false>
__device__ __forceinline__ void spmv_load(SpmvChunk<kChunk, kF32> &c, const double2 *__restrict__ v, int k0, int W,
                                          const float2 *__restrict__ v32 = nullptr)
{
    typedef typename SpmvChunk<kChunk, kF32>::Word Word;
#pragma unroll
    for (int q = 0; q < kChunk; q++) {
        if (k0 + q < W) {
            // non-temporal loads: the operator is read once per launch and leaves the caches to x
            const Word *vv = kF32 ? reinterpret_cast<const Word *>(v32 + (size_t)(k0 + q) * 3 * kSliceRows)
                                  : reinterpret_cast<const Word *>(v + (size_t)(k0 + q) * 3 * kSliceRows);
            c.a[q][0] = __builtin_nontemporal_load(vv);
            c.a[q][1] = __builtin_nontemporal_load(vv + kSliceRows);
            c.a[q][2] = __builtin_nontemporal_load(vv + 2 * kSliceRows);
        } else {
#pragma unroll
            for (int t = 0; t < 3; t++) c.a[q][t] = (Word){0, 0};
        }
    }
}
template <int kChunk, bool kF32>
__device__ __forceinline__ double spmv_fma(const SpmvChunk<kChunk, kF32> &c, const double2 *__restrict__ xs, int k0, int W, double acc)
{
#pragma unroll
    for (int q = 0; q < kChunk; q++) {
        if (k0 + q < W) {
            const double2 *xx = xs + (size_t)(k0 + q) * 3 * kSliceNodes;
            const double2 x0 = xx[0], x1 = xx[1], x2 = xx[2];
            acc += (double)c.a[q][0].x * x0.x;
            acc += (double)c.a[q][0].y * x0.y;
            acc += (double)c.a[q][1].x * x1.x;
            acc += (double)c.a[q][1].y * x1.y;
            acc += (double)c.a[q][2].x * x2.x;
            acc += (double)c.a[q][2].y * x2.y;
        }
    }
    return acc;
}

// (cheb: what the product does with its result, kernels.hpp SpmvEpilogue -- with a Chebyshev step y is r_out, base_vec r_in with
//  sign -1, x the direction d_in)
template <int kChunk, bool kF32 = false>
__global__ __launch_bounds__(192) void k_spmv(DeviceMatrix m, const double *__restrict__ x,
                                              double *__restrict__ y, double *__restrict__ partials,
                                              const CgScalars *s, const int32_t *__restrict__ order, int count,
                                              int panel, SpmvEpilogue cheb)
{
    const double *base_vec = cheb.base_vec;
    const double sign = cheb.sign;
    extern __shared__ double2 xs_all[]; // panel slots x 32 nodes x 3 words: x of the slice's block columns
    __shared__ double sh[3];
    __shared__ double rs[kSliceRows]; // Chebyshev epilogue: the slice's new residual, node-major
    if (s != nullptr && s->done != 0) return;
    const int t = threadIdx.x;
    const double2 *x2 = reinterpret_cast<const double2 *>(x);
    const double2 *xs = xs_all + 3 * (t & 31);
    double dotv = 0.0;
    for (SliceWalk w(count); w.valid(); w.next()) {
        const int sl = order != nullptr ? order[w.s] : w.s;
        const int64_t base = m.slice_base[sl];
        const int W = m.slice_width[sl];
        double acc = 0.0;
        double2 xw = make_double2(0.0, 0.0);
        // slices wider than the LDS panel (restriction operators of coarse multigrid levels: a coarse node collects
        // from every fine node its basis function touches) go through it in several passes
        for (int p0 = 0; p0 == 0 || p0 < W; p0 += panel) {
            const int Wp = W - p0 < panel ? W - p0 : panel;
            const double2 *v = reinterpret_cast<const double2 *>(m.vals + base * 36) + (size_t)p0 * 3 * kSliceRows + t;
            const int32_t *cols = m.cols + base + (int64_t)p0 * kSliceNodes;
            const float2 *v32 = kF32 ? reinterpret_cast<const float2 *>(m.vals32 + base * 36) + (size_t)p0 * 3 * kSliceRows + t : nullptr;
            // (the float variant keeps two chunks in flight: the second chunk's words travel during the staging of x as well, every
            //  later chunk while its predecessor is multiplied -- 96 registers of words; the FP64 variant has room for one)
            SpmvChunk<kChunk, kF32> ch, ch2;
            spmv_load<kChunk, kF32>(ch, v, 0, Wp, v32);
            if (kF32 && kChunk < Wp) spmv_load<kChunk, kF32>(ch2, v, kChunk, Wp, v32);
            __syncthreads(); // the previous panel's readers are done with xs_all
            for (int e = t; e < Wp * kSliceNodes; e += kSliceRows) {
                const double2 *xv = x2 + 3 * (int64_t)cols[e];
                const double2 x0 = xv[0], x1 = xv[1], x2w = xv[2];
                xs_all[3 * e] = x0;
                xs_all[3 * e + 1] = x1;
                xs_all[3 * e + 2] = x2w;
            }
            __syncthreads();
            acc = spmv_fma<kChunk, kF32>(ch, xs, 0, Wp, acc);
            if (kF32) {
                // slots in ascending order as before: ch (0), ch2 (kChunk), ch (2 kChunk), ch2 (3 kChunk), ...
                for (int k0 = kChunk; k0 < Wp; k0 += 2 * kChunk) {
                    if (k0 + kChunk < Wp) spmv_load<kChunk, kF32>(ch, v, k0 + kChunk, Wp, v32);
                    acc = spmv_fma<kChunk, kF32>(ch2, xs, k0, Wp, acc);
                    if (k0 + kChunk < Wp) {
                        if (k0 + 2 * kChunk < Wp) spmv_load<kChunk, kF32>(ch2, v, k0 + 2 * kChunk, Wp, v32);
                        acc = spmv_fma<kChunk, kF32>(ch, xs, k0 + kChunk, Wp, acc);
                    }
                }
            } else {
                for (int k0 = kChunk; k0 < Wp; k0 += kChunk) {
                    spmv_load<kChunk, kF32>(ch, v, k0, Wp, v32);
                    acc = spmv_fma<kChunk, kF32>(ch, xs, k0, Wp, acc);
                }
            }
            // x[row] is in LDS during the first panel: slot 0 is the diagonal block, its column is the lane's own node
            if (p0 == 0 && partials != nullptr) xw = xs[t >> 6]; // word (t / 32) / 2 of the node's six entries
        }
        const int64_t row = (int64_t)sl * kSliceRows + (t & 31) * 6 + (t >> 5);
        // base_vec: y = base + sign * K x (residual b - K x, prolongation x + P x_c); may alias y
        const double yv = base_vec != nullptr ? base_vec[row] + sign * acc : acc;
        y[row] = yv;
        if (cheb.prod_out != nullptr) {
            if (cheb.prod_float) reinterpret_cast<float *>(cheb.prod_out)[row] = (float)acc;
            else cheb.prod_out[row] = acc;
        }
        if (cheb.d_out != nullptr) {
            // (MEASURED, round 4: fetching the epilogue's operands -- D^-1 row, d, x, base vector -- ahead of the product, in an
            //  instantiation of its own, costs 24 registers and a wave per SIMD there and was 2 % SLOWER on the 4M solves
            //  although the small levels are latency chains: profiles/r04_spmv_epilogue_prefetch_ab.txt.  Left as it is.)
            // d_out = a d_in + c D^-1 r_out on the lane's row; the six residual entries of its node sit in six lanes of
            // three waves (lane = node + 32 dof): exchanged through LDS
            const int n = t & 31, i = t >> 5;
            double mrow[6];
            if (m.minv32 != nullptr) {
                const float *mi = m.minv32 + (int64_t)sl * kMinvWords * kSliceNodes + n;
#pragma unroll
                for (int j = 0; j < 6; j++) mrow[j] = (double)mi[minv_word(i < j ? i : j, i < j ? j : i) * kSliceNodes];
            } else {
                const double *mi = m.minv + (int64_t)sl * kMinvWords * kSliceNodes + n;
#pragma unroll
                for (int j = 0; j < 6; j++) mrow[j] = mi[minv_word(i < j ? i : j, i < j ? j : i) * kSliceNodes];
            }
            const double dv = cheb.start ? 0.0 : x[row], xv = cheb.start == 2 ? 0.0 : cheb.xsol[row];
            __syncthreads();
            rs[n * 6 + i] = yv;
            __syncthreads();
            double z = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) z += mrow[j] * rs[n * 6 + j];
            if (cheb.start) {
                // (the expression of k_cheb_start_node, so that the compiler contracts it the same way -- x = fma(c, z, x) -- and the
                //  fused start gives the bits of the separate pass)
                const double dn = cheb.c * z;
                cheb.d_out[row] = dn;
                cheb.xsol[row] = xv + dn;
            } else {
                const double dn = cheb.a * dv + cheb.c * z;
                cheb.d_out[row] = dn;
                cheb.xsol[row] = xv + dn;
            }
        }
        if (partials != nullptr) dotv += acc * (((t >> 5) & 1) ? xw.y : xw.x);
    }
    if (partials != nullptr) {
        const double tot = block_sum(dotv, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = tot;
    }
}

// =====================================================================================
// Symmetric storage (plan.hpp): of every off-diagonal pair of owned nodes only the block K_ac of the lower row a is
// stored.  Phase 1 (k_spmv_sym), one lane per NODE row: the lane streams the 36 words of each of its blocks once and
// uses them twice -- y_a += K_ac x_c for its own row and u = K_ac^T x_a for row c, written next to the slot (48
// bytes).  With a lane per node both products are lane-local: no reduction across lanes or waves.  Phase 2
// (k_sym_gather_node), one lane per node row again: y_c += sum of the u of the blocks (a, c), in the fixed order of the plan's
// in-lists -- deterministic, no atomics.  Traffic on the 4M-triangle panel: 2.31 GB of blocks + 0.29 GB of u written
// and read once, against 4.03 GB of blocks with full storage.  Two refinements: of the symmetric diagonal block only the
// words of the upper triangle are read (2.12 GB of blocks), and a product whose row c lies in the lane's own slice waits
// in LDS for the end of the slice instead of going through HBM (plan.hpp loc_index / loc_list: 0.19 GB of u).
// The fused dot x.Kx of CG needs no second phase: x.Kx = sum_a x_a.(direct part of y_a) + sum over stored
// off-diagonal blocks of x_c.u.
// =====================================================================================
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));
// (kNT: non-temporal loads -- an operator that is streamed once per launch and larger than the caches leaves them to the vectors;
//  kNT = false, plain loads: operators small enough for the 256 MB Infinity Cache to serve the NEXT product of the same cycle --
//  a level-1 operator of the 4M hierarchy is multiplied sixteen times per outer iteration)
template <bool kF32, bool kNT = true> __device__ __forceinline__ v2d load_word(const double2 *v, const float2 *v32, size_t off)
{
    if (kF32) {
        const v2f *p = reinterpret_cast<const v2f *>(v32) + off;
        const v2f w = kNT ? __builtin_nontemporal_load(p) : *p;
        v2d r;
        r.x = (double)w.x;
        r.y = (double)w.y;
        return r;
    }
    const v2d *p = reinterpret_cast<const v2d *>(v) + off;
    return kNT ? __builtin_nontemporal_load(p) : *p;
}

// the 18 words (jp, i) of block slot k: wd[jp * 6 + i] = columns 2jp, 2jp+1 of row i.  diag: only the words of the upper triangle
// are needed (slot 0 of a symmetric-storage row); the others stay unset
// kVal: 0 = FP64 values, 1 = the float copy (m.vals32)
template <int kVal, bool kDiag, bool kNT = true>
__device__ __forceinline__ void load_block_words(const double2 *v, const float2 *v32, int k, v2d wd[18])
{
#pragma unroll
    for (int e = 0; e < 18; e++)
        if (!kDiag || 2 * (e / 6) + 1 >= e % 6) wd[e] = load_word<(kVal == 1), kNT>(v, v32, ((size_t)k * 18 + e) * kSliceNodes);
}

// kVal: the blocks come from m.vals (0) or from m.vals32 (1: single precision, same layout); the arithmetic stays FP64
// (A bfloat16 copy -- 72 B per block -- was built and measured in round 5 and is gone again: the smoother's copy needs about 20
//  significant bits.  The residuals a cycle restricts are increments of products with that copy, and an error of 2^-8 ||A|| ||d||
//  in them is amplified by the coarse solves: the 4M-triangle panel did not converge at all, and the float copy rounded to 18 / 17 /
//  16 bits takes 129 / 186 / 394 iterations on the cylinder instead of 97: profiles/r05_smoother_significant_bits.txt.)
// kVec (with kVal >= 1 only; DeviceMatrix::vec32): 1 = y and the transposed products are stored as floats, 2 = x is read as floats too
// (The float-storing variants compile to 182-194 registers, two waves per SIMD where the FP64 product has three.  MEASURED, round
//  4: held to three waves -- amdgpu_waves_per_eu(3, 3), 168 registers, five dwords spilled -- the 4M solves take the same time
//  within the run-to-run scatter of 1 %: profiles/r04_spmv_sym_waves_ab.txt, four alternating rounds.  Left to the compiler.)
template <int kVal, int kVec, bool kNT = true>
__global__ __launch_bounds__(64) void k_spmv_sym(DeviceMatrix m, const double *__restrict__ x, double *__restrict__ y,
                                                 double *__restrict__ partials, const CgScalars *s,
                                                 const int32_t *__restrict__ order, int count)
{
    if (s != nullptr && s->done != 0) return;
    const int lane = threadIdx.x, half = lane >> 5, n = lane & 31;
    double dotv = 0.0;
    extern __shared__ double2 lds_products[]; // [half][max_loc][3]: transposed products that stay inside a slice
    const bool has_local = m.loc_index != nullptr;
    double2 *lu = lds_products + (size_t)half * m.max_loc * 3;
    const int n_pairs = (count + 1) >> 1;
    for (SliceWalk w(n_pairs); w.valid(); w.next()) {
        const int q = 2 * w.s + half;
        const bool live = q < count;
        const int sl = live ? (order != nullptr ? order[q] : q) : 0;
        const int64_t base = m.slice_base[sl];
        const int W = live ? m.slice_width[sl] : 0;
        const int a = sl * kSliceNodes + n;
        double xa[6], ya[6];
        load_node6(x, a, kVec == 2, xa);
#pragma unroll
        for (int i = 0; i < 6; i++) ya[i] = 0.0;
        const double2 *v = reinterpret_cast<const double2 *>(m.vals + base * 36) + n;
        const float2 *v32 = kVal == 1 ? reinterpret_cast<const float2 *>(m.vals32 + base * 36) + n : nullptr;
        double2 *tb = reinterpret_cast<double2 *>(m.tbuf + base * 6);
        float2 *tbf = reinterpret_cast<float2 *>(m.tbuf) + base * 3; // (kVec >= 1: float (slot * 6 + j) of the same buffer)
        const uint8_t *li = has_local ? m.loc_index + base + n : nullptr;
        if (W > 0) {
            // slot 0 is the diagonal block K_aa, which is symmetric: only the 12 of its 18 words that hold the upper
            // triangle are read (each word is 512 contiguous bytes of the slice, so the other six never leave HBM);
            // element (i, j) below the diagonal is taken from (j, i).  Same order of the sum over j as in the loop
            // below, so a block whose halves mirror each other exactly (k_assemble's do) gives the same bits.
            v2d wd[18];
            load_block_words<kVal, true, kNT>(v, v32, 0, wd);
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const int r = j >= i ? i : j, cl = j >= i ? j : i; // (r, cl): the element of the upper triangle
                    const v2d kw = wd[(cl >> 1) * 6 + r];
                    ya[i] += ((cl & 1) ? kw.y : kw.x) * xa[j];
                }
        }
        for (int k = 1; k < W; k++) {
            const int c = m.cols[base + (int64_t)k * kSliceNodes + n];
            v2d wd[18];
            load_block_words<kVal, false, kNT>(v, v32, k, wd); // word (jp = e/6, i = e%6)
            double xc[6];
            load_node6(x, c, kVec == 2, xc);
            double u[6];
#pragma unroll
            for (int j = 0; j < 6; j++) u[j] = 0.0;
#pragma unroll
            for (int jp = 0; jp < 3; jp++)
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const v2d kw = wd[jp * 6 + i];
                    ya[i] += kw.x * xc[2 * jp];
                    ya[i] += kw.y * xc[2 * jp + 1];
                    u[2 * jp] += kw.x * xa[i];
                    u[2 * jp + 1] += kw.y * xa[i];
                }
            // the transpose acts on row c when c is another owned row (ghost columns belong to another rank,
            // padding slots point at the own row)
            if (c != a && c < m.n_pad) {
                const int local = has_local ? (int)li[(size_t)k * kSliceNodes] : 255;
                // (row c is a row of this slice: the product waits in LDS for the end of the slice, else next to the slot)
                if (kVec >= 1 && local == 255) {
                    float2 *t = tbf + ((size_t)k * kSliceNodes + n) * 3;
                    t[0] = make_float2((float)u[0], (float)u[1]);
                    t[1] = make_float2((float)u[2], (float)u[3]);
                    t[2] = make_float2((float)u[4], (float)u[5]);
                } else {
                    double2 *t = local != 255 ? lu + local * 3 : tb + ((size_t)k * kSliceNodes + n) * 3;
                    t[0] = make_double2(u[0], u[1]);
                    t[1] = make_double2(u[2], u[3]);
                    t[2] = make_double2(u[4], u[5]);
                }
                if (partials != nullptr)
                    dotv += xc[0] * u[0] + xc[1] * u[1] + xc[2] * u[2] + xc[3] * u[3] + xc[4] * u[4] + xc[5] * u[5];
            }
        }
        if (live && partials != nullptr) // (before the in-slice products join: x_c.u counted them above)
            dotv += xa[0] * ya[0] + xa[1] * ya[1] + xa[2] * ya[2] + xa[3] * ya[3] + xa[4] * ya[4] + xa[5] * ya[5];
        if (has_local) {
            // the transposed products of this slice's own rows, in the order of the in-list
            __syncthreads(); // (one wave per workgroup)
            const int Wi = live ? m.in_width[sl] : 0;
            const uint8_t *ll = m.loc_list + m.in_base[sl] + n;
            for (int k = 0; k < Wi; k++) {
                const int idx = ll[(size_t)k * kSliceNodes];
                if (idx != 255) {
                    const double2 t0 = lu[idx * 3], t1 = lu[idx * 3 + 1], t2 = lu[idx * 3 + 2];
                    ya[0] += t0.x; ya[1] += t0.y; ya[2] += t1.x; ya[3] += t1.y; ya[4] += t2.x; ya[5] += t2.y;
                }
            }
            __syncthreads(); // the next slice overwrites the products
        }
        if (live) {
            if (kVec >= 1) {
                float2 *yo = reinterpret_cast<float2 *>(y) + 3 * (int64_t)a;
                yo[0] = make_float2((float)ya[0], (float)ya[1]);
                yo[1] = make_float2((float)ya[2], (float)ya[3]);
                yo[2] = make_float2((float)ya[4], (float)ya[5]);
            } else {
                double2 *yo = reinterpret_cast<double2 *>(y) + 3 * (int64_t)a;
                yo[0] = make_double2(ya[0], ya[1]);
                yo[1] = make_double2(ya[2], ya[3]);
                yo[2] = make_double2(ya[4], ya[5]);
            }
        }
    }
    if (partials != nullptr) {
        const double tot = wave_sum(dotv);
        if (threadIdx.x == 0) partials[blockIdx.x] = tot;
    }
}

// Is the operator of a size at which the next product of the same cycle finds it in the 256 MB Infinity Cache -- and at which that
// pays?  Upper bound of the bytes of its values from the padded slot count; plain loads between FEMSHELL_SPMV_CACHED_MIN_MB and
// FEMSHELL_SPMV_CACHED_MB (defaults 128 and 300; CACHED_MB=0: every operator is streamed with non-temporal loads as in rounds 1-4).
// MEASURED, round 5, alternating on one box (symmetric-storage smoothing products only): the level-1 operator of the 4M hierarchies
// (197 MB of floats, sixteen smoothing products per outer iteration) with plain loads: panel 0.6454 -> 0.6372 s, cylinder 0.6031 ->
// 0.5945 s; level 0 as well (1.2 GB): 0.6002 s -- it does not fit, and its lines evict the vectors; the 250k-triangle roof, whose
// level 0 is 72 MB: 0.0603 -> 0.0614 s -- an operator that small is gone from the L2s anyway and costs the vectors their place.
static bool operator_fits_the_caches(const DeviceMatrix &m)
{
    static const double max_mb = knob_double("FEMSHELL_SPMV_CACHED_MB", 300.0);
    static const double min_mb = knob_double("FEMSHELL_SPMV_CACHED_MIN_MB", 128.0);
    const double bytes_per_value = m.vals32 != nullptr ? 4.0 : 8.0;
    const double mb = (double)m.n_slices * m.max_slice_width * kSliceNodes * 36.0 * bytes_per_value * 1e-6;
    return mb <= max_mb && mb >= min_mb;
}

static void spmv_sym_phase1(const DeviceMatrix &m, const double *x, double *y, double *partials, const CgScalars *s,
                            const int32_t *order, int count, int grid, hipStream_t st, bool f32 = false)
{
    const size_t lds = m.loc_index != nullptr ? (size_t)2 * m.max_loc * 48 : 0;
    // operators whose single-precision values fit the Infinity Cache are read with plain loads: the next smoothing product of the
    // same visit finds them there (operator_fits_the_caches)
    if (f32 && m.vals32 != nullptr && m.vec32 == 2 && operator_fits_the_caches(m)) {
        hipLaunchKernelGGL((k_spmv_sym<1, 2, false>), dim3(grid), dim3(64), lds, st, m, x, y, partials, s, order, count);
        return;
    }
    if (f32 && m.vals32 != nullptr) {
        if (m.vec32 == 2) hipLaunchKernelGGL((k_spmv_sym<1, 2>), dim3(grid), dim3(64), lds, st, m, x, y, partials, s, order, count);
        else if (m.vec32 == 1) hipLaunchKernelGGL((k_spmv_sym<1, 1>), dim3(grid), dim3(64), lds, st, m, x, y, partials, s, order, count);
        else hipLaunchKernelGGL((k_spmv_sym<1, 0>), dim3(grid), dim3(64), lds, st, m, x, y, partials, s, order, count);
    } else {
        hipLaunchKernelGGL((k_spmv_sym<0, 0>), dim3(grid), dim3(64), lds, st, m, x, y, partials, s, order, count);
    }
}

__global__ __launch_bounds__(256) void k_to_f32(const double *__restrict__ src, float *__restrict__ dst, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = (float)src[i];
}

void launch_to_f32(const double *src, float *dst, int64_t n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(k_to_f32, dim3(4096), dim3(256), 0, st, src, dst, n);
}

// second phase, one lane per node (device_common.hpp node_gather): out = base_vec + sign * (y + the row's transposed products)
// (kQ32: y and the transposed products were stored as floats by a smoothing product, DeviceMatrix::vec32; out is FP64)
template <bool kQ32>
__global__ __launch_bounds__(64) void k_sym_gather_node(DeviceMatrix m, const double *y, double *out, const double *base_vec, double sign,
                                                        const CgScalars *s)
{
    if (s != nullptr && s->done != 0) return;
    const int half = threadIdx.x >> 5, n = threadIdx.x & 31;
    for (SliceWalk w(node_pairs(m.n_slices)); w.valid(); w.next()) {
        const int sl = 2 * w.s + half;
        if (sl >= m.n_slices) continue;
        const int64_t node = (int64_t)sl * kSliceNodes + n;
        double acc[6], bv[6];
        load_node6(y, node, kQ32, acc);
        if (base_vec != nullptr) load_node6(base_vec, node, false, bv);
        node_gather<kQ32>(m, sl, n, acc);
        if (base_vec != nullptr) {
#pragma unroll
            for (int j = 0; j < 6; j++) acc[j] = bv[j] + sign * acc[j];
        }
        store_node6(out, node, false, acc);
    }
}

void launch_sym_gather(const DeviceMatrix &m, double *y, const double *base_vec, double sign, const CgScalars *s, hipStream_t st,
                       bool q32, double *out)
{
    if (out == nullptr) out = y;
    if (q32) hipLaunchKernelGGL(k_sym_gather_node<true>, dim3(node_grid(m)), dim3(64), 0, st, m, y, out, base_vec, sign, s);
    else hipLaunchKernelGGL(k_sym_gather_node<false>, dim3(node_grid(m)), dim3(64), 0, st, m, y, out, base_vec, sign, s);
}

// Residual r = b - K x with the products and the row sums carried in double-double (error-free TwoProduct by FMA,
// TwoSum accumulation): on the thin-shell systems ||K|| ||x|| exceeds ||b|| by seven to nine orders of magnitude, so a
// residual evaluated in plain FP64 is rounding noise at 1e-7 ||b|| and restarting CG from it makes the answer worse.
// This kernel feeds the residual replacement of the multigrid-preconditioned solve (amg_solve.cpp).  Same data
// movement as k_spmv (HBM-bound at 0.2 flop/B; the five-fold arithmetic stays far below the FP64 ridge).
struct DD {
    double hi, lo;
};
// (with the default -ffp-contract=fast the compiler fuses acc.hi + a*x and a*x - bb into FMAs -- HIP's __dmul_rn /
// __dadd_rn are plain operators and `#pragma clang fp contract(off)` did not prevent it either; the product is
// therefore issued through inline assembly -- and the error terms below, which assume
// s = fl(acc.hi + fl(a x)), would be those of a different sum: measured, the "double-double" residual was then no
// better than the FP64 one)
__device__ __forceinline__ void dd_fma_acc(DD &acc, double a, double x)
{
    double p; // fl(a x) as an opaque instruction: neither pragmas nor the _rn intrinsics stop the backend from fusing
    asm("v_mul_f64 %0, %1, %2" : "=v"(p) : "v"(a), "v"(x));
    const double e = __fma_rn(a, x, -p);          // a*x = p + e exactly
    const double s = __dadd_rn(acc.hi, p);
    const double bb = __dsub_rn(s, acc.hi);
    const double err = __dadd_rn(__dsub_rn(acc.hi, __dsub_rn(s, bb)), __dsub_rn(p, bb)); // acc.hi + p = s + err exactly
    acc.hi = s;
    acc.lo = __dadd_rn(acc.lo, __dadd_rn(err, e));
}

__global__ __launch_bounds__(192) void k_residual_dd(DeviceMatrix m, const double *__restrict__ x, const double *__restrict__ b,
                                                     double *__restrict__ r)
{
    extern __shared__ double2 xs_all[];
    const int t = threadIdx.x;
    const double2 *x2 = reinterpret_cast<const double2 *>(x);
    for (SliceWalk w(m.n_slices); w.valid(); w.next()) {
        const int sl = w.s;
        const int64_t base = m.slice_base[sl];
        const int W = m.slice_width[sl];
        const double2 *v = reinterpret_cast<const double2 *>(m.vals + base * 36) + t;
        __syncthreads();
        for (int e = t; e < W * kSliceNodes; e += kSliceRows) {
            const double2 *xv = x2 + 3 * (int64_t)m.cols[base + e];
            xs_all[3 * e] = xv[0];
            xs_all[3 * e + 1] = xv[1];
            xs_all[3 * e + 2] = xv[2];
        }
        __syncthreads();
        const double2 *xs = xs_all + 3 * (t & 31);
        DD acc{0.0, 0.0};
        for (int k0 = 0; k0 < W; k0 += 4) {
            SpmvChunk<4> ch;
            spmv_load<4>(ch, v, k0, W);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (k0 + q < W) {
                    const double2 *xx = xs + (size_t)(k0 + q) * 3 * kSliceNodes;
#pragma unroll
                    for (int u = 0; u < 3; u++) {
                        const double2 xw = xx[u];
                        dd_fma_acc(acc, ch.a[q][u].x, xw.x);
                        dd_fma_acc(acc, ch.a[q][u].y, xw.y);
                    }
                }
            }
        }
        const int64_t row = (int64_t)sl * kSliceRows + (t & 31) * 6 + (t >> 5);
        // r = b - (hi + lo), the difference b - hi taken exactly
        const double bv = b[row];
        const double s = __dsub_rn(bv, acc.hi);
        const double bb = __dsub_rn(s, bv);
        const double err = __dadd_rn(__dsub_rn(bv, __dsub_rn(s, bb)), __dsub_rn(-acc.hi, bb));
        r[row] = __dadd_rn(s, __dsub_rn(err, acc.lo));
    }
}

// Double-double residual with symmetric storage: a lane per scalar row walks the blocks of its own row (row i of the
// block) and the blocks of its in-list (column i of the block, the transpose); used once per refinement pass.
__global__ __launch_bounds__(192) void k_residual_dd_sym(DeviceMatrix m, const double *__restrict__ x, const double *__restrict__ b,
                                                         double *__restrict__ r)
{
    const int t = threadIdx.x, n = t / 6, i = t % 6;
    for (SliceWalk w(m.n_slices); w.valid(); w.next()) {
        const int sl = w.s;
        const int64_t base = m.slice_base[sl];
        const int W = m.slice_width[sl];
        const int a = sl * kSliceNodes + n;
        DD acc{0.0, 0.0};
        for (int k = 0; k < W; k++) {
            const int c = (k == 0) ? a : m.cols[base + (int64_t)k * kSliceNodes + n];
            const double *blk = m.vals + base * 36 + (int64_t)k * 36 * kSliceNodes; // [(jp*6 + i)*32 + n]*2 + jj
            const double *xc = x + 6 * (int64_t)c;
            if (k == 0 && m.diag_upper) {
                // the diagonal block holds its upper triangle only: (i, j), j < i, is (j, i) -- same order of the sum over j
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const int r = j >= i ? i : j, cl = j >= i ? j : i;
                    dd_fma_acc(acc, blk[((size_t)((cl >> 1) * 6 + r) * kSliceNodes + n) * 2 + (cl & 1)], xc[j]);
                }
                continue;
            }
#pragma unroll
            for (int jp = 0; jp < 3; jp++) {
                const double *wd = blk + ((size_t)(jp * 6 + i) * kSliceNodes + n) * 2;
                dd_fma_acc(acc, wd[0], xc[2 * jp]);
                dd_fma_acc(acc, wd[1], xc[2 * jp + 1]);
            }
        }
        const int Wi = m.in_width[sl];
        const int64_t ib = m.in_base[sl];
        for (int k = 0; k < Wi; k++) {
            const int32_t slot = m.in_slots[ib + (int64_t)k * kSliceNodes + n];
            if (slot < 0) continue;
            const int src = m.in_rows[ib + (int64_t)k * kSliceNodes + n];
            const int ns = slot & 31;
            const double *blk = m.vals + (int64_t)(slot - ns) * 36; // the (slice, k) group of 32 blocks the slot sits in
            const double *xs = x + 6 * (int64_t)src;
            // column i of the block: entries K[i'][i], word (jp = i/2, i'), component i & 1
#pragma unroll
            for (int ip = 0; ip < 6; ip++)
                dd_fma_acc(acc, blk[((size_t)((i >> 1) * 6 + ip) * kSliceNodes + ns) * 2 + (i & 1)], xs[ip]);
        }
        const int64_t row = (int64_t)sl * kSliceRows + t;
        const double bv = b[row];
        const double sdd = __dsub_rn(bv, acc.hi);
        const double bb = __dsub_rn(sdd, bv);
        const double err = __dadd_rn(__dsub_rn(bv, __dsub_rn(sdd, bb)), __dsub_rn(-acc.hi, bb));
        r[row] = __dadd_rn(sdd, __dsub_rn(err, acc.lo));
    }
}

void launch_residual_dd(const DeviceMatrix &m, const double *x, const double *b, double *r, hipStream_t st)
{
    if (m.symmetric) {
        hipLaunchKernelGGL(k_residual_dd_sym, dim3(slice_grid(m)), dim3(192), 0, st, m, x, b, r);
        return;
    }
    const size_t lds = (size_t)m.max_slice_width * kSliceNodes * 3 * sizeof(double2);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_residual_dd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_residual_dd, dim3(slice_grid(m)), dim3(192), lds, st, m, x, b, r);
}

// Full-storage product with one lane per NODE row (round 5): y = base_vec + sign * K x for operators with few blocks per row -- the
// prolongations, 2.5 blocks per fine node.  k_spmv stages the x of a slice's block columns through LDS behind two barriers per
// slice, which pays for wide rows; with two to four slots a slice is two barriers around a handful of loads, and the prolongation
// onto level 0 of the 4M-triangle panel moved its 1.14 GB at 3.6 TB/s (312 us).  Here a lane streams the words of its blocks as
// k_spmv_sym does and reads the six entries of each column node straight from the caches.  Per row the sum runs over the slots
// in ascending order and inside a block over the columns in ascending order, as in k_spmv: same bits.
template <bool kF32>
__global__ __launch_bounds__(64) void k_spmv_node(DeviceMatrix m, const double *__restrict__ x, double *y, const CgScalars *s,
                                                  const double *base_vec, double sign, double *prod_out, int prod_float)
{
    if (s != nullptr && s->done != 0) return;
    const int half = threadIdx.x >> 5, n = threadIdx.x & 31;
    for (SliceWalk w(node_pairs(m.n_slices)); w.valid(); w.next()) {
        const int sl = 2 * w.s + half;
        if (sl >= m.n_slices) continue;
        const int64_t base = m.slice_base[sl];
        const int W = m.slice_width[sl];
        const int64_t node = (int64_t)sl * kSliceNodes + n;
        const double2 *v = reinterpret_cast<const double2 *>(m.vals + base * 36) + n;
        const float2 *v32 = kF32 ? reinterpret_cast<const float2 *>(m.vals32 + base * 36) + n : nullptr;
        double ya[6], bv[6];
#pragma unroll
        for (int i = 0; i < 6; i++) ya[i] = 0.0;
        if (base_vec != nullptr) load_node6(base_vec, node, false, bv);
        for (int k = 0; k < W; k++) {
            const int c = m.cols[base + (int64_t)k * kSliceNodes + n];
            v2d wd[18];
            load_block_words<(kF32 ? 1 : 0), false>(v, v32, k, wd);
            double xc[6];
            load_node6(x, c, false, xc);
#pragma unroll
            for (int jp = 0; jp < 3; jp++)
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const v2d kw = wd[jp * 6 + i];
                    ya[i] += kw.x * xc[2 * jp];
                    ya[i] += kw.y * xc[2 * jp + 1];
                }
        }
        if (prod_out != nullptr) store_node6(prod_out, node, prod_float != 0, ya);
        if (base_vec != nullptr) {
#pragma unroll
            for (int i = 0; i < 6; i++) ya[i] = bv[i] + sign * ya[i];
        }
        store_node6(y, node, false, ya);
    }
}

// rows narrower than this go through k_spmv_node (FEMSHELL_SPMV_NODE_WIDTH; 0 = never)
static int spmv_node_width()
{
    static const int w = (int)knob_long("FEMSHELL_SPMV_NODE_WIDTH", 8);
    return w;
}

static bool spmv_node_applies(const DeviceMatrix &m) { return !m.symmetric && m.max_slice_width > 0 && m.max_slice_width <= spmv_node_width(); }

constexpr int kSpmvPanel = 64; // block slots of x staged in LDS at a time by k_spmv
static void spmv_dispatch(const DeviceMatrix &m, const double *x, double *y, double *partials, const CgScalars *s,
                          const int32_t *order, int count, int grid, hipStream_t st, const SpmvEpilogue &e)
{
    static const int chunk = (int)knob_long("FEMSHELL_SPMV_CHUNK", 8); // tuning knob: block slots loaded together
    const dim3 g(grid), b(192);
    // x of the block columns, at most kSpmvPanel slots at a time (96 KiB of the CU's 160)
    const int panel = m.max_slice_width < kSpmvPanel ? (m.max_slice_width > 0 ? m.max_slice_width : 1) : kSpmvPanel;
    const size_t lds = (size_t)panel * kSliceNodes * 3 * sizeof(double2);
    // (k_spmv's own arrays -- sh, rs -- count towards a workgroup's LDS as well: a row of 42 blocks stays below 64 KiB with
    //  its panel alone and passes it with them)
    constexpr size_t kStaticLds = (3 + kSliceRows) * sizeof(double);
    auto launch = [&](auto kernel) {
        if (lds + kStaticLds > 64 * 1024) // beyond the default LDS limit (slices of 42 blocks and wider)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, g, b, lds, st, m, x, y, partials, s, order, count, panel, e);
    };
    // (MEASURED, round 5: plain loads here -- the latency-bound products of the small levels -- LOSE: with them the 4M panel keeps
    //  0.5 % of the 1.3 % the symmetric-storage products gain, and the 250k-triangle roof, all of whose operators fit, takes 0.0609 s
    //  instead of 0.0594 s.  The instantiations are gone; k_spmv streams every operator with non-temporal loads.)
    if (m.vals32 != nullptr) { // a product of the multigrid cycle on a single-precision copy of the values (amg_solve.cpp)
        launch(k_spmv<8, true>);
        return;
    }
    switch (chunk) {
    case 1: launch(k_spmv<1>); break;
    case 2: launch(k_spmv<2>); break;
    case 4: launch(k_spmv<4>); break;
    default: launch(k_spmv<8>); break;
    }
}

static int span_grid(const DeviceMatrix &m, int count)
{
    const int g = 8 * ((count + 7) / 8), cap = slice_grid(m);
    return g < cap ? g : cap;
}

int launch_spmv_sym_phase1(const DeviceMatrix &m, const double *x, double *y, double *partials, const CgScalars *s, hipStream_t st,
                           const SpmvSpan &span, bool single_precision_values)
{
    const int count = span.all() ? m.n_slices : span.count;
    if (count <= 0) return 0;
    const int grid = span.all() ? slice_grid(m) : span_grid(m, count);
    spmv_sym_phase1(m, x, y, partials, s, span.all() ? nullptr : span.order + span.begin, count, grid, st, single_precision_values);
    return grid;
}

int launch_spmv(const DeviceMatrix &m, const double *x, double *y, const SpmvEpilogue &e, const CgScalars *s, hipStream_t st,
                const SpmvSpan &span, double *partials)
{
    if (m.symmetric && (e.d_out != nullptr || e.prod_out != nullptr)) return -1; // (full storage only: kernels.hpp)
    if (!span.all()) { // (full storage: k_spmv_node walks all slices, a symmetric product ends with a pass over all rows)
        if (span.count <= 0) return 0;
        const int grid = span_grid(m, span.count);
        spmv_dispatch(m, x, y, partials, s, span.order + span.begin, span.count, grid, st, e);
        return grid;
    }
    // narrow rows that come with a base vector or a kept product: the prolongations and the residuals of operators as narrow.  (Plain
    // products -- restrictions, the K cycle's own, the CG's -- and Chebyshev epilogues have always gone through k_spmv.)
    if (spmv_node_applies(m) && e.d_out == nullptr && partials == nullptr && (e.base_vec != nullptr || e.prod_out != nullptr)) {
        const dim3 g(node_grid(m)), b(64);
        if (m.vals32 != nullptr) hipLaunchKernelGGL(k_spmv_node<true>, g, b, 0, st, m, x, y, s, e.base_vec, e.sign, e.prod_out, e.prod_float);
        else hipLaunchKernelGGL(k_spmv_node<false>, g, b, 0, st, m, x, y, s, e.base_vec, e.sign, e.prod_out, e.prod_float);
        return 0;
    }
    if (m.symmetric) { // (base_vec must not be y here: phase 1 overwrites y with the direct part)
        spmv_sym_phase1(m, x, y, partials, s, nullptr, m.n_slices, slice_grid(m), st);
        launch_sym_gather(m, y, e.base_vec, e.sign, s, st);
        return slice_grid(m);
    }
    spmv_dispatch(m, x, y, partials, s, nullptr, m.n_slices, slice_grid(m), st, e);
    return slice_grid(m);
}

} // namespace femshell
