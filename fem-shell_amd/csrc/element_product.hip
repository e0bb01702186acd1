// element_product.hip -- the matrix-free product with the UNCONSTRAINED stiffness, y = sum_e K_e x_e (gfx950, wave64).
//
// The assembly writes zero rows and columns with a counting diagonal for the fixed dofs (assemble_kernel.hpp), so the coupling
// blocks between free and constrained dofs and the constrained rows never reach HBM.  Prescribed displacements (the right-hand
// side F = mask(loads - K_unc u_bar)) and support reactions (r = K_unc u - loads) need exactly those, once or twice per load
// case: this kernel forms the product from the element records instead of a second stored matrix.
//
// One workgroup per slice (32 node rows), over the slice's element list (slice_elem_ptr / slice_elem_nodes, the list k_assemble
// builds its records from) in tiles of kTile elements:
//   A  one lane per element of the tile builds the element's record in LDS (tri3_record / quad4_record, the element's own
//      material where the context has sections) -- once per slice, as in k_assemble;
//   B  one lane per (element, local node): where that node is a row of this slice the lane forms the 6-vector
//      sum_b K_e[a,b] (x_b + xp_b) from the 3 or 4 blocks of the block row (block_add_rec, unconstrained) and leaves it in LDS;
//   C  one lane per scalar row (node, component) walks the tile IN LIST ORDER and adds the entries of the elements that contain
//      its node (the walk of k_lumped_mass).  The row sum stays in the lane's register from tile to tile: the order of the
//      additions is the list order whatever the tile size is, there are no atomics, and two launches give the same bits.
// The tile keeps the LDS of a workgroup under 64 KB (two workgroups per CU and more) at every list length the plan accepts; a
// structured slice (about 130 triangles) takes two tiles.
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "k_element_product assumes 32-node slices");

constexpr int kEpThreads = 256;
template <bool kHasQuads> struct EpLayout {
    static constexpr int nn = kHasQuads ? 4 : 3;                          // local nodes (block rows) per element
    static constexpr int rec = kHasQuads ? kRecDoublesQuad : kRecDoubles; // doubles per record
    static constexpr int tile = kHasQuads ? 64 : 128;                     // elements per tile
    // records | 6-vectors | node ids: 59,392 bytes (triangles), 47,104 bytes (with quadrilaterals)
    static constexpr int lds_bytes = tile * (rec * 8 + nn * 6 * 8 + 16);
};
static_assert(EpLayout<false>::lds_bytes <= 64 * 1024 && EpLayout<true>::lds_bytes <= 64 * 1024, "static LDS of k_element_product");

__device__ __forceinline__ int ep_node(const int4 &c, int j) { return j == 0 ? c.x : (j == 1 ? c.y : (j == 2 ? c.z : c.w)); }

// y[a] = sum_{e contains a} sum_{b in e} K_e[a,b] (x_b + xp_b) - sub[a] on the owned rows a, zero on padding rows.
// xp, sub: nullptr = absent.  rhs != 0: y[a] = fixed dof ? 0 : sub[a] - (the sum), the masked combine of the right-hand side.
template <bool kHasQuads, bool kSections>
__global__ __launch_bounds__(kEpThreads, 2) void k_element_product(DeviceMatrix m, MatConst mc, DeviceSections ds, const double *__restrict__ x,
                                                                const double *__restrict__ xp, const double *__restrict__ sub,
                                                                double *__restrict__ y, int rhs)
{
    using L = EpLayout<kHasQuads>;
    constexpr int kRec = L::rec, kNN = L::nn, kTile = L::tile;
    __shared__ __attribute__((aligned(16))) double s_rec[kTile * kRec];
    __shared__ double s_vec[kTile * kNN * 6];
    __shared__ int4 s_nodes[kTile]; // (-1, -1, -1, -1): a degenerate element, which contributes nothing
    const int tid = threadIdx.x;
    SliceWalk w(m.n_slices);
    for (; w.valid(); w.next()) {
        const int s = w.s;
        const int e0 = m.slice_elem_ptr[s], ne = m.slice_elem_ptr[s + 1] - e0;
        const int row0 = s * kSliceNodes;
        const int my_node = row0 + tid / 6, my_v = tid % 6; // phase C: lanes 0 .. 191
        double sum = 0.0;
        for (int t0 = 0; t0 < ne; t0 += kTile) {
            const int nt = min(kTile, ne - t0);
            // ---- A: records
            for (int i = tid; i < nt; i += kEpThreads) {
                int4 c = m.slice_elem_nodes[e0 + t0 + i];
                double rec[kRec];
                bool ok;
                const SecConst sc = kSections ? fetch_section(ds.table, ds.slice_elem_section[e0 + t0 + i]) : SecConst{0.0, 0.0, 0.0, 0.0};
                const MatConst me = kSections ? mat_of_section(sc, mc.flags) : mc; // the element's material
                if (!kHasQuads || c.w < 0) {
                    double X[9];
                    const int nid[3] = {c.x, c.y, c.z};
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const double *pt = m.xyz + 3 * (int64_t)nid[q];
                        X[3 * q + 0] = pt[0];
                        X[3 * q + 1] = pt[1];
                        X[3 * q + 2] = pt[2];
                    }
                    ok = tri3_record(X, me, rec);
                    if (kHasQuads) {
#pragma unroll
                        for (int q = kRecDoubles; q < kRec; q++) rec[q] = 0.0;
                    }
                } else {
                    double X[12];
                    const int nid[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const double *pt = m.xyz + 3 * (int64_t)nid[q];
                        X[3 * q + 0] = pt[0];
                        X[3 * q + 1] = pt[1];
                        X[3 * q + 2] = pt[2];
                    }
                    ok = quad4_record(X, me, rec);
                }
                const bool quad = kHasQuads && c.w >= 0;
                if (!ok) {
                    report_status(m.status, e0 + t0 + i + 1); // as the assembly reports it
                    c = make_int4(-1, -1, -1, -1);
                }
                s_nodes[i] = c;
                double2 *dst = reinterpret_cast<double2 *>(s_rec + (size_t)i * kRec);
#pragma unroll
                for (int q = 0; q < kRec / 2; q++) dst[q] = make_double2(rec[2 * q], rec[2 * q + 1]);
                // what phase B needs of the element's material, into the record where it lies in LDS (on the private copy the
                // kind-dependent word would be an indexed store, which the compiler answers with scratch)
                if (kSections && ok) rec_put_section<kHasQuads>(s_rec + (size_t)i * kRec, sc, quad);
            }
            __syncthreads();
            // ---- B: block rows times the element's x
            for (int it = tid; it < nt * kNN; it += kEpThreads) {
                const int i = it / kNN, ia = it % kNN;
                const int4 c = s_nodes[i];
                const int a = ep_node(c, ia);
                if (a < row0 || a >= row0 + kSliceNodes) continue; // not a row of this slice (or no such local node)
                const double *rec = s_rec + (size_t)i * kRec;
                const MatConst me = kSections ? rec_material<kHasQuads>(rec, mc.flags) : mc;
                double v6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1 // (one copy of the block code, local column as data: the assembly's register budget)
                for (int ib = 0; ib < kNN; ib++) {
                    const int b = ep_node(c, ib);
                    if (kHasQuads && b < 0) continue; // a triangle's fourth node
                    double xb[6];
                    load_node6(x, b, false, xb);
                    if (xp != nullptr) {
                        double xq[6];
                        load_node6(xp, b, false, xq);
#pragma unroll
                        for (int q = 0; q < 6; q++) xb[q] += xq[q];
                    }
                    double blk[36];
#pragma unroll
                    for (int q = 0; q < 36; q++) blk[q] = 0.0;
                    block_add_rec<kHasQuads>(rec, ia, ib, me, blk);
#pragma unroll
                    for (int r = 0; r < 6; r++)
#pragma unroll
                        for (int q = 0; q < 6; q++) v6[r] += blk[6 * r + q] * xb[q];
                }
                double *dst = s_vec + (size_t)it * 6;
#pragma unroll
                for (int r = 0; r < 6; r++) dst[r] = v6[r];
            }
            __syncthreads();
            // ---- C: row sums in list order
            if (tid < kSliceRows) {
                for (int i = 0; i < nt; i++) {
                    const int4 c = s_nodes[i];
#pragma unroll
                    for (int j = 0; j < kNN; j++)
                        if (ep_node(c, j) == my_node) sum += s_vec[(size_t)(i * kNN + j) * 6 + my_v];
                }
            }
            __syncthreads(); // (the next tile overwrites the records and the vectors)
        }
        if (tid < kSliceRows) {
            const int64_t row = (int64_t)s * kSliceRows + tid;
            double out = 0.0;
            if (my_node < m.n_own) {
                const double sb = sub != nullptr ? sub[row] : 0.0;
                if (rhs) out = ((m.dmask[my_node] >> my_v) & 1u) ? 0.0 : sb - sum;
                else out = sum - sb;
            }
            y[row] = out;
        }
    }
}

void launch_element_product(const DeviceMatrix &m, const MatConst &mc, const DeviceSections *sections, const double *x, const double *xp,
                            const double *sub, double *y, bool rhs, hipStream_t st)
{
    if (m.n_slices == 0) return;
    const DeviceSections ds = sections ? *sections : DeviceSections();
    const int g = slice_grid(m);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(g), dim3(kEpThreads), 0, st, m, mc, ds, x, xp, sub, y, rhs ? 1 : 0); };
    if (sections) { // (the instantiations with sections: contexts without never launch them)
        if (m.n_lquad > 0) launch(k_element_product<true, true>);
        else launch(k_element_product<false, true>);
    } else if (m.n_lquad > 0) {
        launch(k_element_product<true, false>);
    } else {
        launch(k_element_product<false, false>);
    }
}

} // namespace femshell
