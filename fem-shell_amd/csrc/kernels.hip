// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of libfemshell: the assembly side -- grids, the assembly kernels
// of assemble_kernel.hpp, constraint words, right-hand side, element matrices, the block-Jacobi setup.  The products are in
// spmv_kernels.hip, the CG vector kernels in cg_kernels.hip, structural dynamics in dynamics_kernels.hip.
//
// All these kernels are HBM-bandwidth-bound FP64 streaming kernels; none uses MFMA (the blocks
// are 6x6 and there is a single right-hand side, so there is no GEMM-shaped contraction).
// Layout rules they share (plan.hpp): a slice = 32 node rows = 192 scalar rows; per-slice
// kernels map one lane to one scalar row so that every matrix/vector stream is read with
// consecutive lanes on consecutive 16-byte (matrix) or 8-byte (vector) words; workgroup b
// works on slice (b%8)*ceil(S/8) + b/8 so that each XCD (blocks are dealt round-robin over
// the 8 XCDs) sweeps one contiguous eighth of the rows and its L2 keeps the x entries shared
// by neighbouring slices.
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

#include <type_traits>
#include "assemble_kernel.hpp"

#include <cstdlib>

namespace femshell {

static_assert(kSliceNodes == 32 && kSliceRows == 192, "kernels assume 32-node slices");

static int assemble_grid(const DeviceMatrix &m)
{
    static const int cap = grid_cap(knob_text("FEMSHELL_ASM_GRID"), 2048); // (plan.hpp: a multiple of 8, at least 8)
    const int g = 8 * ((m.n_slices + 7) / 8);
    return g < cap ? g : cap;
}

int slice_grid(const DeviceMatrix &m)
{
    // tuning knob; one slice per workgroup up to 2M node rows: best SpMV rate; more rows share workgroups
    static const int cap = grid_cap(knob_text("FEMSHELL_SLICE_GRID"), 65536);
    const int g = 8 * ((m.n_slices + 7) / 8);
    return g < cap ? g : cap;
}

// lab builds (-DFEMSHELL_SECTIONS_LAB=256|512|768, assemble_kernel.hpp): parts of the sectioned pipelined kernel of triangle
// meshes switched off, to time them; 0 in the product
#ifndef FEMSHELL_SECTIONS_LAB
#define FEMSHELL_SECTIONS_LAB 0
#endif
constexpr int kSectionsLab = FEMSHELL_SECTIONS_LAB;

bool launch_assemble(const DeviceMatrix &m, const MatConst &mc, hipStream_t st, const DeviceSections *sections)
{
    const size_t lds = (size_t)m.lds_bytes;
    const DeviceSections ds = sections ? *sections : DeviceSections();
    const int g = assemble_grid(m);
    auto launch = [&](auto kernel) {
        if (lds > 64 * 1024) // beyond the default dynamic-LDS limit
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, dim3(g), dim3(256), lds, st, m, mc, ds);
    };
    if (sections && (!ds.table || !ds.slice_elem_section)) return false; // (nothing launched: the caller reports it)
    if (m.pipe) { // two workgroups per CU, b and b + G/2 on the same one: their roles complement each other
        static const int pipe_cap = [] { // two workgroups per CU of this device (FEMSHELL_ASM_PIPE_GRID overrides)
            int dev = 0, cus = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
                cus = 256;
            return grid_cap(knob_text("FEMSHELL_ASM_PIPE_GRID"), 8 * ((2 * cus + 7) / 8));
        }();
        const int gp = g < pipe_cap ? g : pipe_cap;
        auto launch_pipe = [&](auto kernel) {
            if (lds > 64 * 1024)
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kernel, dim3(gp), dim3(256), lds, st, m, mc, ds);
        };
        if (sections) { // (the instantiations with sections: contexts without never launch them)
            if (m.n_lquad > 0) launch_pipe(k_assemble_pipe<0, true, true>);
            else launch_pipe(k_assemble_pipe<kSectionsLab, false, true>);
        } else if (m.n_lquad > 0) {
            launch_pipe(k_assemble_pipe<0, true>);
        } else {
            launch_pipe(k_assemble_pipe<0, false>);
        }
        return true;
    }
    if (sections) {
        if (m.n_lquad > 0) launch(k_assemble<2, 0, true, true>);
        else launch(k_assemble<2, 0, false, true>);
        return true;
    }
    // (compiled for two waves per SIMD: one is the same code, three and four spill -- profiles/sections_kernel_resources.txt)
    if (m.n_lquad > 0) launch(k_assemble<2, 0, true>);
    else launch(k_assemble<2, 0, false>);
    return true;
}

// Constraint word of every assembly work item (DeviceMatrix::item_flags): the assembly kernel fetches it together
// with the item, one slice ahead, instead of chasing cols -> dmask[col] in its block phase.
// (In kernel statistics this kernel can show 15-27 ms per call at 4M triangles: it is the first kernel behind the uploads
// of femshell_set_mesh / femshell_set_dirichlet -- launched twice in a row it takes 17 ms and 78 us, and 115 us behind the
// uploads of femshell_set_loads alone (tools/lab/flags_prof.sh, idle_prof.sh).  Idle gaps of up to half a second in front
// of a kernel cost it nothing.)
__global__ __launch_bounds__(256) void k_item_flags(DeviceMatrix m)
{
    for (int s = blockIdx.x; s < m.n_slices; s += gridDim.x) {
        const int64_t base = m.slice_base[s];
        const int i0 = m.item_ptr[s], ni = m.item_ptr[s + 1] - i0;
        for (int it = threadIdx.x; it < ni; it += blockDim.x) {
            const uint32_t x = m.items[i0 + it].x;
            const int slot_in_slice = (int)(x & 0xffffu), chunk = (int)((x >> 16) & 0xffu), nchunks = (int)(x >> 24);
            uint32_t f = 0u;
            if (chunk == 0 && nchunks > 0) {
                const int64_t slot = base + slot_in_slice;
                const int row = s * kSliceNodes + (slot_in_slice & 31), col = m.cols[slot];
                const uint32_t valence = (uint32_t)(m.pair_ptr[slot + 1] - m.pair_ptr[slot]);
                // (the plan accepts at most 765 contributions per slot, plan.cpp: ten bits hold the count in full -- it is the
                //  diagonal entry of a constrained dof; in the pipelined layout the word's 23 bits sit above the wave word's 9)
                f = (uint32_t)m.dmask[row] | ((uint32_t)m.dmask[col] << 6) | ((valence < kFlagValenceMask ? valence : kFlagValenceMask) << 12) |
                    (col == row ? 1u << kFlagDiagBit : 0u);
            }
            if (m.pipe) { // the pipelined kernel reads the word from the item itself: one load and 4 bytes per item less
                uint32_t *w = &const_cast<uint4 *>(m.items)[i0 + it].w;
                *w = (*w & ((1u << kPipeFlagShift) - 1u)) | (f << kPipeFlagShift);
            } else {
                m.item_flags[i0 + it] = f;
            }
        }
    }
}

void launch_item_flags(const DeviceMatrix &m, int64_t n_items, hipStream_t st)
{
    if (n_items == 0 || m.n_slices == 0) return;
    hipLaunchKernelGGL(k_item_flags, dim3(m.n_slices < 8192 ? m.n_slices : 8192), dim3(256), 0, st, m);
}

// Right-hand side: contribRHS (fem-shell.cpp:1118-1153) is a masked copy -- every node's load
// enters once, fixed dofs get 0 (fem-shell.cpp:1227).
__global__ void k_rhs(DeviceMatrix m, const double *loads, double *F)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)m.n_pad * 6) return;
    const int node = (int)(i / 6), v = (int)(i % 6);
    const bool fixed = (m.dmask[node] >> v) & 1u;
    F[i] = (fixed || node >= m.n_own) ? 0.0 : loads[i];
}

void launch_rhs(const DeviceMatrix &m, const double *loads, double *F, hipStream_t st)
{
    const int64_t n = (int64_t)m.n_pad * 6;
    hipLaunchKernelGGL(k_rhs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m, loads, F);
}

// Unconstrained element matrices in the reference's variable-major ordering
// (fem-shell.cpp:1105-1109); one lane per node block.  Parity/debug export only.
// Elements [0,n_ltri) are triangles (9 blocks each), the rest quads (16 blocks each).
__global__ __launch_bounds__(128) void k_element_matrices(DeviceMatrix m, MatConst mc_ctx, DeviceSections ds, int first, int count, double *out)
{
    const bool quads = first >= m.n_ltri;
    const int nn = quads ? 4 : 3, nb = nn * nn;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)count * nb) return;
    const int e = (int)(t / nb), pr = (int)(t % nb), ia = pr / nn, ib = pr % nn;
    // the element's own material where the context has sections
    const MatConst mc = ds.elem_section ? mat_of_section(ds.table[ds.elem_section[first + e]], mc_ctx.flags) : mc_ctx;
    double rec[kRecDoublesQuad];
    bool ok;
    if (!quads) {
        const int32_t *c = m.tri + 3 * (int64_t)(first + e);
        double X[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int d = 0; d < 3; d++) X[3 * i + d] = m.xyz[3 * (int64_t)c[i] + d];
        ok = tri3_record(X, mc, rec);
    } else {
        const int32_t *c = m.quad + 4 * (int64_t)(first + e - m.n_ltri);
        double X[12];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int d = 0; d < 3; d++) X[3 * i + d] = m.xyz[3 * (int64_t)c[i] + d];
        ok = quad4_record(X, mc, rec);
    }
    double acc[36];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0.0;
    if (ok) block_add_rec<true>(rec, ia, ib, mc, acc);
    else report_status(m.status, kStatusDirect + first + e);
    const int N = 6 * nn;
    double *Ke = out + (int64_t)e * N * N;
#pragma unroll
    for (int al = 0; al < 6; al++)
#pragma unroll
        for (int be = 0; be < 6; be++) Ke[(nn * al + ia) * N + nn * be + ib] = acc[6 * al + be];
}

void launch_element_matrices(const DeviceMatrix &m, const MatConst &mc, int32_t first, int32_t count,
                             double *Ke_out, hipStream_t st, const DeviceSections *sections)
{
    const int64_t n = (int64_t)count * (first >= m.n_ltri ? 16 : 9);
    hipLaunchKernelGGL(k_element_matrices, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, m, mc,
                       sections ? *sections : DeviceSections(), first, count, Ke_out);
}

// =====================================================================================
// Block-Jacobi setup: invert the 6x6 diagonal block of every owned node (Cholesky: the blocks are SPD)
// into the packed layout the CG vector kernels stream.
// =====================================================================================
__global__ void k_block_jacobi(DeviceMatrix m)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= m.n_pad) return;
    const int s = a / kSliceNodes, n = a % kSliceNodes;
    double *mi = m.minv + (int64_t)s * kMinvWords * kSliceNodes + n;
    if (a >= m.n_own) {
#pragma unroll
        for (int e = 0; e < kMinvWords; e++) mi[e * kSliceNodes] = 0.0;
        return;
    }
    const double2 *src = reinterpret_cast<const double2 *>(m.vals + m.slice_base[s] * 36);
    double A[6][6], B[6][6];
#pragma unroll
    for (int jp = 0; jp < 3; jp++)
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (m.diag_upper && 2 * jp + 1 < i) continue; // (never written: the mirror image below fills it in)
            const double2 v = src[(jp * 6 + i) * kSliceNodes + n];
            A[i][2 * jp] = v.x;
            A[i][2 * jp + 1] = v.y;
        }
    if (m.diag_upper) {
#pragma unroll
        for (int i = 1; i < 6; i++)
#pragma unroll
            for (int j = 0; j < i; j++) A[i][j] = A[j][i];
    }
    // Cholesky A = L L^T (the blocks are SPD), then A^-1 = L^-T L^-1: symmetric by construction and backward
    // stable without pivoting, which matters on sliver elements (block condition numbers around 1e9)
    double L[6][6], Li[6][6];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double d = A[c][c];
#pragma unroll
        for (int k = 0; k < c; k++) d -= L[c][k] * L[c][k];
        if (!(d > 0.0)) {
            ok = false;
            d = 1.0;
        }
        const double lcc = sqrt(d), il = 1.0 / lcc;
        L[c][c] = lcc;
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            double v = A[r][c];
#pragma unroll
            for (int k = 0; k < c; k++) v -= L[r][k] * L[c][k];
            L[r][c] = v * il;
        }
    }
    // Li = L^-1 (lower triangular) by forward substitution
#pragma unroll
    for (int c = 0; c < 6; c++) {
        Li[c][c] = 1.0 / L[c][c];
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            double v = 0.0;
#pragma unroll
            for (int k = c; k < r; k++) v -= L[r][k] * Li[k][c];
            Li[r][c] = v / L[r][r];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j2 = i; j2 < 6; j2++) {
            double v = 0.0;
#pragma unroll
            for (int k = j2; k < 6; k++) v += Li[k][i] * Li[k][j2];
            B[i][j2] = v;
        }
    if (!ok) {
        report_status(m.status, -(a + 1));
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j2 = i; j2 < 6; j2++) B[i][j2] = (i == j2) ? 1.0 : 0.0;
    }
    // the inverse of a symmetric block is symmetric: its upper triangle is stored (and applied), 21 words per node
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) mi[minv_word(i, j) * kSliceNodes] = B[i][j];
}

__global__ void k_status_flags(const int32_t *__restrict__ status, double *__restrict__ agree)
{
    const int32_t st = *status;
    agree[0] = st > 0 ? 1.0 : 0.0;
    agree[1] = st < 0 ? 1.0 : 0.0;
}

void launch_status_flags(const int32_t *status, double *agree, hipStream_t st)
{
    hipLaunchKernelGGL(k_status_flags, dim3(1), dim3(1), 0, st, status, agree);
}

void launch_block_jacobi(const DeviceMatrix &m, hipStream_t st)
{
    hipLaunchKernelGGL(k_block_jacobi, dim3((m.n_pad + 127) / 128), dim3(128), 0, st, m);
}

} // namespace femshell
