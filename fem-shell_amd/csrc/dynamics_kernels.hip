// dynamics_kernels.hip -- lumped mass and the vector kernels of a Newmark step (femshell_dynamics_*, api_dynamics.cpp).
#include "kernels.hpp"
#include "plan.hpp"
#include "device_common.hpp"

namespace femshell {

// =====================================================================================
// Structural dynamics: lumped mass and the vector kernels of a Newmark step (include/femshell.h).  One lane per node, as the
// smoother kernels of the multigrid cycle: the six entries of a vector are three 16-byte words of the lane, nothing goes
// through LDS and nothing waits at a barrier.
// =====================================================================================
__device__ __forceinline__ void node_xyz(const double *xyz, int node, double p[3])
{
    p[0] = xyz[3 * (int64_t)node];
    p[1] = xyz[3 * (int64_t)node + 1];
    p[2] = xyz[3 * (int64_t)node + 2];
}
__device__ __forceinline__ double cross_norm(const double a[3], const double b[3])
{
    const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    return sqrt(cx * cx + cy * cy + cz * cz);
}

// One lane per owned row walks its slice's element list in order and adds the shares of the elements that contain the row: no
// atomics, a fixed summation order.  (Every element that contains an owned node contributes to that node's diagonal block,
// so it is in the list of the node's slice whatever the storage is.)
__global__ __launch_bounds__(64) void k_lumped_mass(DeviceMatrix m, double2 rho_t, const double2 *__restrict__ sec_mass,
                                                    const int32_t *__restrict__ slice_elem_section, double *__restrict__ mass)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= m.n_pad) return;
    double mt = 0.0, mr = 0.0;
    if (a < m.n_own) {
        const int s = a / kSliceNodes;
        const int e0 = m.slice_elem_ptr[s], e1 = m.slice_elem_ptr[s + 1];
        for (int e = e0; e < e1; e++) {
            const int4 c = m.slice_elem_nodes[e];
            if (c.x != a && c.y != a && c.z != a && c.w != a) continue;
            double pa[3], pb[3], pc[3], d1[3], d2[3];
            node_xyz(m.xyz, c.x, pa);
            node_xyz(m.xyz, c.y, pb);
            node_xyz(m.xyz, c.z, pc);
            double share;
            if (c.w < 0) { // TRI3: A = |(b - a) x (c - a)| / 2, a third to each node
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    d1[d] = pb[d] - pa[d];
                    d2[d] = pc[d] - pa[d];
                }
                share = 0.5 * cross_norm(d1, d2) / 3.0;
            } else { // QUAD4: A = |d1 x d2| / 2 with the diagonals d1 = c - a, d2 = d - b, a quarter to each node
                double pd[3];
                node_xyz(m.xyz, c.w, pd);
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    d1[d] = pc[d] - pa[d];
                    d2[d] = pd[d] - pb[d];
                }
                share = 0.5 * cross_norm(d1, d2) / 4.0;
            }
            const double2 rt = sec_mass ? sec_mass[slice_elem_section[e]] : rho_t;
            mt += rt.x * share;
            mr += rt.y * share;
        }
    }
    const double out[6] = {mt, mt, mt, mr, mr, mr};
    store_node6(mass, a, false, out);
}

void launch_lumped_mass(const DeviceMatrix &m, double2 rho_t, const double2 *sec_mass, const int32_t *slice_elem_section, double *mass,
                        hipStream_t st)
{
    if (m.n_pad == 0) return;
    hipLaunchKernelGGL(k_lumped_mass, dim3((unsigned)((m.n_pad + 63) / 64)), dim3(64), 0, st, m, rho_t, sec_mass, slice_elem_section, mass);
}

// K_eff = K + shift M on the free dofs: the six diagonal words of the row's diagonal block (slot 0 of the row; entry (i, i) is
// component i & 1 of word (i / 2, i), which belongs to the upper triangle: written with DeviceMatrix::diag_upper too)
__global__ __launch_bounds__(64) void k_mass_shift(DeviceMatrix m, const double *__restrict__ mass, double shift)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= m.n_own) return;
    const int s = a / kSliceNodes, n = a % kSliceNodes;
    double *blk = m.vals + m.slice_base[s] * 36;
    const uint32_t fixed = m.dmask[a];
    double mv[6];
    load_node6(mass, a, false, mv);
#pragma unroll
    for (int i = 0; i < 6; i++)
        if (!((fixed >> i) & 1u)) blk[(((i >> 1) * 6 + i) * kSliceNodes + n) * 2 + (i & 1)] += shift * mv[i];
}

void launch_mass_shift(const DeviceMatrix &m, const double *mass, double shift, hipStream_t st)
{
    if (m.n_own == 0) return;
    hipLaunchKernelGGL(k_mass_shift, dim3((unsigned)((m.n_own + 63) / 64)), dim3(64), 0, st, m, mass, shift);
}

__global__ __launch_bounds__(256) void k_newmark_init(DeviceMatrix m, const double *__restrict__ mass, const double *__restrict__ F,
                                                      const double *__restrict__ Ku, const double *__restrict__ u0, const double *__restrict__ v0,
                                                      double alpha, double *__restrict__ u, double *__restrict__ v, double *__restrict__ a)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    double uu[6] = {0, 0, 0, 0, 0, 0}, vv[6] = {0, 0, 0, 0, 0, 0}, aa[6] = {0, 0, 0, 0, 0, 0};
    if (node < m.n_own) {
        const uint32_t fixed = m.dmask[node];
        double mv[6], f[6], ku[6] = {0, 0, 0, 0, 0, 0};
        load_node6(mass, node, false, mv);
        load_node6(F, node, false, f);
        if (u0) load_node6(u0, node, false, uu);
        if (v0) load_node6(v0, node, false, vv);
        if (Ku) load_node6(Ku, node, false, ku);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const bool free_dof = !((fixed >> i) & 1u);
            uu[i] = free_dof ? uu[i] : 0.0;
            vv[i] = free_dof ? vv[i] : 0.0;
            aa[i] = (free_dof && mv[i] > 0.0) ? (f[i] - alpha * mv[i] * vv[i] - ku[i]) / mv[i] : 0.0;
        }
    }
    store_node6(u, node, false, uu);
    store_node6(v, node, false, vv);
    store_node6(a, node, false, aa);
}

void launch_newmark_init(const DeviceMatrix &m, const double *mass, const double *F, const double *Ku, const double *u0, const double *v0,
                         double alpha, double *u, double *v, double *a, hipStream_t st)
{
    if (m.n_pad == 0) return;
    hipLaunchKernelGGL(k_newmark_init, dim3((unsigned)((m.n_pad + 255) / 256)), dim3(256), 0, st, m, mass, F, Ku, u0, v0, alpha, u, v, a);
}

__global__ __launch_bounds__(256) void k_newmark_rhs(DeviceMatrix m, NewmarkCoef k, const double *__restrict__ mass, const double *__restrict__ F,
                                                     const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ a,
                                                     double *__restrict__ b)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    double out[6] = {0, 0, 0, 0, 0, 0};
    if (node < m.n_own) {
        const uint32_t fixed = m.dmask[node];
        double mv[6], f[6], uu[6], vv[6], aa[6];
        load_node6(mass, node, false, mv);
        load_node6(F, node, false, f);
        load_node6(u, node, false, uu);
        load_node6(v, node, false, vv);
        load_node6(a, node, false, aa);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double inertia = k.a0 * uu[i] + k.a2 * vv[i] + k.a3 * aa[i];
            const double damping = k.a1 * uu[i] + k.a4 * vv[i] + k.a5 * aa[i];
            out[i] = ((fixed >> i) & 1u) ? 0.0 : f[i] + mv[i] * (inertia + k.alpha * damping);
        }
    }
    store_node6(b, node, false, out);
}

void launch_newmark_rhs(const DeviceMatrix &m, const NewmarkCoef &k, const double *mass, const double *F, const double *u, const double *v,
                        const double *a, double *b, hipStream_t st)
{
    if (m.n_pad == 0) return;
    hipLaunchKernelGGL(k_newmark_rhs, dim3((unsigned)((m.n_pad + 255) / 256)), dim3(256), 0, st, m, k, mass, F, u, v, a, b);
}

__global__ __launch_bounds__(256) void k_newmark_update(DeviceMatrix m, NewmarkCoef k, const double *__restrict__ x, const double *__restrict__ u,
                                                        const double *__restrict__ v, const double *__restrict__ a, double *__restrict__ u1,
                                                        double *__restrict__ v1, double *__restrict__ a1)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= m.n_pad) return;
    double un[6] = {0, 0, 0, 0, 0, 0}, vn[6] = {0, 0, 0, 0, 0, 0}, an[6] = {0, 0, 0, 0, 0, 0};
    if (node < m.n_own) {
        const uint32_t fixed = m.dmask[node];
        double xx[6], uu[6], vv[6], aa[6];
        load_node6(x, node, false, xx);
        load_node6(u, node, false, uu);
        load_node6(v, node, false, vv);
        load_node6(a, node, false, aa);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if ((fixed >> i) & 1u) continue;
            un[i] = xx[i];
            an[i] = k.a0 * (un[i] - uu[i]) - k.a2 * vv[i] - k.a3 * aa[i];
            vn[i] = vv[i] + k.dt * ((1.0 - k.gamma) * aa[i] + k.gamma * an[i]);
        }
    }
    store_node6(u1, node, false, un);
    store_node6(v1, node, false, vn);
    store_node6(a1, node, false, an);
}

void launch_newmark_update(const DeviceMatrix &m, const NewmarkCoef &k, const double *x, const double *u, const double *v, const double *a,
                           double *u1, double *v1, double *a1, hipStream_t st)
{
    if (m.n_pad == 0) return;
    hipLaunchKernelGGL(k_newmark_update, dim3((unsigned)((m.n_pad + 255) / 256)), dim3(256), 0, st, m, k, x, u, v, a, u1, v1, a1);
}

// partial sums of v.Mv, u.q and u.Mu: workgroup b over its contiguous stretch of the owned rows (the pattern of
// k_sqnorm_partials: a fixed grid, so the same sums whatever the device does)
__global__ __launch_bounds__(256) void k_newmark_energy_partials(DeviceMatrix m, const double *__restrict__ mass, const double *__restrict__ u,
                                                                 const double *__restrict__ v, const double *__restrict__ q,
                                                                 double *__restrict__ partials)
{
    __shared__ double sh[4];
    const int per = (m.n_own + gridDim.x - 1) / gridDim.x, b = blockIdx.x * per, e = min(b + per, m.n_own);
    double kin = 0.0, uq = 0.0, umu = 0.0;
    for (int node = b + threadIdx.x; node < e; node += blockDim.x) {
        double mv[6], uu[6], vv[6], qq[6];
        load_node6(mass, node, false, mv);
        load_node6(u, node, false, uu);
        load_node6(v, node, false, vv);
        load_node6(q, node, false, qq);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            kin += vv[i] * mv[i] * vv[i];
            uq += uu[i] * qq[i];
            umu += uu[i] * mv[i] * uu[i];
        }
    }
    kin = block_sum(kin, sh);
    uq = block_sum(uq, sh);
    umu = block_sum(umu, sh);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = kin;
        partials[gridDim.x + blockIdx.x] = uq;
        partials[2 * gridDim.x + blockIdx.x] = umu;
    }
}
// out3[j] = partials[j][0] + partials[j][1] + ... in index order (the pattern of k_sums_in_order; G <= 256)
__global__ __launch_bounds__(192) void k_newmark_energy_sums(const double *__restrict__ partials, int G, double *__restrict__ out3)
{
    __shared__ double buf[3][kEnergyGrid];
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = lane; i < G; i += 64) buf[j][i] = partials[j * G + i];
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < G; i++) s += buf[j][i];
        out3[j] = s;
    }
}

void launch_newmark_energy(const DeviceMatrix &m, const double *mass, const double *u, const double *v, const double *q, double *partials,
                           double *out3, hipStream_t st)
{
    hipLaunchKernelGGL(k_newmark_energy_partials, dim3(kEnergyGrid), dim3(256), 0, st, m, mass, u, v, q, partials);
    hipLaunchKernelGGL(k_newmark_energy_sums, dim3(1), dim3(192), 0, st, partials, kEnergyGrid, out3);
}

} // namespace femshell
