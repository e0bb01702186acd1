// amg_solve.cpp -- the multigrid preconditioner (amg.hpp) at work: the V / K cycle over the hierarchy in HBM, the norms and the
// flexible PCG around it, and the cycle's byte count.  The hierarchy itself is built by amg_hierarchy.cpp (amg_dist.cpp for the
// row-partitioned levels).  Replaces what `-pc_type gamg`-style options select inside PETSc's KSPSolve behind
// equation_systems.solve() (fem-shell.cpp:138, doc/implementation.tex:68-72).
#include "amg_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace femshell {

// ---- the cycle -------------------------------------------------------------------------------------------------------
// One code path for single-rank contexts and for row-partitioned ones (amg_dist.cpp).  On a row-partitioned level every
// operator product is preceded by a halo exchange of its input (level 0: beside the interior slices, cg_driver.cpp), a
// restriction by one of the residual and a prolongation by one of the coarse correction (P was smoothed across the cuts);
// the K cycle's dot products are all-reduced; below the last row-partitioned level the rank's rows of the restricted
// residual are all-gathered and the replicated levels run as on one rank.
namespace {

// FEMSHELL_AMG_FUSED_CHEB=0: product and Chebyshev step of the full-storage levels as two launches (A/B runs)
bool fused_cheb() { return knob_flag("FEMSHELL_AMG_FUSED_CHEB", true); }

// FEMSHELL_AMG_RESIDUAL_INCREMENT=0: the residual in front of a restriction as b - A x, a product of its own in FP64, and the
// post-smoothing from x += P x_c with a residual product of its own as well (A/B runs)
bool residual_increment() { return knob_flag("FEMSHELL_AMG_RESIDUAL_INCREMENT", true); }

// does the matrix view carry the single-precision copy of its values for the smoothing products?
bool has_lowp(const DeviceMatrix &A) { return A.vals32 != nullptr; }

// FEMSHELL_AMG_FUSE (bit mask; A/B runs and tests): the first step of a Chebyshev smoothing runs in the epilogue of the kernel that
// produces its residual.  1: k_pcg_update_start_node (the update of the flexible PCG + the second phase of q = K p + the start of the
// cycle's pre-smoothing on level 0); 2: k_sym_gather_start_node (second phase of the increment product in front of a post-smoothing,
// symmetric-storage levels) -- both repeat the arithmetic of the passes they replace bit for bit; 4: the same in the epilogue of
// k_spmv on full-storage levels (rounds x + c z as one multiply-add: not the same bits).  Default 3: measured on the 4M-triangle
// panel, with the one-lane-per-node vector kernels the fused passes take as long as the passes they replace (147 against 65 + 81
// us, 226 against 82 + 85 + 81 us: these kernels are bound by their load instructions, not by their bytes), so the gain is the
// launches only; bit 2 changed the iteration count by rounding luck (104 -> 106) and stays off.
int fuse_mask() { return (int)knob_long("FEMSHELL_AMG_FUSE", 3); }

struct Cycle {
    femshell_ctx *c;
    Amg &H;
    const CgScalars *gate;
    hipStream_t st;
    int rc = FEMSHELL_OK;
    const int fuse = fuse_mask();
    // level 0: the caller's kernel (k_pcg_update_start_node) has taken the first step of the pre-smoothing already -- d in L.d, x = d
    bool pre_started0 = false;

    bool dist(int l) const { return H.levels[(size_t)l]->dist; }
    void halo(int l, double *x)
    {
        if (rc || !dist(l)) return;
        rc = level_halo_exchange(c, *H.levels[(size_t)l]->halo, x, 6, st);
    }
    // Products of a row-partitioned level >= 1 with the halo exchange of their input BESIDE the slices that read owned columns only
    // (round 5; level 0 has done so since round 2, cg_driver.cpp spmv_with_halo): pack and grouped send/recv on the halo stream,
    // the interior slices on the main stream meanwhile, the slices with ghost columns behind the exchange.  FEMSHELL_HALO_OVERLAP=0,
    // or a level without the slice order: the blocking sequence halo(l, x) + product.
    bool overlap(int l) const
    {
        const AmgLevel &L = *H.levels[(size_t)l];
        return L.dist && l >= 1 && c->halo_overlap && c->halo_stream != nullptr && L.order.p != nullptr && L.n_interior >= 0;
    }
    // span(begin, count): launches the product over the slices order[begin, begin + count) of level l on the main stream
    template <class Span> void overlapped(int l, double *x, Span span)
    {
        if (rc) return;
        AmgLevel &L = *H.levels[(size_t)l];
        const int ns = L.n_pad / kSliceNodes;
        hipError_t e = hipEventRecord(c->ev_p_ready, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->halo_stream, c->ev_p_ready, 0);
        if (e == hipSuccess) {
            rc = level_halo_exchange(c, *L.halo, x, 6, c->halo_stream);
            if (rc) return;
            e = hipEventRecord(c->ev_halo_done, c->halo_stream);
        }
        if (e == hipSuccess) {
            span(0, L.n_interior);
            e = hipStreamWaitEvent(st, c->ev_halo_done, 0);
        }
        if (e != hipSuccess) {
            rc = set_err(FEMSHELL_ERR_HIP, std::string("multigrid cycle, overlapped halo exchange: ") + hipGetErrorString(e));
            return;
        }
        span(L.n_interior, ns - L.n_interior);
    }
    // y = op(A x) of level l (>= 1 row-partitioned: overlapped when possible): first phase of a symmetric-storage product, or a
    // full-storage product with epilogue e
    void sym_phase1(int l, const DeviceMatrix &A, double *x, double *y)
    {
        if (overlap(l)) {
            const int32_t *order = H.levels[(size_t)l]->order.p;
            overlapped(l, x, [&](int b, int n) { launch_spmv_sym_phase1(A, x, y, nullptr, gate, st, SpmvSpan{order, b, n}, has_lowp(A)); });
            return;
        }
        halo(l, x);
        launch_spmv_sym_phase1(A, x, y, nullptr, gate, st, SpmvSpan(), has_lowp(A));
    }
    void full_product(int l, const DeviceMatrix &A, double *x, double *y, const SpmvEpilogue &e)
    {
        if (overlap(l)) {
            const int32_t *order = H.levels[(size_t)l]->order.p;
            overlapped(l, x, [&](int b, int n) { launch_spmv(A, x, y, e, gate, st, SpmvSpan{order, b, n}); });
            return;
        }
        halo(l, x);
        launch_spmv(A, x, y, e, gate, st);
    }
    // y = K x on level 0 of a row-partitioned context: the halo exchange beside the interior slices (symmetric storage with
    // defer: the direct part only, the consumer collects the transposed products)
    // (lowp: a smoothing product on the single-precision copy of K's values that matrix view carries)
    void product0(double *x, double *y, bool defer, const DeviceMatrix *lowp = nullptr, int vec32 = 0)
    {
        if (rc) return;
        CgVectors vv;
        vv.s = const_cast<CgScalars *>(gate);
        int np = 0;
        rc = spmv_with_halo(c, vv, x, y, nullptr, &np, defer, lowp != nullptr ? lowp->vals32 : nullptr, vec32);
    }
    // out = b - A_l x
    void residual(int l, const double *b, double *x, double *out)
    {
        AmgLevel &L = *H.levels[(size_t)l];
        const DeviceMatrix &A = amg_level_matrix(c, l);
        if (l == 0 && dist(0)) {
            if (A.symmetric) {
                product0(x, out, true);
                launch_sym_gather(A, out, b, -1.0, gate, st);
            } else {
                product0(x, L.q.p, false);
                launch_sub(b, L.q.p, out, 6ll * A.n_pad, st);
            }
            return;
        }
        halo(l, x);
        SpmvEpilogue e;
        e.base_vec = b;
        e.sign = -1.0;
        launch_spmv(A, x, out, e, gate, st);
    }

    // (r_given: the residual of x, where the caller has it -- in L.r or a vector of its own, never L.q or L.d)
    // (d_started: the kernel that produced the residual took the first step too -- d = inv_theta D^-1 r in this vector, L.d or, on a
    //  full-storage level, L.q; x updated)
    // the cluster blocks' share of a smoothing step that applied c D^-1 r with the point blocks (amg_patch.hpp): d += c M r, x += c M r
    void patch(int l, const double *r, double coef, double *d, bool d_float, double *x)
    {
        AmgLevel &L = *H.levels[(size_t)l];
        if (rc || !L.patches) return;
        launch_patch_correct(L.patches->view(), r, coef, d, d_float, x, gate, st);
    }
    void smooth(int l, const double *b, double *x, bool zero_guess, const double *r_given = nullptr, double *d_started = nullptr)
    {
        AmgLevel &L = *H.levels[(size_t)l];
        // (the operator as the smoother sees it: single-precision copies of the values and of D^-1 where the level has them)
        const DeviceMatrix &A = L.smooth_ready ? L.smooth_dm : amg_level_matrix(c, l);
        // what the smoothing products keep in single precision besides the operator's values (DeviceMatrix::vec32)
        const int v32 = (A.symmetric && has_lowp(A)) ? A.vec32 : 0;
        const double *rcur = b;
        if (!zero_guess) {
            if (r_given == nullptr) residual(l, b, x, L.r.p);
            rcur = r_given != nullptr ? r_given : L.r.p;
        }
        if (d_started == nullptr) launch_cheb_start(A, rcur, L.d.p, x, L.inv_theta, !zero_guess, gate, st, v32);
        // full-storage levels: the direction alternates between the two vectors
        double *d_cur = d_started != nullptr ? d_started : L.d.p, *d_next = d_cur == L.d.p ? L.q.p : L.d.p;
        const bool d_is_float = v32 == 2; // (the direction of a symmetric-storage level that keeps it in single precision)
        patch(l, rcur, L.inv_theta, d_cur, d_is_float, x); // (behind a fused start as well: the kernel that took it applied the point blocks)
        for (size_t k = 0; k < L.cheb_a.size(); k++) {
            if (l == 0 && dist(0)) {
                product0(L.d.p, L.q.p, A.symmetric != 0, &A, v32);
                launch_cheb_step(A, rcur, L.q.p, L.r.p, L.d.p, x, L.cheb_a[k], L.cheb_c[k], gate, st, A.symmetric != 0, v32);
                patch(l, L.r.p, L.cheb_c[k], L.d.p, d_is_float, x);
            } else if (A.symmetric) { // first phase of the product; the step kernel collects the transposed products
                sym_phase1(l, A, L.d.p, L.q.p);
                launch_cheb_step(A, rcur, L.q.p, L.r.p, L.d.p, x, L.cheb_a[k], L.cheb_c[k], gate, st, true, v32);
                patch(l, L.r.p, L.cheb_c[k], L.d.p, d_is_float, x);
            } else if (fused_cheb()) { // product and step in one launch (the small levels are bound by launch latency)
                SpmvEpilogue e;
                e.base_vec = rcur;
                e.sign = -1.0;
                e.d_out = d_next;
                e.xsol = x;
                e.a = L.cheb_a[k];
                e.c = L.cheb_c[k];
                full_product(l, A, d_cur, L.r.p, e);
                patch(l, L.r.p, L.cheb_c[k], d_next, false, x);
                std::swap(d_cur, d_next);
            } else {
                halo(l, L.d.p);
                launch_spmv(amg_level_matrix(c, l), L.d.p, L.q.p, SpmvEpilogue(), gate, st);
                launch_cheb_step(A, rcur, L.q.p, L.r.p, L.d.p, x, L.cheb_a[k], L.cheb_c[k], gate, st);
                patch(l, L.r.p, L.cheb_c[k], L.d.p, false, x);
            }
            rcur = L.r.p;
        }
        last_r = rcur;
        last_d = A.symmetric || (l == 0 && dist(0)) ? L.d.p : d_cur;
    }
    // what the last smooth() left: the residual of its iterate BEFORE the last direction was added, and that direction
    const double *last_r = nullptr;
    double *last_d = nullptr;

    // r_base - A dvec without a product with the iterate.  Right behind a pre-smoothing from a zero guess the smoother carries
    // the residual of its iterate up to the last direction d it added, so b - A x = last_r - A d; behind the coarse-grid
    // correction e = P x_c the residual is the one that was restricted minus A e.  Either way the product is with an
    // INCREMENT of the iterate, its result of the size of the residual itself -- not of ||A|| ||x||, seven to nine decades
    // above it -- and the single-precision copy of the values serves (relative error 1e-7 of the increment; the numpy
    // restatement with these products rounded needs the same iterations, tools/lab/f32_vectors_experiment.py).
    // Returns where the result is: L.r, or L.q for the first of the two on a symmetric-storage level in FP64.
    // (start_x: the result is the residual a post-smoothing of the iterate start_x begins with -- where the kernel that finishes
    //  the product can take the smoothing's first step as well it does, d = inv_theta D^-1 r and start_x += d, and *d_started
    //  receives the vector that holds d; else *d_started stays null)
    double *residual_minus_product(int l, const double *r_base, double *dvec, double *start_x = nullptr, double **d_started = nullptr)
    {
        AmgLevel &L = *H.levels[(size_t)l];
        const DeviceMatrix &A = L.smooth_ready ? L.smooth_dm : amg_level_matrix(c, l);
        // (a product that left its results in single precision -- DeviceMatrix::vec32 -- is collected into L.r, FP64)
        const bool q32 = A.symmetric && has_lowp(A) && A.vec32 >= 1;
        const bool d32 = q32 && A.vec32 == 2;
        const bool start = start_x != nullptr && d_started != nullptr && (fuse & (A.symmetric ? 2 : 4)) != 0;
        // the buffer the direct part of a symmetric product lands in: not the one the base vector lives in
        double *pb = (!q32 && r_base == L.q.p) ? L.r.p : L.q.p;
        // second phase of a symmetric product, with the smoothing's first step where asked for (dvec has been read by then: d
        // goes to L.d, where the step kernels of a symmetric-storage level expect it)
        auto gather = [&]() -> double * {
            double *out = q32 ? L.r.p : pb;
            if (start) {
                launch_sym_gather_start(A, pb, out, r_base, -1.0, L.d.p, start_x, L.inv_theta, q32, d32, gate, st);
                *d_started = L.d.p;
            } else if (q32) {
                launch_sym_gather(A, pb, r_base, -1.0, gate, st, true, L.r.p);
            } else {
                launch_sym_gather(A, pb, r_base, -1.0, gate, st);
            }
            return out;
        };
        if (l == 0 && dist(0)) {
            if (A.symmetric) {
                product0(dvec, pb, true, &A, A.vec32);
                return gather();
            }
            product0(dvec, L.q.p, false);
            launch_sub(r_base, L.q.p, L.r.p, 6ll * A.n_pad, st);
            return L.r.p;
        }
        if (A.symmetric) {
            sym_phase1(l, A, dvec, pb);
            return gather();
        }
        // (dvec is L.d or L.q, never L.r; r_base may be L.r)
        SpmvEpilogue e;
        e.base_vec = r_base;
        e.sign = -1.0;
        if (start) {
            // the product's Chebyshev epilogue as a first step: r = r_base - A dvec, d = inv_theta D^-1 r into the other direction vector
            double *d_out = dvec == L.d.p ? L.q.p : L.d.p;
            e.d_out = d_out;
            e.xsol = start_x;
            e.c = L.inv_theta;
            e.start = 1;
            *d_started = d_out;
        }
        full_product(l, A, dvec, L.r.p, e);
        return L.r.p;
    }

    // x = M_l(b): one cycle on level l
    void cycle(int l, const double *b, double *x)
    {
        AmgLevel &L = *H.levels[(size_t)l];
        if ((size_t)l + 1 == H.levels.size()) {
            if (H.coarse_lda > 0) launch_dense_gemv_big(H.coarse_inv.p, H.coarse_inv32.p, H.coarse_lda, b, x, 6 * L.n, 6 * L.n_pad, gate, st);
            else launch_dense_gemv(H.coarse_inv.p, b, x, 6 * L.n, 6 * L.n_pad, gate, st);
            return;
        }
        AmgLevel &N = *H.levels[(size_t)l + 1];
        if (l == 0 && pre_started0) {
            pre_started0 = false;
            smooth(l, b, x, true, nullptr, L.d.p);
        } else {
            smooth(l, b, x, true);
        }
        double *rf = L.r.p; // r = b - A x
        const bool increments = residual_increment();
        if (increments) rf = residual_minus_product(l, last_r, last_d);
        else residual(l, b, x, L.r.p);
        // b_c = R r
        if (dist(l)) {
            halo(l, rf); // (R = P^T reaches the rows of the neighbours' nodes along the cut)
            if (N.dist) {
                launch_spmv(L.R.dm, rf, N.b.p, SpmvEpilogue(), gate, st);
            } else {
                // the rank's rows of the restricted residual, all-gathered into the replicated level
                launch_spmv(L.R.dm, rf, L.bown.p, SpmvEpilogue(), gate, st);
                if (N.part_begin.size() + 1 != N.part.size()) { // (once per hierarchy, not per restriction)
                    N.part_begin.assign(N.part.begin(), N.part.end() - 1);
                    N.part_end.assign(N.part.begin() + 1, N.part.end());
                }
                std::string e;
                if (!rc && !comm_gather_rows(c->comm, L.bown.p, N.b.p, N.part_begin, N.part_end, st, &e)) rc = set_err(FEMSHELL_ERR_COMM, e);
            }
        } else {
            launch_spmv(L.R.dm, rf, N.b.p, SpmvEpilogue(), gate, st);
        }
        const bool next_is_coarsest = (size_t)l + 2 == H.levels.size();
        // (every level above the coarsest is wrapped into the K cycle's two Krylov steps: they cannot be taken off any level --
        //  4M-triangle panel 100 -> 196 iterations with the K cycle on level 1 only, profiles/r06_kcycle_levels.txt)
        if (H.opt.cycle == FEMSHELL_CYCLE_K && !next_is_coarsest) kcycle(l + 1);
        else cycle(l + 1, N.b.p, N.x.p);
        if (N.dist) halo(l + 1, N.x.p);
        if (increments) {
            // x += e, e = P x_c kept in the direction vector -- as floats where the smoothing products read theirs as floats --
            // and the residual the post-smoothing starts from is the restricted one minus A e (with b - A x, an FP64 product with
            // the iterate, in its place the CG broke down on the strip and Delaunay meshes: profiles/r04_breakdown_probe.txt)
            const DeviceMatrix &A = L.smooth_ready ? L.smooth_dm : amg_level_matrix(c, l);
            const bool e32 = A.symmetric && has_lowp(A) && A.vec32 == 2;
            SpmvEpilogue keep;
            keep.base_vec = x;
            keep.prod_out = L.d.p;
            keep.prod_float = e32 ? 1 : 0;
            launch_spmv(L.P.dm, N.x.p, x, keep, gate, st);
            double *d_started = nullptr;
            const double *r2 = residual_minus_product(l, rf, L.d.p, x, &d_started);
            smooth(l, b, x, false, r2, d_started);
            return;
        }
        SpmvEpilogue add;
        add.base_vec = x;
        launch_spmv(L.P.dm, N.x.p, x, add, gate, st); // x += P x_c
        smooth(l, b, x, false);
    }

    // y = A_l x on the FP64 operator of level l (the K cycle's own products)
    void krylov_product(int l, const DeviceMatrix &A, double *x, double *y)
    {
        if (A.symmetric) {
            sym_phase1(l, A, x, y);
            launch_sym_gather(A, y, nullptr, 1.0, gate, st);
        } else {
            full_product(l, A, x, y, SpmvEpilogue());
        }
    }

    // two steps of flexible CG on A_l x = b_l preconditioned by the cycle (Notay & Vassilevski's K cycle)
    void kcycle(int l)
    {
        AmgLevel &L = *H.levels[(size_t)l];
        const DeviceMatrix &A = amg_level_matrix(c, l);
        const int64_t n6 = 6ll * L.n_pad;
        const bool small = n6 <= kKcycSmall && !L.dist; // coefficient steps as single launches (amg_kernels.hpp)
        // row-partitioned level: the rank's sums are in L.ksums (left there by the last workgroup of the dot-product kernel); the
        // kernel that applies the coefficients forms them from the all-reduced sums itself -- three launches per coefficient step
        // where rounds 4-5 had five (two one-workgroup kernels around the collective: 12.7 launches of 4.3 us per outer iteration
        // on the 1/8 strip of the 4M panel, profiles/r06_dist_budget_N8.txt)
        auto reduce = [&]() {
            std::string e;
            if (!rc && !comm_allreduce_sum(c->comm, L.ksums.p, 3, st, &e)) rc = set_err(FEMSHELL_ERR_COMM, e);
        };
        cycle(l, L.b.p, L.c1.p);
        krylov_product(l, A, L.c1.p, L.v1.p);
        if (small) {
            launch_kcyc_step1_small(L.c1.p, L.v1.p, L.b.p, L.r2.p, n6, L.ks.p, gate, st);
        } else {
            if (L.dist) {
                launch_kcyc_dots_local(1, L.c1.p, L.v1.p, L.c1.p, L.b.p, nullptr, nullptr, n6, L.kscratch.p, L.ksums.p, gate, st);
                reduce();
            } else {
                launch_kcyc_dots(1, L.c1.p, L.v1.p, L.c1.p, L.b.p, nullptr, nullptr, n6, L.ks.p, L.kscratch.p, gate, st);
            }
            launch_kcyc_r2(L.b.p, L.v1.p, L.r2.p, n6, L.ks.p, gate, st, L.dist ? L.ksums.p : nullptr);
        }
        cycle(l, L.r2.p, L.c2.p);
        krylov_product(l, A, L.c2.p, L.v2.p);
        if (small) {
            launch_kcyc_step2_small(L.c1.p, L.c2.p, L.v1.p, L.v2.p, L.r2.p, L.x.p, n6, L.ks.p, gate, st);
        } else {
            if (L.dist) {
                launch_kcyc_dots_local(2, L.c2.p, L.v1.p, L.c2.p, L.v2.p, L.c2.p, L.r2.p, n6, L.kscratch.p, L.ksums.p, gate, st);
                reduce();
            } else {
                launch_kcyc_dots(2, L.c2.p, L.v1.p, L.c2.p, L.v2.p, L.c2.p, L.r2.p, n6, L.ks.p, L.kscratch.p, gate, st);
            }
            launch_kcyc_combine(L.c1.p, L.c2.p, L.x.p, n6, L.ks.p, gate, st, L.dist ? L.ksums.p : nullptr);
        }
    }
};

// host side of the stopping test
struct AmgPoll {
    int32_t next_check = 1, step = 1;
    int operator()(femshell_ctx *c, const CgVectors &v, int32_t it, int32_t max_it, CgScalars *hs)
    {
        if (it + 1 != next_check && it + 1 < max_it) return 0;
        FS_HIP(hipMemcpyAsync(hs, v.s, sizeof *hs, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(hipStreamSynchronize(c->stream));
        CommWatch::heartbeat(); // (progress: the watchdog of multi-rank contexts counts from here again)
        if (hs->done != 0) return 1;
        if (step < 4) step *= 2;
        next_check += step;
        return 0;
    }
};

} // namespace

double *amg_apply_iterate(femshell_ctx *c, double *z) { return c->amg->dist ? c->amg->dist->x0.p : z; }

int amg_apply(femshell_ctx *c, const double *r, double *z, const CgScalars *gate, bool pre_started)
{
    Cycle cy{c, *c->amg, gate, c->stream};
    cy.pre_started0 = pre_started;
    if (c->amg->dist) {
        // the iterate of level 0 is an input of the halo product: it needs ghost space, which the CG's z does not have
        double *x = c->amg->dist->x0.p;
        cy.cycle(0, r, x);
        launch_copy(x, z, 6ll * c->plan.n_pad, gate, c->stream);
    } else {
        cy.cycle(0, r, z);
    }
    if (cy.rc) return cy.rc;
    FS_HIP(hipGetLastError());
    return FEMSHELL_OK;
}

// ||a||^2 and ||b||^2 over the owned rows of all ranks (two partial arrays of 128 groups, room for a third, and behind them the
// two-word staging slot of the all-reduce)
int two_squared_norms(femshell_ctx *c, const double *a, const double *b, int64_t n6, double sums[2])
{
    hipStream_t st = c->stream;
    constexpr size_t kDotsStage = 3 * 128;
    FS_HIP(c->dots_scratch.alloc(kDotsStage + 2));
    const int groups = launch_two_dots(a, a, b, b, n6, c->dots_scratch.p, st);
    double hp[2 * 128];
    FS_HIP(hipMemcpyAsync(hp, c->dots_scratch.p, sizeof hp, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    sums[0] = sums[1] = 0.0;
    for (int g = 0; g < groups; g++) {
        sums[0] += hp[g];
        sums[1] += hp[128 + g];
    }
    if (c->comm.active()) { // every rank holds its own rows
        FS_HIP(hipMemcpyAsync(c->dots_scratch.p + kDotsStage, sums, 2 * sizeof(double), hipMemcpyHostToDevice, st));
        std::string e;
        if (!comm_allreduce_sum(c->comm, c->dots_scratch.p + kDotsStage, 2, st, &e)) return set_err(FEMSHELL_ERR_COMM, e);
        FS_HIP(hipMemcpyAsync(sums, c->dots_scratch.p + kDotsStage, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
    }
    return FEMSHELL_OK;
}
static int squared_norm(femshell_ctx *c, const double *a, int64_t n6, double *out)
{
    double sums[2];
    const int rc = two_squared_norms(c, a, a, n6, sums);
    *out = sums[0];
    return rc;
}

// Flexible preconditioned CG (beta = z.(r - r_old) / r_old.z_old, so that the K cycle's slightly varying operator
// does not break the recurrence); stopping rule and scalars as in cg_classic.
//
// Iterative refinement: on the thin-shell systems ||K|| ||x|| exceeds ||b|| by seven to nine orders of magnitude.
// Every product K p then carries rounding noise of eps ||K|| ||p||, part of which falls on the soft modes: the
// displacement error against a direct solve stalls at 2e-10 on the 250k-triangle roof however far the recurrence
// residual is driven.  After the recurrence has converged the residual of the iterate is therefore evaluated in
// double-double (k_residual_dd; in plain FP64 it is noise itself, and restarting from it made the error worse:
// 2e-10 -> 2e-9) and the correction equation K e = b - K x is solved by the same method from e = 0 in a vector of
// its own -- there the noise scales with ||e||, not ||x|| -- and added once: x += e.  (Continuing the recurrence on
// x itself does not help: every update x += alpha p rounds at eps ||x||.)  Measured on the roof: 2e-10 -> 2e-13
// with one pass.  femshell_pc_options::refine_passes passes at most (default 1; 0 = off).  A pass stops on the drop of its
// own right-hand side, whatever the residual tolerance of the solve: ||e|| / ||x|| of the pass is the displacement error of
// the iterate before it (manufactured solutions at 4M triangles: 4.8e-8 estimated, 4.8e-8 true) and the pass leaves about
// that times its drop -- it runs until that product, with the ||e_k|| so far, is a fifth of rtol (cg_kernels.hip: kRefineTarget;
// 1e-4 flat with FEMSHELL_REFINE_ADAPTIVE=0); passes after the first run while the product exceeds rtol.
// *true_rr_out = ||b - K x||^2 (double-double) of the returned iterate.
int cg_amg(femshell_ctx *c, const CgVectors &v0, double rtol, int32_t max_it, double *true_rr_out, double *rec_rr_out, const double *x0)
{
    const DeviceMatrix &m = c->dm;
    hipStream_t st = c->stream;
    const int64_t n6 = 6ll * m.n_pad;
    *true_rr_out = -1.0;
    *rec_rr_out = -1.0;
    const int refine = c->amg->opt.refine_passes;
    // With a refinement pass to follow, the first phase stops a factor 100 = 1 / sqrt(drop of a pass) above the tolerance:
    // what the tolerance is for is the displacement error, the pass reduces the error of the iterate it starts from by
    // its drop whatever that iterate is, and the digits the recurrence adds beyond 100 rtol are the ones its rounding noise
    // spoils anyway (manufactured solutions at 4M triangles, first phase to 1e-10 / 1e-8: 99 / 76 iterations, error 2e-14 /
    // 1e-12 on the panel; 86 / 70 iterations, 2e-13 / 2e-11 on the cylinder; to 1e-7 the cylinder's error is 1.3e-10).
    // Should the estimate of the first pass still exceed the tolerance, one pass more than refine_passes may run.
    const bool loosened = refine >= 1 && rtol > 0.0;
    const double rtol_first = loosened ? std::min(100.0 * rtol, 1e-2) : rtol;
    const int pass_limit = refine + (loosened ? 1 : 0);
    // FEMSHELL_REFINE_ADAPTIVE=0: every pass to a drop of 1e-4 of its own right-hand side, as before round 5 (A/B runs)
    const bool adaptive_pass = knob_flag("FEMSHELL_REFINE_ADAPTIVE", true);
    CgVectors v = v0;
    CgScalars hs{};
    double pass_host[3] = {0.0, 0.0, 0.0}; // source of an asynchronous copy below: lives until the function's next synchronisation
    int32_t it = 0;
    c->refine = femshell_ctx::RefineStats();
    double pass_rhs_rr = 0.0; // ||rhs||^2 of the running refinement pass
    for (int pass = 0;; pass++) {
        int rc;
        if (pass == 0) {
            launch_pcg_init(m, v, st);
            rc = scalar_step(c, v, 1, CG_PHASE_FLEX_INIT, rtol_first);
            if (rc) return rc;
            if (x0 != nullptr) {
                // A solve from an initial guess (femshell_set_initial_guess): x0 becomes the accumulated iterate and the first phase
                // solves the correction equation K e = b - K x0 -- its right-hand side evaluated in double-double, as a refinement
                // pass's -- down to the threshold the step above derived from b.  What follows is the solve from zero: x0 + e takes
                // the place of the first phase's iterate, the refinement passes correct it.
                FS_HIP(c->xacc.alloc((size_t)n6 + 6 * (size_t)m.n_ghost));
                FS_HIP(c->xacc.zero(st));
                FS_HIP(c->rres.alloc((size_t)n6));
                launch_copy(x0, c->xacc.p, n6, nullptr, st);
                rc = halo_exchange(c, c->xacc.p, st);
                if (rc) return rc;
                launch_residual_dd(m, c->xacc.p, v0.b, c->rres.p, st);
                v.b = c->rres.p;
                launch_pcg_init(m, v, st); // x = 0, r = b - K x0, partial sums of r.r
                rc = scalar_step(c, v, 1, CG_PHASE_FLEX_WARM, rtol_first);
                if (rc) return rc;
            }
        } else {
            // correction equation: right-hand side = residual of the accumulated solution, evaluated in double-double
            TraceRange trace("femshell refinement pass: double-double residual");
            rc = halo_exchange(c, c->xacc.p, st); // no-op without a communicator
            if (rc) return rc;
            launch_residual_dd(m, c->xacc.p, v0.b, c->rres.p, st);
            v.b = c->rres.p;
            if (adaptive_pass) {
                // ||x||^2 of the iterate this pass corrects, for the pass's own stopping rule (cg_kernels.hip: kRefineTarget)
                double xx = 0.0;
                rc = squared_norm(c, c->xacc.p, n6, &xx);
                if (rc) return rc;
                pass_host[0] = xx;
                pass_host[1] = 0.0;
                pass_host[2] = rtol;
                FS_HIP(hipMemcpyAsync(reinterpret_cast<char *>(v.s) + offsetof(CgScalars, pass_xx), pass_host, sizeof pass_host, hipMemcpyHostToDevice, st));
            }
            launch_pcg_init(m, v, st); // x = 0, r = rhs, partial sums of r.r
            // (rtol = 0: the pass stops on the relative drop kRefineDrop of its own right-hand side alone -- the residual
            //  tolerance of the solve says little about the displacement error on these systems: at 4M triangles a
            //  manufactured solution is 4e-9 off at a double-double residual of 8.7e-11 ||b||, and under uniform pressure
            //  the double-double residual of a converged iterate is 5.6e-5 ||b||, rounding noise of K x)
            rc = scalar_step(c, v, 1, CG_PHASE_FLEX_RESTART, 0.0);
            if (rc) return rc;
            FS_HIP(hipMemcpyAsync(&hs, v.s, sizeof hs, hipMemcpyDeviceToHost, st));
            FS_HIP(hipStreamSynchronize(st));
            *true_rr_out = hs.rr;
            pass_rhs_rr = hs.rr;
            // passes beyond the first run only while the error estimate of the previous one is above the tolerance
            const bool accurate = pass >= 2 && c->refine.correction_rel * c->refine.residual_reduction <= rtol;
            if (hs.done != 0 || pass > pass_limit || it >= max_it || accurate) {
                const int32_t one = 1; // the solve as a whole has converged
                FS_HIP(hipMemcpyAsync(reinterpret_cast<char *>(v.s) + offsetof(CgScalars, done), &one, sizeof one, hipMemcpyHostToDevice, st));
                launch_copy(c->xacc.p, v.x, n6, nullptr, st);
                FS_HIP(hipStreamSynchronize(st));
                return FEMSHELL_OK;
            }
        }
        rc = amg_apply(c, v.r, v.z, v.s);
        if (rc) return rc;
        launch_pcg_dots(m, v, st);
        rc = scalar_step(c, v, 1, CG_PHASE_FLEX_RZ0, rtol);
        if (rc) return rc;
        launch_copy(v.z, v.p, n6, v.s, st);
        AmgPoll poll;
        poll.next_check = it + 1;
        bool finished = false;
        // FEMSHELL_AMG_FUSE bit 0: the update kernel also finishes q = K p (second phase of the symmetric-storage product) and
        // takes the first step of the cycle's pre-smoothing on the new residual (k_pcg_update_start_node: three passes become one)
        AmgLevel &L0 = *c->amg->levels[0];
        const bool fused_update = (fuse_mask() & 1) != 0 && c->amg->levels.size() > 1;
        const DeviceMatrix &S0 = L0.smooth_ready ? L0.smooth_dm : m;
        const bool d32_0 = S0.symmetric && has_lowp(S0) && S0.vec32 == 2;
        for (; it < max_it; it++) {
            int n_partials = 0;
            const bool defer = fused_update && m.symmetric != 0;
            if (c->comm.active()) rc = spmv_with_halo(c, v, v.p, v.q, v.partials, &n_partials, defer);
            else if (defer) launch_spmv_sym_phase1(m, v.p, v.q, v.partials, v.s, st);
            else launch_spmv(m, v.p, v.q, SpmvEpilogue(), v.s, st, SpmvSpan(), v.partials);
            if (rc) return rc;
            rc = scalar_step(c, v, 1, CG_PHASE_ALPHA, rtol, n_partials);
            if (rc) return rc;
            if (fused_update) launch_pcg_update_start(S0, v, L0.d.p, amg_apply_iterate(c, v.z), L0.inv_theta, defer, d32_0, st);
            else launch_pcg_update(m, v, st);
            rc = scalar_step(c, v, 2, CG_PHASE_FLEX_CONV, rtol); // (r.r and, for the stopping rule of a refinement pass, x.x)
            if (rc) return rc;
            rc = amg_apply(c, v.r, v.z, v.s, fused_update);
            if (rc) return rc;
            launch_pcg_dots(m, v, st);
            rc = scalar_step(c, v, 2, CG_PHASE_FLEX_BETA, rtol);
            if (rc) return rc;
            launch_cg_direction(m, v, st);
            rc = poll(c, v, it, max_it, &hs);
            if (rc < 0) return rc;
            if (rc == 1) {
                finished = true;
                break;
            }
        }
        if (!finished) {
            FS_HIP(hipMemcpyAsync(&hs, v.s, sizeof hs, hipMemcpyDeviceToHost, st));
            FS_HIP(hipStreamSynchronize(st));
        }
        it = hs.iters;
        if (pass == 0 && x0 != nullptr) {
            // the iterate of the first phase is x0 + e, whatever ended the phase
            launch_add(v.x, c->xacc.p, n6, st);
            launch_copy(c->xacc.p, v.x, n6, nullptr, st);
            v.b = v0.b;
        }
        if (pass == 0) *rec_rr_out = hs.rr; // what the stopping rule of the first phase saw (a refinement pass stops on
                                            // the drop of its own right-hand side, see CG_PHASE_FLEX_RESTART)
        if (pass > 0) {
            // error estimate of the solve: ||e|| / ||x|| of this pass (the error of the iterate before it) and the factor
            // by which the pass reduced the residual of its correction equation
            double sums[2];
            rc = two_squared_norms(c, v.x, c->xacc.p, n6, sums);
            if (rc) return rc;
            c->refine.passes = pass;
            c->refine.correction_rel = sums[1] > 0.0 ? std::sqrt(sums[0] / sums[1]) : 0.0;
            c->refine.residual_reduction = pass_rhs_rr > 0.0 ? std::sqrt(hs.rr / pass_rhs_rr) : 0.0;
            // x += e; the context's x is the accumulated solution again
            launch_add(v.x, c->xacc.p, n6, st);
            launch_copy(c->xacc.p, v.x, n6, nullptr, st);
        }
        if (hs.done != 1 || rtol <= 0.0) return FEMSHELL_OK; // iteration limit or breakdown: no refinement
        if (pass == 0) {
            FS_HIP(c->xacc.alloc((size_t)n6 + 6 * (size_t)m.n_ghost)); // ghost space: input of the double-double residual
            FS_HIP(c->xacc.zero(st));
            FS_HIP(c->rres.alloc((size_t)n6));
            launch_copy(v.x, c->xacc.p, n6, nullptr, st);
        }
    }
    return FEMSHELL_OK;
}

// Algorithmic HBM bytes of one multigrid cycle, level by level (per_level[l]: everything the cycle does ON level l over all its
// visits per outer iteration: smoothing products and steps, the two residual increments, the transfers to and from level l+1,
// the K cycle's own products and vector passes; the dense solve on the coarsest level).  Counted is what the kernels have to
// stream as the cycle is built today (round 5) -- NOT 292 B per block for every product as rounds 2-4 counted:
//   * a smoothing product or a residual increment reads the smoother's copy of the operator: 148 B per stored block where the
//     level keeps the single-precision copy (144 B of values + 4 B column index), 292 B else; symmetric storage stores (and streams)
//     the diagonal and one block per pair; its input and output vectors are floats where DeviceMatrix::vec32 says so
//   * the K cycle's two products per coarse solve and nothing else of the cycle read the FP64 operator
//   * the transposed-product buffers of symmetric storage are overhead of the method and are not counted (as for bytes_spmv)
//   * vector passes: every vector a kernel reads or writes once, 48 B per node (24 B as floats), the block-Jacobi inverse 168 B
//     per node (84 B from its single-precision copy)
double amg_cycle_bytes(const femshell_ctx *c, std::vector<double> *per_level)
{
    const Amg &H = *c->amg;
    const size_t nl = H.levels.size();
    std::vector<double> visits(nl, 0.0), bytes(nl, 0.0);
    visits[0] = 1.0;
    const bool kcyc = H.opt.cycle == FEMSHELL_CYCLE_K;
    for (size_t l = 0; l + 1 < nl; l++) {
        const AmgLevel &L = *H.levels[l], &N = *H.levels[l + 1];
        const DeviceMatrix &A = amg_level_matrix(c, (int)l);
        const double n = (double)L.n;
        const bool lowp = L.A32.p != nullptr;
        const int v32 = (A.symmetric && lowp) ? L.smooth_dm.vec32 : 0;
        // blocks a product of the level operator streams (symmetric storage: the stored ones)
        const double blocks = l == 0 ? (double)c->plan.stored_blocks : (A.symmetric ? 0.5 * ((double)L.nnzb + n) : (double)L.nnzb);
        const double deg = (double)L.cheb_a.size() + 1.0;
        const double vec = 48.0 * n, fvec = 24.0 * n;
        const double minv = (lowp ? 84.0 : 168.0) * n;
        const double in_vec = v32 == 2 ? fvec : vec, out_vec = v32 >= 1 ? fvec : vec;
        const double smooth_product = blocks * (lowp ? 148.0 : 292.0) + in_vec + out_vec;
        // per visit: 2 (deg - 1) products inside the two smoothings + the two increments
        double per_visit = 2.0 * deg * smooth_product;
        // Chebyshev steps (2 (deg - 1)): rin, q, d, x, D^-1 read; rout, d, x written
        per_visit += 2.0 * (deg - 1.0) * (vec + out_vec + in_vec + vec + minv + vec + in_vec + vec);
        // the two starts: r, D^-1 (and x behind the coarse correction) read; d, x written -- and the two second phases / axpys
        // of the increments: product and base vector read, residual written
        per_visit += 2.0 * (vec + minv + in_vec + vec) + vec + 2.0 * (out_vec + vec + vec);
        // transfers: R (rows of level l+1) and P (rows of level l), single-precision copies where the setup made them
        const double rp_block = L.P32.p != nullptr ? 148.0 : 292.0;
        // (the prolongation is a product over the rows of this level; the restriction one over the rows of the next and is booked
        //  there -- which is also where a kernel trace by grid size finds it, tools/amg_level_times.py)
        per_visit += rp_block * (double)L.P.nnzb + (48.0 * N.n + 2.0 * vec + in_vec);
        bytes[l + 1] += visits[l] * (rp_block * (double)L.R.nnzb + vec + 48.0 * N.n);
        // the K cycle on this level (levels >= 1 that are not the coarsest): per coarse solve = per two visits, two FP64 products
        // and the vector passes of the two coefficient steps
        if (kcyc && l >= 1) per_visit += 0.5 * (2.0 * (292.0 * blocks + 2.0 * vec) + 14.0 * vec);
        bytes[l] += visits[l] * per_visit;
        const bool next_k = kcyc && l + 2 < nl;
        visits[l + 1] = visits[l] * (next_k ? 2.0 : 1.0);
    }
    const AmgLevel &C = *H.levels.back();
    bytes[nl - 1] += visits.back() * ((H.coarse_inv32.p != nullptr ? 4.0 : 8.0) * 36.0 * (double)C.n * (double)C.n + 96.0 * C.n);
    double total = 0.0;
    for (double b : bytes) total += b;
    if (per_level != nullptr) *per_level = bytes;
    return total;
}

} // namespace femshell
