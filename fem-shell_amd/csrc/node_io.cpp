// node_io.cpp -- see node_io.hpp.  The only code that indexes c->perm / c->iperm besides femshell_set_mesh, which builds them, and
// femshell_export_bsr, which relabels a matrix (and the F it downloads beside it, under the same synchronisation).
#include "node_io.hpp"

#include <cstring>

#include "amg.hpp" // parallel_chunks

namespace femshell {

int32_t internal_node(const femshell_ctx *c, int32_t a)
{
    if (a < 0 || a >= c->plan.n_nodes) return -1;
    return c->iperm.empty() ? a : c->iperm[(size_t)a];
}

int32_t caller_node(const femshell_ctx *c, int32_t i)
{
    return (i >= 0 && i < (int32_t)c->perm.size()) ? c->perm[(size_t)i] : i;
}

int upload_node_block(femshell_ctx *c, NodeOrder order, int32_t n_cols, const double *X, double *dst, size_t ld, std::vector<double> *stage)
{
    const Plan &p = c->plan;
    const size_t n6 = (size_t)p.n_own * 6;
    const bool caller = order == NodeOrder::caller, reorder = caller && !c->perm.empty();
    const size_t ldx = caller ? (size_t)p.n_nodes * 6 : n6;
    FS_HIP(hipMemsetAsync(dst, 0, (size_t)n_cols * ld * sizeof(double), c->stream));
    if (n6 == 0) return FEMSHELL_OK;
    if (reorder) {
        stage->resize((size_t)n_cols * n6);
        for (int32_t j = 0; j < n_cols; j++)
            for (int32_t i = 0; i < p.n_own; i++)
                std::memcpy(&(*stage)[(size_t)j * n6 + 6ull * (size_t)i], X + (size_t)j * ldx + 6ull * (size_t)c->perm[(size_t)(p.row_begin + i)], 6 * sizeof(double));
    }
    for (int32_t j = 0; j < n_cols; j++) {
        // (without a renumbering the owned rows are one contiguous piece of the caller's column)
        const double *xj = reorder ? stage->data() + (size_t)j * n6 : X + (size_t)j * ldx + (caller ? 6ull * (size_t)p.row_begin : 0);
        FS_HIP(hipMemcpyAsync(dst + (size_t)j * ld, xj, n6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    return FEMSHELL_OK;
}

// rows [first, first + n_rows) of the internal numbering, n_cols columns of them in HBM -> the host; to_caller: column j goes to
// Y + j * ldy, every row to the place of the caller's id of its node, else the rows as they lie to Y + j * ldy.  One synchronisation.
static int fetch_rows(femshell_ctx *c, bool to_caller, int32_t first, int32_t n_rows, int32_t n_cols, const double *src, size_t ld, double *Y, size_t ldy)
{
    const size_t n6 = (size_t)n_rows * 6;
    const bool reorder = to_caller && !c->perm.empty();
    std::vector<double> h(reorder ? (size_t)n_cols * n6 : 0); // internal numbering -> the caller's
    for (int32_t j = 0; j < n_cols && n6 > 0; j++) {
        double *yj = reorder ? h.data() + (size_t)j * n6 : Y + (size_t)j * ldy + (to_caller ? 6ull * (size_t)first : 0);
        FS_HIP(hipMemcpyAsync(yj, src + (size_t)j * ld, n6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    FS_HIP(hipStreamSynchronize(c->stream));
    if (reorder)
        parallel_chunks((int64_t)n_cols * n_rows, [&](int64_t b, int64_t e) {
            for (int64_t q = b; q < e; q++) {
                const int64_t j = q / n_rows, i = q % n_rows;
                std::memcpy(Y + (size_t)j * ldy + 6ull * (size_t)c->perm[(size_t)(first + i)], &h[(size_t)j * n6 + 6ull * (size_t)i], 6 * sizeof(double));
            }
        }, 1 << 16);
    return FEMSHELL_OK;
}

int download_node_block(femshell_ctx *c, NodeOrder order, int32_t n_cols, const double *src, size_t ld, double *Y)
{
    const Plan &p = c->plan;
    const bool caller = order == NodeOrder::caller;
    return fetch_rows(c, caller, p.row_begin, p.n_own, n_cols, src, ld, Y, (size_t)(caller ? p.n_nodes : p.n_own) * 6);
}

int gather_node_vector(femshell_ctx *c, const double *owned, double *u_out)
{
    if (!c->comm.active()) return download_node_block(c, NodeOrder::caller, 1, owned, 0, u_out);
    const Plan &p = c->plan;
    FS_HIP(c->ufull.alloc((size_t)p.n_nodes * 6));
    std::string e;
    if (!comm_gather_rows(c->comm, owned, c->ufull.p, c->all_begin, c->all_end, c->stream, &e))
        return set_err(FEMSHELL_ERR_COMM, e);
    return fetch_rows(c, true, 0, p.n_nodes, 1, c->ufull.p, 0, u_out, 0);
}

} // namespace femshell
