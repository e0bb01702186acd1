// node_io.hpp -- node-indexed data across the library's boundary.  A context created with FEMSHELL_REORDER_MORTON / _RCM numbers the
// nodes anew inside the library (c->perm, c->iperm: context.hpp); the caller never sees that numbering.  Every node id and node
// vector that enters or leaves the C ABI crosses it here, and nowhere else.
#pragma once

#include "context.hpp"

#pragma GCC visibility push(hidden)
namespace femshell {

// the internal id of the caller's node a; -1: a is not a node of the mesh
int32_t internal_node(const femshell_ctx *c, int32_t a);
// the caller's id of internal node i (i itself where it is no node of the mesh: messages about a node print what they have)
int32_t caller_node(const femshell_ctx *c, int32_t i);

// What a host vector holds: n_nodes x 6 in the caller's numbering, or the rank's owned rows, n_own x 6, as they lie in HBM
// (femshell_pc_apply on a row partition; vectors a caller of this module has put into the internal order itself).
enum class NodeOrder { caller, internal };

// n_cols host columns X -> the block at dst in HBM (column j at dst + j * ld): the owned rows in the internal order, everything
// from 6 n_own up to ld zero.  Enqueued on c->stream, not synchronised: *stage holds the reordered copy where one is needed (never
// for NodeOrder::internal, where it may be null) and, like X, has to outlive the next synchronisation of the stream.
int upload_node_block(femshell_ctx *c, NodeOrder order, int32_t n_cols, const double *X, double *dst, size_t ld, std::vector<double> *stage);

// ... and back: the owned rows of n_cols columns in HBM (column j at src + j * ld) -> the host columns Y.  Synchronises c->stream, once.
int download_node_block(femshell_ctx *c, NodeOrder order, int32_t n_cols, const double *src, size_t ld, double *Y);

// a vector of the owned rows in HBM as n_nodes x 6 in the caller's numbering, whole on every rank (collective on a row partition)
int gather_node_vector(femshell_ctx *c, const double *owned, double *u_out);

} // namespace femshell
#pragma GCC visibility pop
