// The graph part of the relation net for the pages of ONE call (asep_gnn_forward_batch[_dev]): each stage one launch over all pages.
//
// The pages lie one behind the other: page b's nodes are the nodes node_off .. node_off + N_b - 1 of the call, as in the reference's own batched
// graph (graph_gnn.py:189-196: node id += b * max_nodes).  Two kinds of stage follow from that:
//
//   * per page, through the page table (gnn_page_table.h; a block belongs to exactly one page and finds it with page_of_unit): what depends on a
//     page's own sizes -- the dense N_b x N_b edge table of the correction (fill, count, emit: one table per page inside one allocation), the
//     interaction chunks of the attention pairing (chunks of 100000 / N_b targets), the pair classifier (Pt / Qt are [h1][N_b] per page, the
//     relations name page-local nodes).  The kernels below; their bodies are the single-page kernels' (gnn_kernels.h), called with the page's
//     pointers and its block number.
//   * over the nodes of the call, with the single-page kernels themselves: the correction leaves ONE CSR-by-target over all nodes (the scan runs
//     over the call's counts, so page b's in-edges follow page b - 1's; inside a page the order is the page's own, ascending edge code), source
//     nodes numbered in the call, edge-feature rows numbered in the call.  A target's block of the step / message / soft-max / aggregation / LSTM
//     kernels then reads only its own page's rows: the same operations in the same order as on the page alone, whatever else shares the launch.
#pragma once
#include "gnn_kernels.h"
#include "gnn_page_table.h"

namespace asep {

struct GnnPagesArgs {
    const GnnPageRow* rows;       // [n]
    const int32_t* begin;         // [n + 1] the launch's unit table (per-node launches: node_begin)
    int n;
};

// edge_table_kernel per page: page b owns min(ceil(fed entries / 256), 2048) blocks, the single launcher's grid
__global__ __launch_bounds__(256) void edge_table_pages_kernel(const GnnPagesArgs t, const int32_t* __restrict__ edges, int undirected,
                                                               int* __restrict__ table) {
    const int b = page_of_unit(t.begin, t.n, (int)blockIdx.x);
    const GnnPageRow r = t.rows[b];
    const int b0 = t.begin[b];
    edge_table_body(edges + 2 * (size_t)r.edge_off, r.E, r.N, undirected, table + r.table_off, (int)blockIdx.x - b0, t.begin[b + 1] - b0);
}

// edge_count_kernel: one wave per node of the call; counts land at the node's place in the call
__global__ __launch_bounds__(64) void edge_count_pages_kernel(const GnnPagesArgs t, const int* __restrict__ table, int* __restrict__ rowcnt,
                                                              int* __restrict__ colcnt) {
    const int b = page_of_unit(t.begin, t.n, (int)blockIdx.x);
    const GnnPageRow r = t.rows[b];
    edge_count_body(table + r.table_off, r.N, rowcnt + r.node_off, colcnt + r.node_off, (int)blockIdx.x - r.node_off);
}

// edge_emit_kernel: one wave per node of the call (rowptr / colptr: the scans over the call's counts)
__global__ __launch_bounds__(64) void edge_emit_pages_kernel(const GnnPagesArgs t, const int* __restrict__ table, const int* __restrict__ rowptr,
                                                             const int* __restrict__ colptr, int32_t* __restrict__ sorted_edges,
                                                             int* __restrict__ sorted_first, int* __restrict__ tsrc, int* __restrict__ tfirst) {
    const int b = page_of_unit(t.begin, t.n, (int)blockIdx.x);
    const GnnPageRow r = t.rows[b];
    edge_emit_body<true>(table + r.table_off, r.N, rowptr + r.node_off, colptr + r.node_off, sorted_edges, sorted_first, tsrc, tfirst,
                         (int)blockIdx.x - r.node_off, r.node_off, r.edge_off, max(r.E, 1));
}

// edge_chunk_rank_kernel: a block per (page, interaction chunk); it scans its page's part of the (from, to)-sorted list
__global__ __launch_bounds__(256) void edge_chunk_rank_pages_kernel(const GnnPagesArgs t, const int32_t* __restrict__ sorted_edges,
                                                                    const int* __restrict__ rowptr, const int* __restrict__ colptr,
                                                                    int* __restrict__ widx) {
    const int b = page_of_unit(t.begin, t.n, (int)blockIdx.x);
    const GnnPageRow r = t.rows[b];
    const int c = (int)blockIdx.x - t.begin[b];
    const int lo = r.node_off + c * r.chunk_nodes, hi = min(r.node_off + r.N, lo + r.chunk_nodes);
    edge_chunk_rank_body(sorted_edges, colptr, rowptr[r.node_off], rowptr[r.node_off + r.N], lo, hi, widx);
}

// gnn_pair_pre_kernel per page: Pt / Qt of page b are [h1][N_b] at h1 * node_off
__global__ __launch_bounds__(256) void gnn_pair_pre_pages_kernel(const GnnPagesArgs t, const float* __restrict__ h, int H,
                                                                 const float* __restrict__ W1, int H1, float* __restrict__ Pt,
                                                                 float* __restrict__ Qt) {
    const int b = page_of_unit(t.begin, t.n, (int)blockIdx.x);
    const GnnPageRow r = t.rows[b];
    const int b0 = t.begin[b];
    gnn_pair_pre_body(h + (size_t)r.node_off * H, r.N, H, W1, H1, Pt + (size_t)r.node_off * H1, Qt + (size_t)r.node_off * H1,
                      (int)blockIdx.x - b0, t.begin[b + 1] - b0);
}

template <int H1, int H2, int NC>
__global__ __launch_bounds__(256) void gnn_pair_cls_pages_kernel(const GnnPagesArgs t, PairArgs a) {
    const int b = page_of_unit(t.begin, t.n, (int)blockIdx.x);
    const GnnPageRow r = t.rows[b];
    const int b0 = t.begin[b];
    a.Pt += (size_t)r.node_off * H1; a.Qt += (size_t)r.node_off * H1;      // (`a` holds the call's buffers and the weights)
    if (a.rel) a.rel += 2 * (size_t)r.rel_off;
    a.out += (size_t)r.rel_off * NC;
    a.N = r.N; a.R = r.R;
    gnn_pair_cls_kernel_body<H1, H2, NC>(a, (int)blockIdx.x - b0, t.begin[b + 1] - b0);
}
__global__ __launch_bounds__(256) void gnn_pair_cls_generic_pages_kernel(const GnnPagesArgs t, const PairGenArgs a) {
    const int b = page_of_unit(t.begin, t.n, (int)blockIdx.x);
    const GnnPageRow r = t.rows[b];
    const int H1 = a.rest.dims[0], NC = a.rest.dims[a.rest.nl];
    gnn_pair_cls_generic_body(a, a.Pt + (size_t)r.node_off * H1, a.Qt + (size_t)r.node_off * H1, a.rel ? a.rel + 2 * (size_t)r.rel_off : nullptr,
                              a.out + (size_t)r.rel_off * NC, r.N, r.R, (int)blockIdx.x - t.begin[b]);
}

// the call's output: column `cls` of the classifier's [R, NC] probabilities (a copy: the values are the classifier's)
__global__ __launch_bounds__(256) void gnn_take_class_kernel(const float* __restrict__ probs, int R, int NC, int cls, float* __restrict__ out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < R) out[r] = probs[(size_t)r * NC + cls];
}

}  // namespace asep
