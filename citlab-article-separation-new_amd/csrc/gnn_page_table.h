// The page table of asep_gnn_forward_batch[_dev] (the graph part of the relation net for the pages of one call), in plain C++17: no HIP, no
// device types, nothing of the engine, so that a host program can check it (tests/gnn_page_table_check.cpp).
//
// The pages of a call lie one behind the other in every buffer: nodes, fed edges, relations and the dense edge tables of the correction
// (page b's N_b x N_b cells start at table_off).  A row says where a page's part starts; the sums are refused before anything is launched
// where an index of the kernels would not fit 31 bits or the tables would not fit the allocation a single page may ask for.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "launch_plan.h"

namespace asep {

struct GnnPageRow {
    int32_t node_off, N;        // the page's nodes: node_off .. node_off + N - 1 of the call
    int32_t edge_off, E;        // its fed edges (rows of the edge list and of the edge features)
    int32_t rel_off, R;         // its relations (rows of the relation list and of the output)
    int32_t table_off;          // first cell of its N x N edge table
    int32_t chunk_nodes;        // message_fn_chunk.py:77-78: target nodes per interaction chunk, max(1, 100000 / N)
};

constexpr uint64_t GNN_TABLE_CELLS_MAX = (uint64_t)1 << 30;     // N_b^2 of a page, and the sum over the pages of a call
constexpr uint64_t GNN_BATCH_INDEX_MAX = (uint64_t)INT32_MAX;

enum GnnTableError {
    GNN_TABLE_OK = 0,
    GNN_TABLE_BAD_N,            // N_b < 1
    GNN_TABLE_BAD_E,            // E_b < 0
    GNN_TABLE_BAD_R,            // R_b < 0
    GNN_TABLE_PAGE_TOO_LARGE,   // N_b^2 > 2^30
    GNN_TABLE_SUM_TABLES,       // the summed edge tables do not fit 2^30 cells
    GNN_TABLE_SUM_INDEX,        // a summed index (nodes x row width, corrected edges, relations x classes) does not fit 31 bits
};

struct GnnPageTable {
    std::vector<GnnPageRow> rows;
    std::vector<int32_t> node_begin;    // [n + 1]: node_off of every page, then the node count of the call (the per-node kernels' unit table)
    uint64_t nodes = 0, edges = 0, rels = 0, cells = 0;
    uint64_t max_corrected = 0;         // sum of (undirected ? 2 : 1) * max(E_b, 1): what the corrected lists can hold
};

// rows and sums for n pages; `row_width` = the widest row a kernel indexes with node * width or relation * width (in floats).
// On an error *bad_page names the page (the sum errors: the page at which the sum first overflows) and the table is not to be used.
inline GnnTableError gnn_page_table(const int32_t* N, const int32_t* E, const int32_t* R, int n, bool undirected, int row_width,
                                    GnnPageTable& t, int* bad_page) {
    t = GnnPageTable{};
    t.rows.reserve((size_t)std::max(n, 0));
    t.node_begin.assign((size_t)std::max(n, 0) + 1, 0);
    const uint64_t width = (uint64_t)std::max(row_width, 1);
    for (int b = 0; b < n; ++b) {
        *bad_page = b;
        if (N[b] < 1) return GNN_TABLE_BAD_N;
        if (E[b] < 0) return GNN_TABLE_BAD_E;
        if (R[b] < 0) return GNN_TABLE_BAD_R;
        const uint64_t cells = (uint64_t)N[b] * (uint64_t)N[b];
        if (cells > GNN_TABLE_CELLS_MAX) return GNN_TABLE_PAGE_TOO_LARGE;
        if (t.cells + cells > GNN_TABLE_CELLS_MAX) return GNN_TABLE_SUM_TABLES;
        const uint64_t corrected = (uint64_t)(undirected ? 2 : 1) * (uint64_t)std::max(E[b], 1);
        if ((t.nodes + (uint64_t)N[b]) * width > GNN_BATCH_INDEX_MAX || (t.max_corrected + corrected) * width > GNN_BATCH_INDEX_MAX ||
            (t.rels + (uint64_t)R[b]) * width > GNN_BATCH_INDEX_MAX || (t.edges + (uint64_t)E[b]) * width > GNN_BATCH_INDEX_MAX)
            return GNN_TABLE_SUM_INDEX;
        GnnPageRow r{};
        r.node_off = (int32_t)t.nodes; r.N = N[b];
        r.edge_off = (int32_t)t.edges; r.E = E[b];
        r.rel_off = (int32_t)t.rels; r.R = R[b];
        r.table_off = (int32_t)t.cells;
        r.chunk_nodes = std::max(1, 100000 / N[b]);
        t.rows.push_back(r);
        t.nodes += (uint64_t)N[b]; t.edges += (uint64_t)E[b]; t.rels += (uint64_t)R[b]; t.cells += cells; t.max_corrected += corrected;
        t.node_begin[(size_t)b + 1] = (int32_t)t.nodes;
    }
    *bad_page = -1;
    return GNN_TABLE_OK;
}

// The unit tables of the launches whose blocks are not one per node (launch_plan.h page_unit_table: page b owns the units begin[b] ..
// begin[b + 1] - 1).  Per page the counts are the single-page launchers' grids:
//   fill    edge_table_kernel      min(ceil(fed entries / 256), 2048) blocks, fed entries = (undirected ? 2 : 1) * E_b
//   chunk   edge_chunk_rank_kernel ceil(N_b / chunk_nodes) blocks
//   pre     gnn_pair_pre_kernel    min(ceil(N_b * h1 / 256), 1024) blocks
//   cls     the pair classifier    ceil(R_b / pairs_per_block) blocks
struct GnnUnitTables { std::vector<int32_t> fill, chunk, pre, cls; };
inline bool gnn_unit_tables(const GnnPageTable& t, bool undirected, int cls_hidden1, int pairs_per_block, GnnUnitTables& u) {
    const int n = (int)t.rows.size();
    std::vector<size_t> fill((size_t)n), chunk((size_t)n), pre((size_t)n), cls((size_t)n);
    for (int b = 0; b < n; ++b) {
        const GnnPageRow& r = t.rows[(size_t)b];
        const size_t fed = (size_t)(undirected ? 2 : 1) * (size_t)r.E;
        fill[(size_t)b] = std::min<size_t>((fed + 255) / 256, 2048);
        chunk[(size_t)b] = ((size_t)r.N + (size_t)r.chunk_nodes - 1) / (size_t)r.chunk_nodes;
        pre[(size_t)b] = std::min<size_t>(((size_t)r.N * (size_t)cls_hidden1 + 255) / 256, 1024);
        cls[(size_t)b] = ((size_t)r.R + (size_t)pairs_per_block - 1) / (size_t)pairs_per_block;
    }
    return page_unit_table(fill.data(), n, 1, u.fill) && page_unit_table(chunk.data(), n, 1, u.chunk) &&
           page_unit_table(pre.data(), n, 1, u.pre) && page_unit_table(cls.data(), n, 1, u.cls);
}

}  // namespace asep
