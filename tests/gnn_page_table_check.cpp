// Host check of csrc/gnn_page_table.h (the page table and the unit tables of asep_gnn_forward_batch) against brute-force restatements.  Plain C++17,
// no HIP: tests/test_gnn_graph_batch_host.py builds it with the host compiler under the address and undefined-behaviour sanitizers.  Called as
// `check undirected row_width cls_hidden1 pairs_per_block N0 E0 R0 N1 E1 R1 ...` it prints the tables of those pages for the numpy restatement of
// the test (or `refused <code> <page>`).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gnn_page_table.h"

using namespace asep;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static void print_vec(const char* name, const std::vector<int32_t>& v) {
    std::printf("%s", name);
    for (int32_t x : v) std::printf(" %d", x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 5) {
        const bool und = std::atoi(argv[1]) != 0;
        const int width = std::atoi(argv[2]), h1 = std::atoi(argv[3]), ppb = std::atoi(argv[4]);
        std::vector<int32_t> N, E, R;
        for (int i = 5; i + 2 < argc; i += 3) {
            N.push_back((int32_t)std::atol(argv[i])); E.push_back((int32_t)std::atol(argv[i + 1])); R.push_back((int32_t)std::atol(argv[i + 2]));
        }
        GnnPageTable t;
        int bad = -2;
        const GnnTableError e = gnn_page_table(N.data(), E.data(), R.data(), (int)N.size(), und, width, t, &bad);
        if (e != GNN_TABLE_OK) { std::printf("refused %d %d\n", (int)e, bad); return 0; }
        GnnUnitTables u;
        if (!gnn_unit_tables(t, und, h1, ppb, u)) { std::printf("refused units\n"); return 0; }
        for (const GnnPageRow& r : t.rows)
            std::printf("row %d %d %d %d %d %d %d %d\n", r.node_off, r.N, r.edge_off, r.E, r.rel_off, r.R, r.table_off, r.chunk_nodes);
        std::printf("sums %llu %llu %llu %llu %llu\n", (unsigned long long)t.nodes, (unsigned long long)t.edges, (unsigned long long)t.rels,
                    (unsigned long long)t.cells, (unsigned long long)t.max_corrected);
        print_vec("node_begin", t.node_begin);
        print_vec("fill", u.fill); print_vec("chunk", u.chunk); print_vec("pre", u.pre); print_vec("cls", u.cls);
        return 0;
    }

    // ---- every node and every unit of a mixed call finds its own page; per page the unit counts are the single-page launchers' grids ----
    {
        const std::vector<int32_t> N = {1, 2, 3, 7, 64, 65, 130, 400}, E = {0, 1, 5, 0, 300, 9000, 600000, 17}, R = {1, 4, 0, 49, 4096, 5, 16900, 3};
        for (int und = 0; und < 2; ++und) {
            GnnPageTable t;
            int bad = -2;
            CHECK(gnn_page_table(N.data(), E.data(), R.data(), (int)N.size(), und != 0, 64, t, &bad) == GNN_TABLE_OK && bad == -1);
            GnnUnitTables u;
            CHECK(gnn_unit_tables(t, und != 0, 64, 256, u));
            const int n = (int)N.size();
            long long nodes = 0, edges = 0, rels = 0, cells = 0;
            for (int b = 0; b < n; ++b) {
                const GnnPageRow& r = t.rows[(size_t)b];
                CHECK(r.node_off == nodes && r.edge_off == edges && r.rel_off == rels && r.table_off == cells);
                CHECK(r.N == N[(size_t)b] && r.E == E[(size_t)b] && r.R == R[(size_t)b]);
                for (int k = 0; k < r.N; ++k) CHECK(page_of_unit(t.node_begin.data(), n, r.node_off + k) == b);
                int fill = 0;
                for (long long done = 0; done < (long long)(und ? 2 : 1) * r.E && fill < 2048; done += 256) ++fill;
                CHECK(u.fill[(size_t)b + 1] - u.fill[(size_t)b] == fill);
                int chunks = 0;
                for (int lo = 0; lo < r.N; lo += r.chunk_nodes) ++chunks;
                CHECK(r.chunk_nodes == (100000 / r.N > 1 ? 100000 / r.N : 1) && u.chunk[(size_t)b + 1] - u.chunk[(size_t)b] == chunks);
                int pre = 0;
                for (long long done = 0; done < (long long)r.N * 64 && pre < 1024; done += 256) ++pre;
                CHECK(u.pre[(size_t)b + 1] - u.pre[(size_t)b] == pre);
                int cls = 0;
                for (long long done = 0; done < r.R; done += 256) ++cls;
                CHECK(u.cls[(size_t)b + 1] - u.cls[(size_t)b] == cls);
                for (int k = u.cls[(size_t)b]; k < u.cls[(size_t)b + 1]; ++k) CHECK(page_of_unit(u.cls.data(), n, k) == b);
                for (int k = u.fill[(size_t)b]; k < u.fill[(size_t)b + 1]; ++k) CHECK(page_of_unit(u.fill.data(), n, k) == b);
                nodes += r.N; edges += r.E; rels += r.R; cells += (long long)r.N * r.N;
            }
            CHECK((long long)t.nodes == nodes && (long long)t.edges == edges && (long long)t.rels == rels && (long long)t.cells == cells);
            CHECK(t.node_begin[(size_t)n] == nodes);
        }
    }
    // ---- pinned numbers: the first page size of two interaction chunks, and the sizes at which the fill and the per-node launches are capped ----
    {
        const std::vector<int32_t> N = {316, 317, 400, 800, 4200, 4096, 4097}, E = {0, 900, 2500, 300000, 8000, 262144, 262145},
                                   R = {0, 0, 0, 200, 500, 0, 0};
        const int chunk_nodes[] = {316, 315, 250, 125, 23, 24, 24}, chunks[] = {1, 2, 2, 7, 183, 171, 171};
        const int pre[] = {79, 80, 100, 200, 1024, 1024, 1024};                 // N * 64 / 256 blocks up to N = 4096, 1024 beyond
        const int fill_und[] = {0, 8, 20, 2048, 63, 2048, 2048}, fill_dir[] = {0, 4, 10, 1172, 32, 1024, 1025};
        for (int und = 0; und < 2; ++und) {
            GnnPageTable t;
            int bad = -2;
            CHECK(gnn_page_table(N.data(), E.data(), R.data(), (int)N.size(), und != 0, 64, t, &bad) == GNN_TABLE_OK && bad == -1);
            GnnUnitTables u;
            CHECK(gnn_unit_tables(t, und != 0, 64, 256, u));
            for (size_t b = 0; b < N.size(); ++b) {
                CHECK(t.rows[b].chunk_nodes == chunk_nodes[b] && u.chunk[b + 1] - u.chunk[b] == chunks[b]);
                CHECK(u.pre[b + 1] - u.pre[b] == pre[b]);
                CHECK(u.fill[b + 1] - u.fill[b] == (und ? fill_und[b] : fill_dir[b]));
            }
            // what a capped page's blocks stride over: 600 000 fed entries in 2048 x 256, 4200 x 64 first-layer terms in 1024 x 256
            CHECK(!und || 2ll * E[3] > 2048ll * 256);
            CHECK((long long)N[4] * 64 > 1024ll * 256);
        }
    }
    // ---- refusals: the page at fault is named, nothing past the arrays is read ----
    {
        GnnPageTable t;
        int bad = -2;
        const int32_t N0[] = {5, 0, 7}, E0[] = {1, 1, 1}, R0[] = {1, 1, 1};
        CHECK(gnn_page_table(N0, E0, R0, 3, true, 64, t, &bad) == GNN_TABLE_BAD_N && bad == 1);
        const int32_t N1[] = {5, 6}, E1[] = {1, -1}, R1[] = {1, 1};
        CHECK(gnn_page_table(N1, E1, R1, 2, true, 64, t, &bad) == GNN_TABLE_BAD_E && bad == 1);
        const int32_t R2[] = {-3, 1};
        CHECK(gnn_page_table(N1, R1, R2, 2, true, 64, t, &bad) == GNN_TABLE_BAD_R && bad == 0);
        const int32_t N3[] = {32768, 32769}, Z[] = {0, 0};
        CHECK(gnn_page_table(N3, Z, Z, 1, true, 64, t, &bad) == GNN_TABLE_OK);                       // 2^30 cells: the single page's own bound
        CHECK(gnn_page_table(N3 + 1, Z, Z, 1, true, 64, t, &bad) == GNN_TABLE_PAGE_TOO_LARGE && bad == 0);
        const int32_t N4[] = {32768, 1}, N5[] = {20000, 20000, 20000};
        CHECK(gnn_page_table(N4, Z, Z, 2, true, 64, t, &bad) == GNN_TABLE_SUM_TABLES && bad == 1);   // one cell too many
        const int32_t Z3[] = {0, 0, 0};
        CHECK(gnn_page_table(N5, Z3, Z3, 3, true, 64, t, &bad) == GNN_TABLE_SUM_TABLES && bad == 2);
        // sums that leave 31 bits: relations (INT32_MAX / width each), edges
        const int32_t N6[] = {10, 10}, R6[] = {20000000, 20000000};
        CHECK(gnn_page_table(N6, Z, R6, 2, true, 64, t, &bad) == GNN_TABLE_SUM_INDEX && bad == 1);
        CHECK(gnn_page_table(N6, Z, R6, 2, true, 2, t, &bad) == GNN_TABLE_OK);
        const int32_t E6[] = {INT32_MAX, INT32_MAX};
        CHECK(gnn_page_table(N6, E6, Z, 2, false, 1, t, &bad) == GNN_TABLE_SUM_INDEX && bad == 1);
        CHECK(gnn_page_table(N6, E6, Z, 1, true, 1, t, &bad) == GNN_TABLE_SUM_INDEX && bad == 0);    // 2 E entries of an undirected page
        CHECK(gnn_page_table(N6, Z, Z, 0, true, 64, t, &bad) == GNN_TABLE_OK && t.rows.empty() && t.node_begin.size() == 1);
    }
    if (failures) return 1;
    std::printf("gnn page table ok: offsets, unit tables and refusals\n");
    return 0;
}
