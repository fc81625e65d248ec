// Clustering grid (clustering/dbscan.py, DBScanRelation.cluster_relations, and the split / merge counts of as_eval.py): one
// wavefront per (page, setting) problem.  The labels are the host class's, integer for integer: the neighbourhood and
// agreement comparisons are taken in the matrix dtype against the threshold rounded to that dtype, and the agreement mean
// is numpy's np.mean of the gathered row (np_mean below: pairwise summation in numpy's order, then one division).
// Compiled with -ffp-contract=off.  The summation template at the top needs no HIP: a host test compiles it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLG_HD __host__ __device__
#else
#define CLG_HD
#endif

namespace asep {

constexpr int CLG_MAX_NODES = 2048;    // nodes of one page: labels, owner queue and member values of a problem sit in LDS
constexpr int CLG_PAIRWISE_DEPTH = 6;  // halvings of np_pairwise_sum above its 128-element blocks

// numpy's pairwise_sum (the inner loop of np.add.reduce over a contiguous array) for n <= 128: below 8 a serial sum from
// 0, else eight running sums seeded with a[0..7] and stepped by 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
// then the n % 8 tail added serially.
template <class T>
CLG_HD inline T np_block_sum(const T* a, int n) {
    if (n < 8) {
        T res = T(0);
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    T r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += a[i + 0];
        r1 += a[i + 1];
        r2 += a[i + 2];
        r3 += a[i + 3];
        r4 += a[i + 4];
        r5 += a[i + 5];
        r6 += a[i + 6];
        r7 += a[i + 7];
    }
    T res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

// Above 128 elements numpy splits at n2 = n/2 - (n/2) % 8 and adds the two halves' results.  DEPTH bounds the halvings
// (the recursion is unrolled by the template, no device stack): pairwise_depth() says how many a length needs.
template <class T, int DEPTH = CLG_PAIRWISE_DEPTH>
CLG_HD inline T np_pairwise_sum(const T* a, int n) {
    if constexpr (DEPTH > 0) {
        if (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            return np_pairwise_sum<T, DEPTH - 1>(a, n2) + np_pairwise_sum<T, DEPTH - 1>(a + n2, n - n2);
        }
    }
    return np_block_sum(a, n);
}

constexpr int pairwise_depth(int n) {
    int d = 0;
    while (n > 128) {      // the longer half: n - n2
        int n2 = n / 2;
        n2 -= n2 % 8;
        n -= n2;
        ++d;
    }
    return d;
}
static_assert(pairwise_depth(CLG_MAX_NODES) <= CLG_PAIRWISE_DEPTH && pairwise_depth(CLG_MAX_NODES - 1) <= CLG_PAIRWISE_DEPTH,
              "np_pairwise_sum cannot halve a row of CLG_MAX_NODES members down to 128");

// np.mean of a contiguous 1-D array of n >= 1 values, in the array's dtype
template <class T>
CLG_HD inline T np_mean(const T* a, int n) {
    return (T(0) + np_pairwise_sum<T>(a, n)) / T(n);
}

#if defined(__HIPCC__)

constexpr int CLG_WAVE = 64;
constexpr int CLG_MAX_PROBLEMS = 1 << 26;             // blocks of one launch: gridDim.x * blockDim.x stays below 2^32
constexpr int CLG_UNVISITED = 0, CLG_NOISE = -1;      // dbscan.py

constexpr int CLG_DBSCAN = 0, CLG_DBSCAN_STD = 1, CLG_GREEDY = 2;   // ASEP_CLUSTER_* (include/asep_hip.h)

// asep_cluster_setting (include/asep_hip.h)
struct ClgSetting {
    int32_t min_neighbors, assign_noise;
    double conf_thr, agree_thr;
};

// asep_cluster_method_setting (include/asep_hip.h)
struct ClgMethodSetting {
    int32_t method, count, assign_noise, reserved;
    double conf_thr, param;
};

__device__ __forceinline__ int clg_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// number of j != i with conf[i, j] > thr (region_query's length), lanes striding over the row
template <class T>
__device__ __forceinline__ int clg_reach_count(const T* __restrict__ row, int n, int i, T thr, int lane) {
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
        const int j = j0 + lane;
        const bool hit = j < n && j != i && row[j] > thr;
        cnt += __popcll(__ballot(hit));
    }
    return clg_uniform(cnt);
}

// grid n_pages * n_settings blocks of one wave, the settings of a page next to each other (they read the same matrix).
// Dynamic LDS: max_n member values (T), max_n labels, max_n queued owners.  Page k has the nodes node_off[k] ..
// node_off[k+1]-1 and its matrix at conf + conf_off[k]; out_labels [.][node_off[n_pages]], setting s in row out_row[s] (in row s
// without out_row).
template <class T>
__global__ void __launch_bounds__(CLG_WAVE) cluster_grid_kernel(const T* __restrict__ conf, const int64_t* __restrict__ conf_off,
                                                                const int32_t* __restrict__ node_off,
                                                                const ClgSetting* __restrict__ settings, int n_settings, int n_pages,
                                                                int max_n, const int32_t* __restrict__ out_row,
                                                                int32_t* __restrict__ out_labels) {
    extern __shared__ __align__(16) unsigned char clg_lds[];
    T* vals = (T*)clg_lds;
    int32_t* labels = (int32_t*)(vals + max_n);
    int32_t* queue = labels + max_n;

    const int lane = threadIdx.x;
    const int page = blockIdx.x / n_settings, s = blockIdx.x % n_settings;
    const int n0 = node_off[page], n = node_off[page + 1] - n0;
    const T* __restrict__ m = conf + conf_off[page];
    const ClgSetting st = settings[s];
    const T conf_thr = (T)st.conf_thr, agree_thr = (T)st.agree_thr;   // numpy compares an array with a Python float in the array's dtype
    const int min_nb = st.min_neighbors;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;

    int32_t* out = out_labels + (size_t)(out_row ? out_row[s] : s) * node_off[n_pages] + n0;
    if (n == 2) {       // TextblockClustering.calc: two nodes are one article iff conf[0, 1] >= confidence_threshold, no clustering
        if (lane < 2) out[lane] = (lane == 0 || m[1] >= conf_thr) ? 1 : 2;
        return;
    }
    for (int i = lane; i < n; i += CLG_WAVE) labels[i] = CLG_UNVISITED;
    __syncthreads();

    int label = 0;
    for (int node = 0; node < n; ++node) {
        if (labels[node] != CLG_UNVISITED) continue;                  // (one address: the same value in every lane)
        if (clg_reach_count(m + (size_t)node * n, n, node, conf_thr, lane) < min_nb) {
            if (lane == 0) labels[node] = CLG_NOISE;
            __syncthreads();
            continue;
        }
        ++label;
        if (lane == 0) {
            labels[node] = label;
            queue[0] = node;
        }
        __syncthreads();
        // grow_cluster: the frontier is reach(seed) followed by reach(c) of every accepted owner c, in acceptance order;
        // an owner enters the queue once (it leaves UNVISITED when it does), so the queue holds at most n owners
        int q_len = 1;
        for (int q = 0; q < q_len; ++q) {
            const int owner = queue[q];
            const T* __restrict__ orow = m + (size_t)owner * n;
            for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
                const int j = j0 + lane;
                // a node that carries a label keeps it: only NOISE / UNVISITED candidates can still be taken
                const bool hit = j < n && j != owner && orow[j] > conf_thr && labels[j] <= 0;
                unsigned long long todo = __ballot(hit);
                while (todo) {
                    const int cand = j0 + (int)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    const int state = labels[cand];
                    if (state != CLG_NOISE && state != CLG_UNVISITED) continue;     // taken meanwhile, earlier in this row
                    // validate_cluster_agreement: the candidate's confidences to the members, ascending, then np.mean
                    const T* __restrict__ crow = m + (size_t)cand * n;
                    int n_mem = 0;
                    for (int k0 = 0; k0 < n; k0 += CLG_WAVE) {
                        const int k = k0 + lane;
                        const bool mem = k < n && labels[k] == label;
                        const unsigned long long mm = __ballot(mem);
                        if (mem) vals[n_mem + __popcll(mm & lanes_below)] = crow[k];
                        n_mem += __popcll(mm);
                    }
                    __syncthreads();
                    const bool agree = np_mean(vals, n_mem) > agree_thr;
                    __syncthreads();                                   // vals are read before the next gather overwrites them
                    if (!agree) continue;
                    bool expand = false;
                    if (state == CLG_UNVISITED) expand = clg_reach_count(crow, n, cand, conf_thr, lane) >= min_nb;
                    if (lane == 0) {
                        labels[cand] = label;
                        if (expand) queue[q_len] = cand;
                    }
                    if (expand) ++q_len;
                    __syncthreads();
                }
            }
        }
    }
    // create_clusters_for_noise_nodes: fresh labels in index order
    if (st.assign_noise) {
        for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
            const int j = j0 + lane;
            const bool noise = j < n && labels[j] == CLG_NOISE;
            const unsigned long long nm = __ballot(noise);
            if (noise) labels[j] = label + 1 + __popcll(nm & lanes_below);
            label += __popcll(nm);
        }
        __syncthreads();
    }
    for (int i = lane; i < n; i += CLG_WAVE) out[i] = labels[i];
}

// ---- dbscan_std, greedy and rel_LLH (TextblockClustering._dbscan_std, ._greedy, ._calc_relative_LLH) ----------------------------
// The same mapping: one wave per (page, setting), the settings of a page in neighbouring blocks.  `settings` is the call's whole
// list and sel[0 .. n_sel) the indices of the method's own settings in it: block b works on page b / n_sel under setting
// s = sel[b % n_sel] and writes row s of out_labels.  Every page's matrix sits at the page's conf_off in its set.

// calc()'s rule for a page of two nodes, whatever the method: conf01 = _conf_mat[0, 1] as given
template <class T>
__device__ __forceinline__ void clg_two_nodes(T conf01, T conf_thr, int lane, int32_t* __restrict__ out) {
    if (lane < 2) out[lane] = (lane == 0 || conf01 >= conf_thr) ? 1 : 2;
}

// sklearn.cluster.dbscan(dist, metric='precomputed', eps, min_samples), restated in tests/test_cluster_methods_host.py.
// Dynamic LDS: max_n labels, max_n queued owners, max_n core flags (bytes).
template <class T>
__global__ void __launch_bounds__(CLG_WAVE) cluster_std_kernel(const T* __restrict__ conf, const T* __restrict__ dist,
                                                               const int64_t* __restrict__ conf_off,
                                                               const int32_t* __restrict__ node_off,
                                                               const ClgMethodSetting* __restrict__ settings,
                                                               const int32_t* __restrict__ sel, int n_sel, int n_pages, int max_n,
                                                               int32_t* __restrict__ out_labels) {
    extern __shared__ __align__(16) unsigned char clg_lds[];
    int32_t* labels = (int32_t*)clg_lds;
    int32_t* queue = labels + max_n;
    uint8_t* core = (uint8_t*)(queue + max_n);

    const int lane = threadIdx.x;
    const int page = blockIdx.x / n_sel, s = sel[blockIdx.x % n_sel];
    const int n0 = node_off[page], n = node_off[page + 1] - n0;
    const ClgMethodSetting st = settings[s];
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    int32_t* out = out_labels + (size_t)s * node_off[n_pages] + n0;
    if (n == 2) {
        clg_two_nodes(conf[conf_off[page] + 1], (T)st.conf_thr, lane, out);
        return;
    }
    const T* __restrict__ m = dist + conf_off[page];
    const T eps = (T)st.param;
    const int min_samples = st.count;

    for (int i = 0; i < n; ++i) {
        const T* __restrict__ row = m + (size_t)i * n;
        int cnt = 0;
        for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
            const int j = j0 + lane;
            cnt += __popcll(__ballot(j < n && row[j] <= eps));
        }
        if (lane == 0) core[i] = clg_uniform(cnt) >= min_samples;
    }
    for (int i = lane; i < n; i += CLG_WAVE) labels[i] = -1;
    __syncthreads();

    int label = 0;
    for (int seed = 0; seed < n; ++seed) {
        if (labels[seed] != -1 || !core[seed]) continue;                // (one address each: the same in every lane)
        if (lane == 0) {
            labels[seed] = label;
            queue[0] = seed;
        }
        __syncthreads();
        // the closure of the seed: every node is labelled once, and queued when it is labelled and a core point
        int q_len = 1;
        for (int q = 0; q < q_len; ++q) {
            const T* __restrict__ orow = m + (size_t)queue[q] * n;
            for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
                const int j = j0 + lane;
                const bool hit = j < n && orow[j] <= eps && labels[j] == -1;
                const bool grow = hit && core[j];
                const unsigned long long gm = __ballot(grow);
                if (hit) labels[j] = label;
                if (grow) queue[q_len + __popcll(gm & lanes_below)] = j;
                q_len += __popcll(gm);
            }
            __syncthreads();
        }
        ++label;
    }
    for (int i = lane; i < n; i += CLG_WAVE) out[i] = labels[i];
}

template <class T>
__device__ __forceinline__ T clg_neg_inf() {
    return -__builtin_huge_val();
}

// the largest v of the wave and the smallest idx among the lanes that hold it (INT32_MAX when no lane has a candidate)
template <class T>
__device__ __forceinline__ void clg_wave_argmax(T& v, int& idx) {
    T mx = v;
    for (int d = 32; d > 0; d >>= 1) {
        const T o = __shfl_xor(mx, d);
        mx = o > mx ? o : mx;
    }
    int best = v == mx ? idx : INT32_MAX;
    for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d));
    v = mx;
    idx = best;
}

// first maximum of row r of the working matrix over the classes that are left (alive[c] == c), the diagonal excluded
template <class T>
__device__ __forceinline__ void clg_row_argmax(const T* row, const int32_t* alive, int n, int r, int lane, T& mx, int& col) {
    mx = clg_neg_inf<T>();
    col = INT32_MAX;
    for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
        const int j = j0 + lane;
        if (j < n && j != r && alive[j] == j) {
            const T v = row[j];
            if (v > mx) {
                mx = v;
                col = j;
            }
        }
    }
    clg_wave_argmax(mx, col);
}

// TextblockClustering._greedy.  work: N^2 values per problem, block b at work_off[page] * n_sel + (b % n_sel) * N^2; the kernel
// copies delta into it.  Dynamic LDS per node: the row's maximum over the classes left (T), the first column that attains it,
// and the class the node is in (owner[c] == c: class c is left; a class always holds the node of its own index).  np.argmax's
// "first in row-major order" is the lowest row that attains the maximum and that row's first column, so the global argmax is a
// scan of the cached rows.  A row and column that left are not overwritten with -inf: they are skipped through `owner`.
template <class T>
__global__ void __launch_bounds__(CLG_WAVE) cluster_greedy_kernel(const T* __restrict__ conf, const T* __restrict__ delta,
                                                                  const int64_t* __restrict__ conf_off,
                                                                  const int32_t* __restrict__ node_off,
                                                                  const ClgMethodSetting* __restrict__ settings,
                                                                  const int32_t* __restrict__ sel, int n_sel, int n_pages,
                                                                  int max_n, T* work, int32_t* __restrict__ out_labels) {
    extern __shared__ __align__(16) unsigned char clg_lds[];
    T* rowmax = (T*)clg_lds;
    int32_t* rowarg = (int32_t*)(rowmax + max_n);
    int32_t* owner = rowarg + max_n;

    const int lane = threadIdx.x;
    const int page = blockIdx.x / n_sel, g = blockIdx.x % n_sel, s = sel[g];
    const int n0 = node_off[page], n = node_off[page + 1] - n0;
    const ClgMethodSetting st = settings[s];
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    int32_t* out = out_labels + (size_t)s * node_off[n_pages] + n0;
    if (n == 2) {
        clg_two_nodes(conf[conf_off[page] + 1], (T)st.conf_thr, lane, out);
        return;
    }
    const T* __restrict__ src = delta + conf_off[page];
    T* m = work + conf_off[page] * n_sel + (int64_t)g * n * n;
    const int RESCAN = -1;

    for (int i = lane; i < n; i += CLG_WAVE) owner[i] = i;
    __syncthreads();
    for (int r = 0; r < n; ++r) {
        for (int j = lane; j < n; j += CLG_WAVE) m[(size_t)r * n + j] = src[(size_t)r * n + j];
        T mx;
        int col;
        clg_row_argmax(src + (size_t)r * n, owner, n, r, lane, mx, col);
        if (lane == 0) {
            rowmax[r] = mx;
            rowarg[r] = col;
        }
    }
    __syncthreads();

    for (int budget = st.count; budget > 0; --budget) {
        T best = clg_neg_inf<T>();
        int keep = INT32_MAX;
        for (int r = lane; r < n; r += CLG_WAVE)
            if (rowmax[r] > best) {
                best = rowmax[r];
                keep = r;
            }
        clg_wave_argmax(best, keep);
        if (!(best > T(0))) break;
        keep = clg_uniform(keep);
        const int drop = rowarg[keep];
        // the nodes of class `drop` move to class `keep`; owner[drop] != drop from here on: row and column `drop` have left
        for (int x = lane; x < n; x += CLG_WAVE)
            if (owner[x] == drop) owner[x] = keep;
        __syncthreads();
        T kmax = clg_neg_inf<T>();
        int kcol = INT32_MAX;
        for (int idx = lane; idx < n; idx += CLG_WAVE) {
            if (idx == keep || owner[idx] != idx) continue;
            const T v = m[(size_t)idx * n + keep] + m[(size_t)idx * n + drop];
            m[(size_t)idx * n + keep] = v;
            m[(size_t)keep * n + idx] = v;
            if (v > kmax) {
                kmax = v;
                kcol = idx;
            }
            // row idx: column `keep` now holds v, column `drop` has left.  The cached first maximum stays unless it sat in
            // one of the two; in `keep` it stays as well when the entry did not fall
            const T mx = rowmax[idx];
            const int c = rowarg[idx];
            if (c == drop || (c == keep && v < mx)) {
                rowarg[idx] = RESCAN;
            } else if (v > mx || c == keep) {
                rowmax[idx] = v;
                rowarg[idx] = keep;
            } else if (v == mx && keep < c) {
                rowarg[idx] = keep;
            }
        }
        clg_wave_argmax(kmax, kcol);
        if (lane == 0) {
            rowmax[keep] = kmax;
            rowarg[keep] = kcol;
            rowmax[drop] = clg_neg_inf<T>();
        }
        __syncthreads();                                               // the stores to m and the cache, before the rescans read them
        for (int r0 = 0; r0 < n; r0 += CLG_WAVE) {
            const int r = r0 + lane;
            unsigned long long todo = __ballot(r < n && owner[r] == r && rowarg[r] == RESCAN);
            while (todo) {
                const int row = r0 + (int)__builtin_ctzll(todo);
                todo &= todo - 1;
                T mx;
                int col;
                clg_row_argmax(m + (size_t)row * n, owner, n, row, lane, mx, col);
                if (lane == 0) {
                    rowmax[row] = mx;
                    rowarg[row] = col;
                }
            }
        }
        __syncthreads();
    }
    // _classes2labels over the classes that are left, in index order
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += CLG_WAVE) {
        const int c = c0 + lane;
        const bool left = c < n && owner[c] == c;
        const unsigned long long lm = __ballot(left);
        if (left) rowarg[c] = base + __popcll(lm & lanes_below);
        base += __popcll(lm);
    }
    __syncthreads();
    for (int i = lane; i < n; i += CLG_WAVE) out[i] = rowarg[owner[i]];
}

// TextblockClustering._calc_relative_LLH over the labels the clustering kernels wrote, one wave per (page, setting) of the whole
// list: out [n_settings][n_pages].  Each term (delta[i, k] + delta[k, i]) / 2 is formed in T; lane l adds its terms in double in
// the order of the rows i and, within a row, of k = l, l + 64, ...; the 64 sums are then added pairwise across lanes at the
// distances 32, 16, ... 1.
template <class T>
__global__ void __launch_bounds__(CLG_WAVE) cluster_llh_kernel(const int32_t* __restrict__ labels_all, const T* __restrict__ delta,
                                                               const int64_t* __restrict__ conf_off,
                                                               const int32_t* __restrict__ node_off, int n_settings, int n_pages,
                                                               double* __restrict__ out) {
    const int lane = threadIdx.x;
    const int page = blockIdx.x / n_settings, s = blockIdx.x % n_settings;
    const int n = node_off[page + 1] - node_off[page];
    const int32_t* __restrict__ lab = labels_all + (size_t)s * node_off[n_pages] + node_off[page];
    const T* __restrict__ m = delta + conf_off[page];
    double sum = 0.0;
    for (int i = 1; i < n; ++i) {
        const int li = lab[i];
        if (li < 0) continue;
        for (int k = lane; k < i; k += CLG_WAVE)
            if (lab[k] == li) sum += (double)((m[(size_t)i * n + k] + m[(size_t)k * n + i]) / T(2));
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) out[(size_t)s * n_pages + page] = sum;
}

// The counts of as_eval.SepPageBlComper for one (page, setting) per wave, over the labels the kernel above wrote.  Page
// k has the lines line_off[k] .. line_off[k+1]-1: line_node = the node the line hangs in, line_gt = its dense ground
// truth article or -1; and the listed ground truth blocks gtblk_off[k] .. gtblk_off[k+1]-1, block b the lines
// gtblk_lines[gtblk_line_off[b] .. gtblk_line_off[b+1]-1] (indices within the page).  out [n_settings][n_pages] =
// {hypNIs, n_inf, corrects, 0}.  Dynamic LDS: two int arrays of max_n + 2 (labels run from -1 to n).
__global__ void __launch_bounds__(CLG_WAVE) cluster_compare_kernel(const int32_t* __restrict__ labels_all,
                                                                   const int32_t* __restrict__ node_off,
                                                                   const int32_t* __restrict__ line_off,
                                                                   const int32_t* __restrict__ line_node,
                                                                   const int32_t* __restrict__ line_gt,
                                                                   const int32_t* __restrict__ gtblk_off,
                                                                   const int32_t* __restrict__ gtblk_line_off,
                                                                   const int32_t* __restrict__ gtblk_lines, int n_settings,
                                                                   int n_pages, int max_n, int4* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char clg_lds[];
    int32_t* n_lines_of = (int32_t*)clg_lds;          // [label + 1]: lines of the page that carry the label
    int32_t* seen = n_lines_of + max_n + 2;           // [label + 1]: the label occurs in the ground truth article at hand
    const int lane = threadIdx.x;
    const int page = blockIdx.x / n_settings, s = blockIdx.x % n_settings;
    const int n = node_off[page + 1] - node_off[page];
    const int32_t* __restrict__ lab = labels_all + (size_t)s * node_off[n_pages] + node_off[page];
    const int l0 = line_off[page], nl = line_off[page + 1] - l0;
    const int32_t* __restrict__ lnode = line_node + l0;
    const int32_t* __restrict__ lgt = line_gt + l0;

    for (int i = lane; i < n + 2; i += CLG_WAVE) n_lines_of[i] = 0;
    __syncthreads();
    int gt_max = -1;
    for (int i = lane; i < nl; i += CLG_WAVE) {
        atomicAdd(&n_lines_of[lab[lnode[i]] + 1], 1);
        gt_max = max(gt_max, lgt[i]);
    }
    for (int d = 32; d > 0; d >>= 1) gt_max = max(gt_max, __shfl_xor(gt_max, d));
    __syncthreads();
    int hyp = 0;
    for (int i = lane; i < n + 2; i += CLG_WAVE) hyp += n_lines_of[i] > 0;
    // distinct (ground truth article, label) pairs: article by article, the labels of its lines marked and counted
    int inf = 0;
    for (int g = 0; g <= gt_max; ++g) {
        for (int i = lane; i < n + 2; i += CLG_WAVE) seen[i] = 0;
        __syncthreads();
        for (int i = lane; i < nl; i += CLG_WAVE)
            if (lgt[i] == g) seen[lab[lnode[i]] + 1] = 1;
        __syncthreads();
        for (int i = lane; i < n + 2; i += CLG_WAVE) inf += seen[i];
        __syncthreads();
    }
    // a listed block is an article of the hypothesis when its lines share one label and no other line carries it
    int correct = 0;
    for (int b = gtblk_off[page] + lane; b < gtblk_off[page + 1]; b += CLG_WAVE) {
        const int e0 = gtblk_line_off[b], e1 = gtblk_line_off[b + 1];
        if (e1 == e0) continue;
        const int first = lab[lnode[gtblk_lines[e0]]];
        bool same = true;
        for (int e = e0 + 1; e < e1; ++e) same = same && lab[lnode[gtblk_lines[e]]] == first;
        correct += same && n_lines_of[first + 1] == e1 - e0;
    }
    for (int d = 32; d > 0; d >>= 1) {
        hyp += __shfl_xor(hyp, d);
        inf += __shfl_xor(inf, d);
        correct += __shfl_xor(correct, d);
    }
    if (lane == 0) out[(size_t)s * n_pages + page] = make_int4(hyp, inf, correct, 0);
}

#endif  // __HIPCC__

}  // namespace asep
