// Host side of the article separation measure (include/asep_hip.h, "article separation measure" block): entry points on
// the asep_post handle (its stream and buffer pool).  Compiled with -ffp-contract=off, like the kernels it launches.
#include <vector>

#include "asep_common.h"
#include "batch_tables.h"
#include "measure_kernels.h"

using namespace asep;

namespace {

const char* const FN = "asep_measure_run";

// device time of the kernels of this thread's last asep_measure_run (0 count, 1 pair, 2 recall), microseconds
thread_local double g_kernel_us[3] = {0.0, 0.0, 0.0};

// results of this thread's last asep_measure_run, held in the handle's pool until asep_measure_fetch copies them out
struct Results {
    asep_post* owner = nullptr;
    long long n_pairs = 0, n_recs = 0;
    int n_truth = 0, n_tols = 0, bins = 0;
    bool hist = false;
    int2 *pair_ij = nullptr, *rec_ja = nullptr;
    double *pair_hits = nullptr, *rec_hits = nullptr, *truth_hits = nullptr;
    uint32_t *pair_hist = nullptr, *rec_hist = nullptr, *truth_hist = nullptr;
};
thread_local Results g_res;

}  // namespace

double asep_measure_last_kernel_us(int which) { return (which >= 0 && which < 3) ? g_kernel_us[which] : -1.0; }

long long asep_measure_run(asep_post* p, int n_files, const int32_t* t_file_off, const int32_t* r_file_off,
                           const int32_t* t_poly_off, const int32_t* t_points, const int32_t* t_boxes,
                           const int32_t* r_poly_off, const int32_t* r_points, const int32_t* r_boxes,
                           const int32_t* art_file_off, const int32_t* art_off, const int32_t* art_has_id, int n_tols,
                           const double* tols, int dmax, int want_hist, long long* out_counts) {
    g_res = Results();
    if (!p || n_files < 0 || !t_file_off || !r_file_off || !art_file_off || !t_poly_off || !r_poly_off || !art_off ||
        !out_counts || n_tols < 1) {
        set_error("asep_measure_run: bad arguments");
        return ASEP_ERR_ARG;
    }
    if (dmax < 0 || dmax > MEASURE_MAX_DMAX) {
        set_error("asep_measure_run: dmax %d outside 0..%d (three times the largest tolerance)", dmax, MEASURE_MAX_DMAX);
        return ASEP_ERR_ARG;
    }
    const int n_truth = t_file_off[n_files], n_reco = r_file_off[n_files], n_arts = art_file_off[n_files];
    if (n_truth < 0 || n_reco < 0 || n_arts < 0 || !check_offsets(FN, "t_file_off", t_file_off, n_files) ||
        !check_offsets(FN, "r_file_off", r_file_off, n_files) || !check_offsets(FN, "art_file_off", art_file_off, n_files))
        return ASEP_ERR_ARG;
    const int n_tp = t_poly_off[n_truth], n_rp = r_poly_off[n_reco];
    if (!check_offsets(FN, "t_poly_off", t_poly_off, n_truth, true) || !check_offsets(FN, "r_poly_off", r_poly_off, n_reco, true))
        return ASEP_ERR_ARG;
    if (art_off[n_arts] != n_reco) {
        set_error("%s: art_off ends at %d, the files hold %d reco polygons", FN, art_off[n_arts], n_reco);
        return ASEP_ERR_ARG;
    }
    if (!check_offsets(FN, "art_off", art_off, n_arts)) return ASEP_ERR_ARG;
    if ((n_tp && !t_points) || (n_rp && !r_points) || (n_truth && (!t_boxes || !tols)) || (n_reco && !r_boxes) ||
        (n_arts && !art_has_id)) {
        set_error("asep_measure_run: null argument");
        return ASEP_ERR_ARG;
    }
    // the articles of a file must tile the file's reco polygons
    for (int f = 0; f < n_files; ++f) {
        const int a0 = art_file_off[f], a1 = art_file_off[f + 1];
        const int lo = a0 < a1 ? art_off[a0] : r_file_off[f], hi = a0 < a1 ? art_off[a1] : r_file_off[f + 1];
        if (lo != r_file_off[f] || hi != r_file_off[f + 1]) {
            set_error("asep_measure_run: the articles of file %d cover reco polygons %d..%d, the file holds %d..%d", f, lo, hi,
                      r_file_off[f], r_file_off[f + 1]);
            return ASEP_ERR_ARG;
        }
    }
    int max_points = 1;
    for (int j = 0; j < n_truth; ++j) max_points = std::max(max_points, t_poly_off[j + 1] - t_poly_off[j]);
    if (max_points > MEASURE_MAX_POINTS) {
        set_error("asep_measure_run: a truth polygon of %d points (at most %d)", max_points, MEASURE_MAX_POINTS);
        return ASEP_ERR_ARG;
    }
    out_counts[0] = out_counts[1] = 0;
    g_kernel_us[0] = g_kernel_us[1] = g_kernel_us[2] = 0.0;
    const int bins = dmax + 2;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    std::vector<int32_t> r_range(2 * (size_t)n_reco), t_arts(2 * (size_t)n_truth);
    for (int f = 0; f < n_files; ++f) {
        for (int i = r_file_off[f]; i < r_file_off[f + 1]; ++i) {
            r_range[2 * (size_t)i] = t_file_off[f];
            r_range[2 * (size_t)i + 1] = t_file_off[f + 1];
        }
        for (int j = t_file_off[f]; j < t_file_off[f + 1]; ++j) {
            t_arts[2 * (size_t)j] = art_file_off[f];
            t_arts[2 * (size_t)j + 1] = art_file_off[f + 1];
        }
    }
    pool.begin();
    int2* d_tp = upload(pool, st, (const int2*)t_points, (size_t)n_tp);
    int2* d_rp = upload(pool, st, (const int2*)r_points, (size_t)n_rp);
    int* d_toff = upload(pool, st, t_poly_off, (size_t)n_truth + 1);
    int* d_roff = upload(pool, st, r_poly_off, (size_t)n_reco + 1);
    int4* d_tbox = upload(pool, st, (const int4*)t_boxes, (size_t)n_truth);
    int4* d_rbox = upload(pool, st, (const int4*)r_boxes, (size_t)n_reco);
    int2* d_rrange = upload(pool, st, (const int2*)r_range.data(), (size_t)n_reco);
    int2* d_tarts = upload(pool, st, (const int2*)t_arts.data(), (size_t)n_truth);
    int* d_aoff = upload(pool, st, art_off, (size_t)n_arts + 1);
    int* d_aid = upload(pool, st, art_has_id, (size_t)n_arts);
    double* d_tols = upload(pool, st, tols, (size_t)n_truth * n_tols);
    int* d_count = (int*)pool.get(((size_t)n_reco + n_truth + 1) * sizeof(int));
    KernelTimer tm_count, tm_pair, tm_recall;

    std::vector<int> count((size_t)n_reco + n_truth);
    std::vector<long long> off((size_t)n_reco + n_truth + 2, 0);
    if (n_reco + n_truth > 0) {
        tm_count.start(st);
        ms_count_kernel<<<(unsigned)cdiv(n_reco + n_truth, MEASURE_BLOCK), MEASURE_BLOCK, 0, st>>>(
            d_tbox, d_rbox, d_rrange, d_tarts, d_aoff, n_truth, n_reco, dmax, d_count, d_count + n_reco);
        ASEP_HIP_CHECK(hipGetLastError());
        tm_count.stop(st);
        ASEP_HIP_CHECK(hipMemcpyAsync(count.data(), d_count, count.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        ASEP_HIP_CHECK(hipStreamSynchronize(st));
        tm_count.read(g_kernel_us[0]);
    }
    // pair_off [n_reco + 1] and rec_off [n_truth + 1], one after the other
    long long* pair_off = off.data();
    long long* rec_off = off.data() + n_reco + 1;
    for (int i = 0; i < n_reco; ++i) pair_off[i + 1] = pair_off[i] + count[i];
    for (int j = 0; j < n_truth; ++j) rec_off[j + 1] = rec_off[j] + count[(size_t)n_reco + j];
    const long long n_pairs = pair_off[n_reco], n_recs = rec_off[n_truth];
    long long* d_off = upload(pool, st, off.data(), off.size());
    Results r;
    r.owner = p;
    r.n_pairs = n_pairs;
    r.n_recs = n_recs;
    r.n_truth = n_truth;
    r.n_tols = n_tols;
    r.bins = bins;
    r.hist = want_hist != 0;
    r.pair_ij = (int2*)pool.get((size_t)(n_pairs + 1) * sizeof(int2));
    r.pair_hits = (double*)pool.get((size_t)(n_pairs + 1) * n_tols * sizeof(double));
    r.rec_ja = (int2*)pool.get((size_t)(n_recs + 1) * sizeof(int2));
    r.rec_hits = (double*)pool.get((size_t)(n_recs + 1) * n_tols * sizeof(double));
    r.truth_hits = (double*)pool.get(((size_t)n_truth * 2 + 1) * n_tols * sizeof(double));
    if (r.hist) {
        r.pair_hist = (uint32_t*)pool.get((size_t)(n_pairs + 1) * bins * sizeof(uint32_t));
        r.rec_hist = (uint32_t*)pool.get((size_t)(n_recs + 1) * bins * sizeof(uint32_t));
        r.truth_hist = (uint32_t*)pool.get(((size_t)n_truth * 2 + 1) * bins * sizeof(uint32_t));
    }
    if (n_reco > 0 && n_pairs > 0) {
        tm_pair.start(st);
        ms_pair_kernel<<<(unsigned)n_reco, MEASURE_BLOCK, (size_t)bins * sizeof(int), st>>>(
            d_tp, d_toff, d_tbox, d_rp, d_roff, d_rbox, d_rrange, d_tols, n_tols, dmax, d_off, r.pair_ij, r.pair_hits, r.pair_hist);
        ASEP_HIP_CHECK(hipGetLastError());
        tm_pair.stop(st);
    }
    if (n_truth > 0) {
        tm_recall.start(st);
        ms_recall_kernel<<<(unsigned)n_truth, MEASURE_BLOCK, ((size_t)bins + 2 * (size_t)max_points) * sizeof(int), st>>>(
            d_tp, d_toff, d_tbox, d_rp, d_roff, d_rbox, d_tarts, d_aoff, d_aid, d_tols, n_tols, dmax, max_points,
            d_off + n_reco + 1, r.rec_ja, r.rec_hits, r.truth_hits, r.rec_hist, r.truth_hist);
        ASEP_HIP_CHECK(hipGetLastError());
        tm_recall.stop(st);
    }
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    if (n_reco > 0 && n_pairs > 0) tm_pair.read(g_kernel_us[1]);
    if (n_truth > 0) tm_recall.read(g_kernel_us[2]);
    out_counts[0] = n_pairs;
    out_counts[1] = n_recs;
    g_res = r;
    return n_pairs;
    ASEP_GUARD_END
}

int asep_measure_fetch(asep_post* p, int32_t* pair_ij, double* pair_hits, int32_t* rec_ja, double* rec_hits,
                       double* truth_hits, uint32_t* pair_hist, uint32_t* rec_hist, uint32_t* truth_hist) {
    const Results& r = g_res;
    if (!p || r.owner != p) {
        set_error("asep_measure_fetch: no results of asep_measure_run on this handle and thread");
        return ASEP_ERR_ARG;
    }
    if ((pair_hist || rec_hist || truth_hist) && !r.hist) {
        set_error("asep_measure_fetch: histograms were not requested (want_hist)");
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    auto fetch = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    const size_t nt = (size_t)r.n_tols, nb = (size_t)r.bins * sizeof(uint32_t);
    ASEP_HIP_CHECK(fetch(pair_ij, r.pair_ij, (size_t)r.n_pairs * sizeof(int2)));
    ASEP_HIP_CHECK(fetch(pair_hits, r.pair_hits, (size_t)r.n_pairs * nt * sizeof(double)));
    ASEP_HIP_CHECK(fetch(rec_ja, r.rec_ja, (size_t)r.n_recs * sizeof(int2)));
    ASEP_HIP_CHECK(fetch(rec_hits, r.rec_hits, (size_t)r.n_recs * nt * sizeof(double)));
    ASEP_HIP_CHECK(fetch(truth_hits, r.truth_hits, (size_t)r.n_truth * 2 * nt * sizeof(double)));
    ASEP_HIP_CHECK(fetch(pair_hist, r.pair_hist, (size_t)r.n_pairs * nb));
    ASEP_HIP_CHECK(fetch(rec_hist, r.rec_hist, (size_t)r.n_recs * nb));
    ASEP_HIP_CHECK(fetch(truth_hist, r.truth_hist, (size_t)r.n_truth * 2 * nb));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    return ASEP_OK;
    ASEP_GUARD_END
}
