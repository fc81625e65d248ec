// Host side of the relation net evaluation (include/asep_hip.h, "relation net evaluation" block): an accumulator of packed
// (score, label) keys in HBM, the radix sort and the curve passes of relation_eval_kernels.h behind asep_releval_finish.
#include <algorithm>

#include "asep_common.h"
#include "relation_eval_kernels.h"

using namespace asep;

namespace {

constexpr long long RELEV_MAX_PAIRS = (1ll << 31) - 1;    // every count and offset of the kernels is an unsigned 32-bit number
constexpr int RELEV_STAGES = 16;                           // 4 x (hist, scan, scatter), curve count / scan / write, A2
constexpr size_t RELEV_HOST_CHUNK = (size_t)1 << 24;       // append_host uploads this many pairs at a time

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                                        // elements
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
    // at least n elements, contents NOT kept
    void need(size_t n) {
        if (n <= cap) return;
        release();
        ASEP_HIP_CHECK_THROW(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
    }
};

}  // namespace

struct asep_releval {
    DevBuf<uint32_t> keys, alt, table, totals, blk_runs, blk_ones;
    DevBuf<unsigned long long> cnt;
    DevBuf<float> thr, stage_probs;
    DevBuf<long long> tps, fps;
    DevBuf<uint8_t> stage_labels;
    size_t n = 0;                                          // pairs appended
    bool finished = false;
    unsigned long long host_cnt[RELEV_C_SLOTS] = {0};      // the counter block as of the last finish
    hipEvent_t ev[RELEV_STAGES + 2] = {nullptr};          // stage s runs from ev[s] to ev[s + 1]; the last one: see finish
    double stage_us[RELEV_STAGES] = {0};
    ~asep_releval() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// room for `extra` more keys behind the h->n appended ones; grows geometrically and keeps the keys (synchronises `st` then)
int grow(asep_releval* h, size_t extra, hipStream_t st, const char* who) {
    if ((long long)(h->n + extra) > RELEV_MAX_PAIRS) {
        set_error("%s: %zu + %zu pairs: one accumulator holds fewer than 2^31 pairs (counts and offsets are 32-bit on the device)",
                  who, h->n, extra);
        return ASEP_ERR_UNSUPPORTED;
    }
    const size_t want = h->n + extra;
    if (want <= h->keys.cap) return ASEP_OK;
    const size_t cap = std::min<size_t>((size_t)RELEV_MAX_PAIRS, std::max(want, std::max<size_t>(h->keys.cap * 2, (size_t)1 << 20)));
    uint32_t* fresh = nullptr;
    ASEP_HIP_CHECK(hipMalloc((void**)&fresh, cap * sizeof(uint32_t)));
    if (h->n) {
        hipError_t e = hipMemcpyAsync(fresh, h->keys.p, h->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(fresh);
            set_error("%s: moving %zu keys to a larger buffer failed: %s", who, h->n, hipGetErrorString(e));
            return ASEP_ERR_HIP;
        }
    } else {
        ASEP_HIP_CHECK(hipStreamSynchronize(st));          // (a reset's kernels may still read the old buffer)
    }
    h->keys.release();
    h->keys.p = fresh, h->keys.cap = cap;
    return ASEP_OK;
}

int ensure_counters(asep_releval* h, hipStream_t st) {
    if (h->cnt.p) return ASEP_OK;
    h->cnt.need(RELEV_C_SLOTS);
    ASEP_HIP_CHECK(hipMemsetAsync(h->cnt.p, 0, RELEV_C_SLOTS * sizeof(unsigned long long), st));
    return ASEP_OK;
}

}  // namespace

asep_releval* asep_releval_create(void) {
    ASEP_GUARD_BEGIN
    return new asep_releval();
    ASEP_GUARD_END_PTR
}

void asep_releval_free(asep_releval* h) { delete h; }

int asep_releval_reset(asep_releval* h, void* stream) {
    if (!h) {
        set_error("asep_releval_reset: null handle");
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    h->n = 0;
    h->finished = false;
    if (h->cnt.p) ASEP_HIP_CHECK(hipMemsetAsync(h->cnt.p, 0, RELEV_C_SLOTS * sizeof(unsigned long long), (hipStream_t)stream));
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_releval_reserve(asep_releval* h, long long total_pairs, void* stream) {
    if (!h || total_pairs < 0) {
        set_error("asep_releval_reserve: bad arguments");
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    if ((size_t)total_pairs <= h->n) return ASEP_OK;
    return grow(h, (size_t)total_pairs - h->n, (hipStream_t)stream, "asep_releval_reserve");
    ASEP_GUARD_END
}

long long asep_releval_count(const asep_releval* h) { return h ? (long long)h->n : -1; }

int asep_releval_append_dev(asep_releval* h, const float* d_probs, int num_classes, long long R, const int32_t* d_gt_relations,
                            int G, int N, void* stream) {
    if (!h || num_classes < 1 || R < 0 || G < 0 || N < 0 || (R && !d_probs) || (G && !d_gt_relations)) {
        set_error("asep_releval_append_dev: bad arguments (num_classes %d >= 1, R %lld, G %d, N %d >= 0, pointers given)", num_classes, R,
                  G, N);
        return ASEP_ERR_ARG;
    }
    if (R != (long long)N * N) {
        set_error("asep_releval_append_dev: R = %lld, but the labels are those of all N * N = %lld ordered pairs (N = %d)", R,
                  (long long)N * N, N);
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    hipStream_t st = (hipStream_t)stream;
    if (R == 0) return ASEP_OK;
    int rc = grow(h, (size_t)R, st, "asep_releval_append_dev");
    if (rc < 0) return rc;
    if ((rc = ensure_counters(h, st)) < 0) return rc;
    uint32_t* page = h->keys.p + h->n;
    relev_pack_page_kernel<<<(unsigned)((R + RELEV_BLOCK - 1) / RELEV_BLOCK), RELEV_BLOCK, 0, st>>>(d_probs, num_classes, (uint32_t)R, page,
                                                                                                  h->cnt.p);
    ASEP_HIP_CHECK(hipGetLastError());
    if (G) {
        relev_label_page_kernel<<<(unsigned)cdiv(G, RELEV_BLOCK), RELEV_BLOCK, 0, st>>>(d_gt_relations, G, N, page, h->cnt.p);
        ASEP_HIP_CHECK(hipGetLastError());
    }
    h->n += (size_t)R;
    h->finished = false;
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_releval_append_host(asep_releval* h, const float* probs, const uint8_t* labels, long long n, void* stream) {
    if (!h || n < 0 || (n && (!probs || !labels))) {
        set_error("asep_releval_append_host: bad arguments");
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return ASEP_OK;
    int rc = grow(h, (size_t)n, st, "asep_releval_append_host");
    if (rc < 0) return rc;
    if ((rc = ensure_counters(h, st)) < 0) return rc;
    const size_t chunk = std::min<size_t>((size_t)n, RELEV_HOST_CHUNK);
    if (chunk > h->stage_probs.cap) ASEP_HIP_CHECK(hipStreamSynchronize(st));      // (an earlier append may still read the staging)
    h->stage_probs.need(chunk);
    h->stage_labels.need(chunk);
    for (size_t at = 0; at < (size_t)n; at += chunk) {
        const size_t m = std::min(chunk, (size_t)n - at);
        ASEP_HIP_CHECK(hipMemcpyAsync(h->stage_probs.p, probs + at, m * sizeof(float), hipMemcpyHostToDevice, st));
        ASEP_HIP_CHECK(hipMemcpyAsync(h->stage_labels.p, labels + at, m, hipMemcpyHostToDevice, st));
        relev_pack_arrays_kernel<<<(unsigned)((m + RELEV_BLOCK - 1) / RELEV_BLOCK), RELEV_BLOCK, 0, st>>>(
            h->stage_probs.p, h->stage_labels.p, (uint32_t)m, h->keys.p + h->n + at, h->cnt.p);
        ASEP_HIP_CHECK(hipGetLastError());
    }
    ASEP_HIP_CHECK(hipStreamSynchronize(st));              // the caller's arrays are free again
    h->n += (size_t)n;
    h->finished = false;
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_releval_finish(asep_releval* h, void* stream, long long* out_thresholds) {
    if (!h || !out_thresholds) {
        set_error("asep_releval_finish: null argument");
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    hipStream_t st = (hipStream_t)stream;
    if (h->finished) {                                     // nothing was appended since: the results are still there
        *out_thresholds = (long long)h->host_cnt[RELEV_C_T];
        return ASEP_OK;
    }
    *out_thresholds = 0;
    for (double& u : h->stage_us) u = 0;
    std::fill(h->host_cnt, h->host_cnt + RELEV_C_SLOTS, 0ull);
    if (h->n == 0) {
        h->finished = true;
        return ASEP_OK;
    }
    const uint32_t n = (uint32_t)h->n;
    const uint32_t n_tiles = (n + RELEV_TILE - 1) / RELEV_TILE;
    h->alt.need(h->n);
    h->table.need((size_t)RELEV_RADIX * n_tiles);
    h->totals.need(4 * RELEV_RADIX);
    h->blk_runs.need(n_tiles);
    h->blk_ones.need(n_tiles);
    for (hipEvent_t& e : h->ev)
        if (!e) ASEP_HIP_CHECK(hipEventCreate(&e));
    ASEP_HIP_CHECK(hipMemsetAsync(h->totals.p, 0, 4 * RELEV_RADIX * sizeof(uint32_t), st));
    ASEP_HIP_CHECK(hipMemsetAsync(h->cnt.p + RELEV_C_T, 0, (RELEV_C_SLOTS - RELEV_C_T) * sizeof(unsigned long long), st));
    int e = 0;
    ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
    uint32_t *src = h->keys.p, *dst = h->alt.p;
    for (int pass = 0; pass < 4; ++pass) {
        uint32_t* totals = h->totals.p + pass * RELEV_RADIX;
        relev_hist_kernel<<<n_tiles, RELEV_BLOCK, 0, st>>>(src, n, 8 * pass, n_tiles, h->table.p, totals);
        ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
        relev_scan_kernel<<<RELEV_RADIX, RELEV_BLOCK, 0, st>>>(h->table.p, totals, n_tiles);
        ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
        relev_scatter_kernel<<<n_tiles, RELEV_BLOCK, 0, st>>>(src, dst, h->table.p, n, 8 * pass, n_tiles);
        ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
        std::swap(src, dst);
    }
    ASEP_HIP_CHECK(hipGetLastError());
    // four passes: the sorted keys are back in h->keys (== src)
    relev_curve_count_kernel<<<n_tiles, RELEV_BLOCK, 0, st>>>(src, n, h->blk_runs.p, h->blk_ones.p);
    ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
    relev_curve_scan_kernel<<<1, RELEV_BLOCK, 0, st>>>(h->blk_runs.p, h->blk_ones.p, n_tiles, h->cnt.p);
    ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
    ASEP_HIP_CHECK(hipGetLastError());
    ASEP_HIP_CHECK(hipMemcpyAsync(h->host_cnt, h->cnt.p, sizeof(h->host_cnt), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    const unsigned long long T = h->host_cnt[RELEV_C_T], P = h->host_cnt[RELEV_C_P];
    if (T < 1 || T > n || P > n) {
        set_error("asep_releval_finish: %llu thresholds and %llu positives of %u pairs: the curve passes are inconsistent", T, P, n);
        return ASEP_ERR_HIP;
    }
    h->thr.need(T);
    h->tps.need(T);
    h->fps.need(T);
    hipEvent_t write_begin = h->ev[RELEV_STAGES + 1];      // (the wait for T is not part of the write stage)
    ASEP_HIP_CHECK(hipEventRecord(write_begin, st));
    relev_curve_write_kernel<<<n_tiles, RELEV_BLOCK, 0, st>>>(src, n, h->blk_runs.p, h->blk_ones.p, (uint32_t)T, (uint32_t)P, h->thr.p,
                                                             h->tps.p, h->fps.p);
    ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
    const unsigned a2_blocks = (unsigned)std::min<unsigned long long>((T + RELEV_BLOCK - 1) / RELEV_BLOCK, 4096ull);
    relev_curve_a2_kernel<<<a2_blocks, RELEV_BLOCK, 0, st>>>(h->tps.p, h->fps.p, (uint32_t)T, h->cnt.p);
    ASEP_HIP_CHECK(hipEventRecord(h->ev[e++], st));
    ASEP_HIP_CHECK(hipGetLastError());
    ASEP_HIP_CHECK(hipMemcpyAsync(h->host_cnt, h->cnt.p, sizeof(h->host_cnt), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    for (int s = 0; s < RELEV_STAGES; ++s) {
        float ms = 0.f;
        ASEP_HIP_CHECK(hipEventElapsedTime(&ms, s == 14 ? write_begin : h->ev[s], h->ev[s + 1]));
        h->stage_us[s] = 1000.0 * ms;
    }
    h->finished = true;
    *out_thresholds = (long long)T;
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_releval_fetch(asep_releval* h, void* stream, float* thresholds, int64_t* tps, int64_t* fps, uint64_t* counters) {
    if (!h || !h->finished) {
        set_error("asep_releval_fetch: call asep_releval_finish first (and after the last append)");
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    hipStream_t st = (hipStream_t)stream;
    const size_t T = (size_t)h->host_cnt[RELEV_C_T];
    if (T) {
        if (thresholds) ASEP_HIP_CHECK(hipMemcpyAsync(thresholds, h->thr.p, T * sizeof(float), hipMemcpyDeviceToHost, st));
        if (tps) ASEP_HIP_CHECK(hipMemcpyAsync(tps, h->tps.p, T * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (fps) ASEP_HIP_CHECK(hipMemcpyAsync(fps, h->fps.p, T * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        ASEP_HIP_CHECK(hipStreamSynchronize(st));
    }
    if (counters) {
        counters[0] = (uint64_t)h->n;
        counters[1] = h->host_cnt[RELEV_C_BAD];
        counters[2] = h->host_cnt[RELEV_C_POS];
        counters[3] = h->host_cnt[RELEV_C_CORRECT];
        counters[4] = h->host_cnt[RELEV_C_BADGT];
        counters[5] = h->host_cnt[RELEV_C_A2];
        counters[6] = h->host_cnt[RELEV_C_T];
        counters[7] = h->host_cnt[RELEV_C_P];
    }
    return ASEP_OK;
    ASEP_GUARD_END
}

double asep_releval_stage_us(const asep_releval* h, int which) {
    if (!h || which < 0 || which >= RELEV_STAGES) return -1.0;
    return h->stage_us[which];
}
