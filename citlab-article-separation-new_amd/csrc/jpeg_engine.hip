// Host side of the JPEG pixels (include/asep_hip.h, "JPEG pixels" block): checks the frame description against itself, so that nothing
// is indexed by a number the caller's file chose alone, lays the component planes out in the handle's scratch arena and queues the
// two kernels of jpeg_kernels.h.  A translation unit and code object of its own: nothing here touches the net engines.
// Host side of the JPEG entropy decode as well ("JPEG entropy decode" block): checks the segments against the scan and the frame, cuts
// them into subsequences and drives the kernels of jpeg_huffman_kernels.h, reading one word back per launch of the fixed-point loop.
#include <algorithm>
#include <string>
#include <vector>

#include "asep_common.h"
#include "jpeg_huffman_kernels.h"
#include "jpeg_kernels.h"

using namespace asep;

namespace {

thread_local std::string g_launches;         // kernels of the calling thread's last call, one name per line

void record(const char* name) { g_launches += name, g_launches += "\n"; }

// the block grid that width, height and sampling imply; false if `in` says anything else
bool consistent(const asep_jpeg_info& in) {
    if (in.width < 1 || in.height < 1 || in.width > 65535 || in.height > 65535) return false;
    if (in.ncomp != 1 && in.ncomp != 3) return false;
    const bool s11 = in.hs == 1 && in.vs == 1, s21 = in.hs == 2 && in.vs == 1, s22 = in.hs == 2 && in.vs == 2;
    if (!(s11 || ((s21 || s22) && in.ncomp == 3))) return false;
    const int mw = (in.width + 8 * in.hs - 1) / (8 * in.hs), mh = (in.height + 8 * in.vs - 1) / (8 * in.vs);
    if (in.mcus_w != mw || in.mcus_h != mh) return false;
    long long blocks = 0;
    for (int c = 0; c < in.ncomp; ++c) {
        if (in.blocks_w[c] != mw * (c == 0 ? in.hs : 1) || in.blocks_h[c] != mh * (c == 0 ? in.vs : 1)) return false;
        if (in.qt_index[c] < 0 || in.qt_index[c] > 3) return false;
        blocks += (long long)in.blocks_w[c] * in.blocks_h[c];
    }
    return in.coef_bytes == blocks * 64 * (long long)sizeof(int16_t);
}

int pixels_dev(asep_post* p, const asep_jpeg_info& in, const int16_t* d_coef, const uint16_t* qt, int order, uint8_t* d_out,
               hipStream_t st) {
    JpegIdctArgs ia{};
    memcpy(ia.qt, qt, sizeof ia.qt);
    ia.ncomp = in.ncomp;
    long long first = 0, plane_bytes = 0;
    uint8_t* planes = nullptr;
    if (in.ncomp == 3) {
        for (int c = 0; c < 3; ++c) plane_bytes += (long long)in.blocks_w[c] * in.blocks_h[c] * 64;
        planes = (uint8_t*)post_pool(p).get((size_t)plane_bytes);
    }
    long long plane_off = 0;
    for (int c = 0; c < in.ncomp; ++c) {
        JpegIdctComp& k = ia.c[c];
        k.coef = d_coef + first * 64;
        k.blocks_w = in.blocks_w[c];
        k.first = (int)first;
        k.qt = in.qt_index[c];
        if (in.ncomp == 1) {
            k.out = d_out, k.stride = in.width, k.crop_w = in.width, k.crop_h = in.height;
        } else {
            k.out = planes + plane_off, k.stride = (long long)in.blocks_w[c] * 8;
            k.crop_w = in.blocks_w[c] * 8, k.crop_h = in.blocks_h[c] * 8;
            plane_off += (long long)in.blocks_w[c] * in.blocks_h[c] * 64;
        }
        first += (long long)in.blocks_w[c] * in.blocks_h[c];
    }
    ia.total = (int)first;                                           // <= 3 * 8192 * 8192 blocks
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)cdiv(ia.total, JPEG_IDCT_BLOCK)), dim3(JPEG_IDCT_BLOCK), 0, st, ia);
    ASEP_HIP_CHECK(hipGetLastError());
    record("jpeg_idct_kernel");
    if (in.ncomp == 1) return ASEP_OK;
    JpegColourArgs ca{};
    ca.y = ia.c[0].out, ca.cb = ia.c[1].out, ca.cr = ia.c[2].out;
    ca.out = d_out;
    ca.y_stride = in.blocks_w[0] * 8, ca.c_stride = in.blocks_w[1] * 8;
    ca.W = in.width, ca.H = in.height;
    ca.hs = in.hs, ca.vs = in.vs;
    ca.dw = (in.width + in.hs - 1) / in.hs, ca.dh = (in.height + in.vs - 1) / in.vs;
    ca.order = order;
    ca.groups_w = cdiv(in.width, JPEG_COLOUR_PIX);
    const long long threads = (long long)ca.groups_w * in.height;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((threads + JPEG_COLOUR_BLOCK - 1) / JPEG_COLOUR_BLOCK)), dim3(JPEG_COLOUR_BLOCK),
                       0, st, ca);
    ASEP_HIP_CHECK(hipGetLastError());
    record("jpeg_colour_kernel");
    return ASEP_OK;
}

int check_args(const char* fn, asep_post* p, const asep_jpeg_info* info, const void* coef, const uint16_t* qt, int order, const void* out) {
    if (!p || !info || !coef || !qt || !out) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    if (order != ASEP_JPEG_ORDER_GRAY && order != ASEP_JPEG_ORDER_BGR && order != ASEP_JPEG_ORDER_RGB) {
        set_error("%s: order %d: ASEP_JPEG_ORDER_GRAY, _BGR and _RGB are served", fn, order);
        return ASEP_ERR_ARG;
    }
    if (!consistent(*info)) {
        set_error("%s: the frame description contradicts itself (%d x %d, %d components, sampling %d x %d, %lld coefficient bytes)", fn,
                  info->width, info->height, info->ncomp, info->hs, info->vs, (long long)info->coef_bytes);
        return ASEP_ERR_ARG;
    }
    return ASEP_OK;
}

size_t out_bytes(const asep_jpeg_info& in, int order) {
    return (size_t)in.width * in.height * (in.ncomp == 1 || order == ASEP_JPEG_ORDER_GRAY ? 1 : 3);
}

}  // namespace

int asep_jpeg_pixels_dev(asep_post* p, const asep_jpeg_info* info, const int16_t* d_coef, const uint16_t* qt, int order, uint8_t* d_out,
                         void* stream) {
    if (int rc = check_args("asep_jpeg_pixels_dev", p, info, d_coef, qt, order, d_out)) return rc;
    ASEP_GUARD_BEGIN
    g_launches.clear();
    post_pool(p).begin();
    return pixels_dev(p, *info, d_coef, qt, order, d_out, (hipStream_t)stream);
    ASEP_GUARD_END
}

int asep_jpeg_pixels(asep_post* p, const asep_jpeg_info* info, const int16_t* coef, const uint16_t* qt, int order, uint8_t* out) {
    if (int rc = check_args("asep_jpeg_pixels", p, info, coef, qt, order, out)) return rc;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    g_launches.clear();
    pool.begin();
    int16_t* d_coef = (int16_t*)pool.get((size_t)info->coef_bytes);
    const size_t nout = out_bytes(*info, order);
    uint8_t* d_out = (uint8_t*)pool.get(nout);
    ASEP_HIP_CHECK(hipMemcpyAsync(d_coef, coef, (size_t)info->coef_bytes, hipMemcpyHostToDevice, st));
    if (int rc = pixels_dev(p, *info, d_coef, qt, order, d_out, st)) return rc;
    ASEP_HIP_CHECK(hipMemcpyAsync(out, d_out, nout, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    return ASEP_OK;
    ASEP_GUARD_END
}

// ---- the entropy decode ----------------------------------------------------------------------------------------------------------------
namespace {

thread_local int g_rounds = 0, g_subs = 0;   // of the calling thread's last entropy call
thread_local int g_max_rounds = 0;           // a lower cap of rounds for the calling thread's calls, 0 = none

template <int KIND>
int segmented_sums(const JpegHuffArgs& h, BufferPool& pool, long long longest, int comps, hipStream_t st, const char* name) {
    JpegScanArgs sa{};
    sa.h = h;
    sa.chunks = (int)((longest + JPEG_SCAN_CHUNK - 1) / JPEG_SCAN_CHUNK);
    int32_t* words = (int32_t*)pool.get((size_t)3 * comps * sa.chunks * sizeof(int32_t));
    sa.chunk_sum = words, sa.chunk_head = words + (size_t)comps * sa.chunks, sa.chunk_carry = words + (size_t)2 * comps * sa.chunks;
    const dim3 grid((unsigned)sa.chunks, (unsigned)comps);
    hipLaunchKernelGGL((jpeg_huff_scan_kernel<KIND, 0>), grid, dim3(JPEG_SCAN_BLOCK), 0, st, sa);
    hipLaunchKernelGGL((jpeg_huff_carry_kernel<KIND>), dim3((unsigned)comps), dim3(JPEG_SCAN_BLOCK), 0, st, sa);
    hipLaunchKernelGGL((jpeg_huff_scan_kernel<KIND, 2>), grid, dim3(JPEG_SCAN_BLOCK), 0, st, sa);
    ASEP_HIP_CHECK(hipGetLastError());
    record(name), record("jpeg_huff_carry_kernel"), record(name);
    return ASEP_OK;
}

// d_scan, d_coef, d_status: device; tables, segments: host.  Blocks on st (at least once: what it uploads lives on this stack).
int entropy_dev(asep_post* p, const asep_jpeg_info& in, const uint8_t* d_scan, size_t scan_bytes, const asep_jpeg_scan_tables* tables,
                const asep_jpeg_segment* segments, int n_segments, int subseq_bits, int16_t* d_coef, int32_t* d_status, hipStream_t st) {
    const char* fn = "asep_jpeg_entropy";
    if (subseq_bits == 0) subseq_bits = ASEP_JPEG_SUBSEQ_BITS_DEFAULT;
    if (subseq_bits < 64 || subseq_bits % 32 || subseq_bits > (1 << 20)) {
        set_error("%s: subseq_bits %d: a multiple of 32 from 64 to 2^20, or 0 for the default", fn, subseq_bits);
        return ASEP_ERR_ARG;
    }
    if (scan_bytes == 0 || scan_bytes >= ((size_t)1 << 28) || (reinterpret_cast<uintptr_t>(d_scan) & 3)) {
        set_error("%s: a scan of %zu bytes at %p: 1 .. 2^28 - 1 bytes, 4-byte aligned", fn, scan_bytes, (const void*)d_scan);
        return ASEP_ERR_ARG;
    }
    const int bpm = in.ncomp == 1 ? 1 : in.hs * in.vs + 2;
    const long long mcus = (long long)in.mcus_w * in.mcus_h;
    const long long want = in.restart_interval > 0 ? (mcus + in.restart_interval - 1) / in.restart_interval : 1;
    if (in.restart_interval < 0 || n_segments != want) {
        set_error("%s: %d segments for %lld MCUs at restart interval %d", fn, n_segments, mcus, in.restart_interval);
        return ASEP_ERR_ARG;
    }
    // the segments lie back to back in the scan and count the frame's MCUs: nothing the kernels index comes from the file alone
    std::vector<JpegHuffSeg> segs((size_t)n_segments);
    long long next_byte = 0, next_mcu = 0, subs = 0, longest = 0;
    for (int i = 0; i < n_segments; ++i) {
        const asep_jpeg_segment& s = segments[i];
        const long long n_mcus = i == n_segments - 1 ? mcus - next_mcu : in.restart_interval;
        if (s.byte_offset != next_byte || s.byte_length == 0 || next_byte + s.byte_length > (long long)scan_bytes || s.first_mcu != next_mcu ||
            s.n_mcus != n_mcus) {
            set_error("%s: segment %d (bytes %u + %u, MCUs %u + %u) does not continue the scan of %zu bytes and %lld MCUs", fn, i, s.byte_offset,
                      s.byte_length, s.first_mcu, s.n_mcus, scan_bytes, mcus);
            return ASEP_ERR_ARG;
        }
        const long long n_sub = ((long long)s.byte_length * 8 + subseq_bits - 1) / subseq_bits;
        segs[i] = JpegHuffSeg{(uint32_t)(next_byte * 8), (uint32_t)((next_byte + s.byte_length) * 8), (uint32_t)(next_mcu * bpm),
                              (uint32_t)(n_mcus * bpm), (uint32_t)subs};
        subs += n_sub, longest = std::max(longest, n_sub);
        next_byte += s.byte_length, next_mcu += n_mcus;
    }
    if (next_byte != (long long)scan_bytes) {
        set_error("%s: the segments cover %lld of the scan's %zu bytes", fn, next_byte, scan_bytes);
        return ASEP_ERR_ARG;
    }
    BufferPool& pool = post_pool(p);
    JpegHuffArgs h{};
    h.scan = reinterpret_cast<const uint32_t*>(d_scan);
    h.n_words = (uint32_t)((scan_bytes + 3) / 4);
    asep_jpeg_scan_tables* d_tables = (asep_jpeg_scan_tables*)pool.get(sizeof(asep_jpeg_scan_tables));
    JpegHuffSeg* d_segs = (JpegHuffSeg*)pool.get(segs.size() * sizeof(JpegHuffSeg));
    h.tables = d_tables, h.segs = d_segs;
    h.n_segs = n_segments, h.n_subs = (int)subs, h.subseq_bits = subseq_bits;
    h.ncomp = in.ncomp, h.hs = in.hs, h.vs = in.vs, h.bpm = bpm, h.mcus_w = in.mcus_w;
    h.restart_interval = in.restart_interval;
    long long blocks = 0, most = 0;
    for (int c = 0; c < in.ncomp; ++c) {
        h.blocks_w[c] = in.blocks_w[c];
        h.plane_off[c] = blocks * 64;
        h.comp_blocks[c] = (long long)in.blocks_w[c] * in.blocks_h[c];
        blocks += h.comp_blocks[c], most = std::max(most, h.comp_blocks[c]);
    }
    h.entry = (unsigned long long*)pool.get((size_t)subs * 8);
    h.exit_ = (unsigned long long*)pool.get((size_t)subs * 8);
    h.sub_seg = (uint32_t*)pool.get((size_t)subs * 4);
    h.count = (int32_t*)pool.get((size_t)subs * 4);
    h.first_block = (int32_t*)pool.get((size_t)subs * 4);
    h.changed = (int32_t*)pool.get(sizeof(int32_t));
    h.coef = d_coef, h.status = d_status;

    ASEP_HIP_CHECK(hipMemcpyAsync(d_tables, tables, sizeof *tables, hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(JpegHuffSeg), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    ASEP_HIP_CHECK(hipMemsetAsync(d_coef, 0, (size_t)in.coef_bytes, st));
    const dim3 grid((unsigned)((subs + JPEG_HUFF_BLOCK - 1) / JPEG_HUFF_BLOCK)), block(JPEG_HUFF_BLOCK);
    hipLaunchKernelGGL(jpeg_huff_sync_kernel<true>, grid, block, 0, st, h, 0);
    ASEP_HIP_CHECK(hipGetLastError());
    record("jpeg_huff_sync_kernel<speculate>");
    g_subs = (int)subs, g_rounds = 0;
    // The loop's bound.  A launch sees everything earlier launches stored; inside a launch a workgroup may run before the neighbour
    // whose last exit it reads, so rounds carry correctness forward only inside a workgroup.  Where one workgroup holds everything,
    // longest - 1 rounds make the longest segment right.  Else a launch of JPEG_HUFF_BLOCK rounds moves the front of what is right
    // to the next workgroup's start at the least (from a workgroup's start: through the whole workgroup), and a segment touches at
    // most ceil(longest / JPEG_HUFF_BLOCK) + 1 workgroups: so many full launches make it right.  Then one launch of one round
    // confirms; if even that one changes something, or the test cap runs out first, the status is "not converged".
    static_assert(ASEP_JPEG_SYNC_INNER_MAX == JPEG_HUFF_BLOCK, "a full launch carries correctness through a whole workgroup");
    const bool one_group = subs <= JPEG_HUFF_BLOCK;
    const long long need = one_group ? longest - 1 : (longest + JPEG_HUFF_BLOCK - 1) / JPEG_HUFF_BLOCK + 1;     // rounds, or full launches
    bool converged = longest == 1;                                   // every subsequence starts its segment: nothing was guessed
    bool confirmed = false;
    long long rounds = 0, sure = 0;
    int inner = ASEP_JPEG_SYNC_INNER;                                // doubled per launch: a stream that does not synchronise itself costs few launches
    while (!converged && !confirmed && (g_max_rounds == 0 || rounds < g_max_rounds)) {
        const bool confirming = sure >= need;
        int r = confirming ? 1 : (one_group ? (int)std::min<long long>(inner, need - sure) : inner);
        if (g_max_rounds > 0) r = (int)std::min<long long>(r, g_max_rounds - rounds);
        inner = std::min(2 * inner, ASEP_JPEG_SYNC_INNER_MAX);
        int32_t changed = 0;
        ASEP_HIP_CHECK(hipMemsetAsync(h.changed, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(jpeg_huff_sync_kernel<false>, grid, block, 0, st, h, r);
        ASEP_HIP_CHECK(hipGetLastError());
        record("jpeg_huff_sync_kernel");
        ASEP_HIP_CHECK(hipMemcpyAsync(&changed, h.changed, sizeof changed, hipMemcpyDeviceToHost, st));
        ASEP_HIP_CHECK(hipStreamSynchronize(st));
        rounds += r;
        converged = changed == 0;
        confirmed = confirming;
        sure += one_group ? r : (r == JPEG_HUFF_BLOCK ? 1 : 0);
    }
    g_rounds = (int)rounds;
    if (!converged) {
        static const int32_t not_converged = ASEP_JPEG_STATUS_NOT_CONVERGED;
        ASEP_HIP_CHECK(hipMemcpyAsync(d_status, &not_converged, sizeof not_converged, hipMemcpyHostToDevice, st));
        ASEP_HIP_CHECK(hipStreamSynchronize(st));
        return ASEP_OK;
    }
    if (int rc = segmented_sums<JPEG_SCAN_PLACE>(h, pool, subs, 1, st, "jpeg_huff_scan_kernel<place>")) return rc;
    hipLaunchKernelGGL(jpeg_huff_write_kernel, grid, block, 0, st, h);
    ASEP_HIP_CHECK(hipGetLastError());
    record("jpeg_huff_write_kernel");
    if (int rc = segmented_sums<JPEG_SCAN_DC>(h, pool, most, in.ncomp, st, "jpeg_huff_scan_kernel<dc>")) return rc;
    hipLaunchKernelGGL(jpeg_huff_energy_kernel, dim3((unsigned)((blocks + JPEG_SCAN_BLOCK - 1) / JPEG_SCAN_BLOCK)), dim3(JPEG_SCAN_BLOCK), 0, st,
                       h, in.qt_index[0], in.qt_index[in.ncomp > 1 ? 1 : 0], in.qt_index[in.ncomp > 2 ? 2 : 0], blocks);
    ASEP_HIP_CHECK(hipGetLastError());
    record("jpeg_huff_energy_kernel");
    if (longest == 1) ASEP_HIP_CHECK(hipStreamSynchronize(st));      // the uploads above read this stack
    return ASEP_OK;
}

int check_entropy_args(const char* fn, asep_post* p, const asep_jpeg_info* info, const void* scan, const void* tables, const void* segments,
                       const void* coef, const void* status) {
    if (!p || !info || !scan || !tables || !segments || !coef || !status) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    if (!consistent(*info)) {
        set_error("%s: the frame description contradicts itself (%d x %d, %d components, sampling %d x %d, %lld coefficient bytes)", fn,
                  info->width, info->height, info->ncomp, info->hs, info->vs, (long long)info->coef_bytes);
        return ASEP_ERR_ARG;
    }
    return ASEP_OK;
}

}  // namespace

int asep_jpeg_entropy_dev(asep_post* p, const asep_jpeg_info* info, const uint8_t* d_scan, size_t scan_bytes,
                          const asep_jpeg_scan_tables* tables, const asep_jpeg_segment* segments, int n_segments, int subseq_bits,
                          int16_t* d_coef, int32_t* d_status, void* stream) {
    if (int rc = check_entropy_args("asep_jpeg_entropy_dev", p, info, d_scan, tables, segments, d_coef, d_status)) return rc;
    ASEP_GUARD_BEGIN
    g_launches.clear();
    post_pool(p).begin();
    return entropy_dev(p, *info, d_scan, scan_bytes, tables, segments, n_segments, subseq_bits, d_coef, d_status, (hipStream_t)stream);
    ASEP_GUARD_END
}

int asep_jpeg_entropy(asep_post* p, const asep_jpeg_info* info, const uint8_t* scan, size_t scan_bytes,
                      const asep_jpeg_scan_tables* tables, const asep_jpeg_segment* segments, int n_segments, int subseq_bits,
                      int16_t* coef, int32_t* status) {
    if (int rc = check_entropy_args("asep_jpeg_entropy", p, info, scan, tables, segments, coef, status)) return rc;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    g_launches.clear();
    pool.begin();
    if (scan_bytes == 0) {
        set_error("asep_jpeg_entropy: an empty scan");
        return ASEP_ERR_ARG;
    }
    const size_t padded = (scan_bytes + 3) & ~(size_t)3;
    uint8_t* d_scan = (uint8_t*)pool.get(padded);
    int16_t* d_coef = (int16_t*)pool.get((size_t)info->coef_bytes);
    int32_t* d_status = (int32_t*)pool.get(sizeof(int32_t));
    ASEP_HIP_CHECK(hipMemsetAsync(d_scan + padded - 4, 0, 4, st));   // the last word's padding
    ASEP_HIP_CHECK(hipMemcpyAsync(d_scan, scan, scan_bytes, hipMemcpyHostToDevice, st));
    if (int rc = entropy_dev(p, *info, d_scan, scan_bytes, tables, segments, n_segments, subseq_bits, d_coef, d_status, st)) return rc;
    ASEP_HIP_CHECK(hipMemcpyAsync(coef, d_coef, (size_t)info->coef_bytes, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(status, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    return ASEP_OK;
    ASEP_GUARD_END
}

void asep_jpeg_entropy_set_max_rounds(int max_rounds) { g_max_rounds = max_rounds > 0 ? max_rounds : 0; }

int asep_jpeg_entropy_last_rounds(int* n_subsequences) {
    if (n_subsequences) *n_subsequences = g_subs;
    return g_rounds;
}

long asep_jpeg_last_launches(char* buf, size_t max_bytes) {
    if (buf && max_bytes) {
        const size_t n = std::min(max_bytes - 1, g_launches.size());
        memcpy(buf, g_launches.data(), n);
        buf[n] = 0;
    }
    return (long)g_launches.size();
}
