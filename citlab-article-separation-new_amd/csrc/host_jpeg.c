/* libasep_host.so: the sequential half of a JPEG decode (include/asep_host.h).  Only the Huffman decode of a baseline JPEG has to
 * run on one CPU thread; dequantisation, the inverse DCT, chroma upsampling and the colour conversion run on the device
 * (csrc/jpeg_engine.hip).  This file parses the markers, refuses every flavour the device path does not restate (the caller hands
 * those files to Pillow) and writes the quantised coefficients, DC prediction undone, block by block in natural order.
 *
 * Every read is checked against the length of the file, every write against the coefficient size that the probe computed from the
 * frame header; nothing is allocated here. */
#include <string.h>

#include "../../include/asep_host.h"

/* zig-zag position -> natural (row-major) position, ITU-T T.81 figure A.6 */
static const uint8_t NATURAL[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

#define LOOK_BITS 9

typedef struct {
    int defined;
    uint16_t look[1 << LOOK_BITS];   /* (length << 8) | symbol of the code that starts with these bits, 0 = longer than LOOK_BITS */
    int32_t maxcode[18];             /* largest code of each length, -1 = none */
    int32_t valoff[17];              /* index of a length's first symbol minus its first code */
    uint8_t sym[256];
    int nsym;
} huff_table;

typedef struct {
    asep_jpeg_info info;
    uint16_t qt[4][64];              /* natural order */
    int qt_defined[4];
    huff_table dc[4], ac[4];
    int td[3], ta[3];                /* tables of the scan's components */
    size_t scan_begin;               /* first byte of the entropy-coded segment */
} jpeg_header;

static unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

static int build_table(huff_table* t, const uint8_t* counts, const uint8_t* symbols, int nsym) {
    memset(t, 0, sizeof *t);
    memcpy(t->sym, symbols, (size_t)nsym);
    t->nsym = nsym;
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->valoff[l] = k - code;
        for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return ASEP_JPEG_DAMAGED;          /* more codes than the length has */
            if (l <= LOOK_BITS) {
                const int first = code << (LOOK_BITS - l);
                for (int j = 0; j < (1 << (LOOK_BITS - l)); ++j) t->look[first + j] = (uint16_t)((l << 8) | symbols[k]);
            }
        }
        t->maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[17] = 0x7fffffff;
    t->defined = 1;
    return 0;
}

/* The orientation of an EXIF block (after "Exif\0\0"): 0 = the tag is absent, 1..65535 its value, -1 = the block cannot be parsed. */
static int exif_orientation(const uint8_t* t, size_t n) {
    if (n < 8) return -1;
    int le;
    if (t[0] == 'I' && t[1] == 'I') le = 1;
    else if (t[0] == 'M' && t[1] == 'M') le = 0;
    else return -1;
#define RD16(o) (le ? (unsigned)t[o] | ((unsigned)t[(o) + 1] << 8) : ((unsigned)t[o] << 8) | t[(o) + 1])
#define RD32(o) (le ? (uint32_t)RD16(o) | ((uint32_t)RD16((o) + 2) << 16) : ((uint32_t)RD16(o) << 16) | RD16((o) + 2))
    if (RD16(2) != 42) return -1;
    const uint32_t ifd = RD32(4);
    if (ifd > n || n - ifd < 2) return -1;
    const unsigned count = RD16(ifd);
    if ((n - ifd - 2) / 12 < count) return -1;
    for (unsigned i = 0; i < count; ++i) {
        const size_t e = (size_t)ifd + 2 + 12 * (size_t)i;
        if (RD16(e) != 0x0112) continue;
        if (RD16(e + 2) != 3 || RD32(e + 4) != 1) return -1;         /* anything but one SHORT: leave it to Pillow */
        return (int)RD16(e + 8);
    }
    return 0;
#undef RD16
#undef RD32
}

static int contains(const uint8_t* p, size_t n, const char* word) {
    const size_t m = strlen(word);
    for (size_t i = 0; i + m <= n; ++i)
        if (p[i] == (uint8_t)word[0] && memcmp(p + i, word, m) == 0) return 1;
    return 0;
}

/* SOI .. SOS of the one scan.  0, ASEP_JPEG_REFUSED for a flavour that is left to Pillow, ASEP_JPEG_DAMAGED for a stream that ends early
 * or contradicts itself. */
static int parse_header(const uint8_t* b, size_t n, jpeg_header* h) {
    memset(h, 0, sizeof *h);
    if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) return ASEP_JPEG_REFUSED;
    size_t pos = 2;
    int saw_sof = 0, saw_jfif = 0, saw_adobe = 0, adobe_transform = 0, saw_exif = 0;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0};
    asep_jpeg_info* in = &h->info;
    for (;;) {
        if (n - pos < 2) return ASEP_JPEG_DAMAGED;
        if (b[pos] != 0xFF) return ASEP_JPEG_DAMAGED;
        while (pos + 1 < n && b[pos + 1] == 0xFF) ++pos;             /* fill bytes in front of a marker */
        if (n - pos < 2) return ASEP_JPEG_DAMAGED;
        const int m = b[pos + 1];
        pos += 2;
        if (m == 0xD8 || m == 0xD9 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return ASEP_JPEG_DAMAGED;
        if (n - pos < 2) return ASEP_JPEG_DAMAGED;
        const size_t len = be16(b + pos);
        if (len < 2 || n - pos < len) return ASEP_JPEG_DAMAGED;
        const uint8_t* s = b + pos + 2;
        const size_t sl = len - 2;
        pos += len;
        if (m == 0xC0 || m == 0xC1) {                                /* baseline / extended sequential, Huffman */
            if (saw_sof) return ASEP_JPEG_REFUSED;
            saw_sof = 1;
            if (sl < 6) return ASEP_JPEG_DAMAGED;
            if (s[0] != 8) return ASEP_JPEG_REFUSED;                 /* 12-bit samples */
            in->height = (int32_t)be16(s + 1);
            in->width = (int32_t)be16(s + 3);
            in->ncomp = s[5];
            if (in->height == 0) return ASEP_JPEG_REFUSED;           /* the height follows in a DNL segment */
            if (in->width == 0) return ASEP_JPEG_DAMAGED;
            if (in->ncomp != 1 && in->ncomp != 3) return ASEP_JPEG_REFUSED;
            if (sl != 6 + 3 * (size_t)in->ncomp) return ASEP_JPEG_DAMAGED;
            for (int c = 0; c < in->ncomp; ++c) {
                comp_id[c] = s[6 + 3 * c];
                comp_h[c] = s[7 + 3 * c] >> 4;
                comp_v[c] = s[7 + 3 * c] & 15;
                in->qt_index[c] = s[8 + 3 * c];
                if (in->qt_index[c] > 3) return ASEP_JPEG_DAMAGED;
                for (int d = 0; d < c; ++d)
                    if (comp_id[d] == comp_id[c]) return ASEP_JPEG_DAMAGED;
            }
            if (in->ncomp == 1) {
                if (comp_h[0] != 1 || comp_v[0] != 1) return ASEP_JPEG_REFUSED;
            } else {
                if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return ASEP_JPEG_REFUSED;
                if (!((comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 2)))
                    return ASEP_JPEG_REFUSED;
            }
            in->hs = comp_h[0];
            in->vs = comp_v[0];
        } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8) || m == 0xDC) {
            return ASEP_JPEG_REFUSED;                                /* progressive, lossless, arithmetic, DNL */
        } else if (m == 0xC4) {                                      /* DHT */
            size_t o = 0;
            while (o < sl) {
                if (sl - o < 17) return ASEP_JPEG_DAMAGED;
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return ASEP_JPEG_DAMAGED;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
                if (total > 256 || sl - o - 17 < (size_t)total) return ASEP_JPEG_DAMAGED;
                const int rc = build_table(tc ? &h->ac[th] : &h->dc[th], s + o + 1, s + o + 17, total);
                if (rc) return rc;
                o += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {                                      /* DQT */
            size_t o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq == 1) return ASEP_JPEG_REFUSED;               /* 16-bit tables */
                if (pq > 1 || tq > 3 || sl - o < 65) return ASEP_JPEG_DAMAGED;
                for (int i = 0; i < 64; ++i) h->qt[tq][NATURAL[i]] = s[o + 1 + i];
                h->qt_defined[tq] = 1;
                o += 65;
            }
        } else if (m == 0xDD) {                                      /* DRI */
            if (sl != 2) return ASEP_JPEG_DAMAGED;
            in->restart_interval = (int32_t)be16(s);
        } else if (m == 0xE0) {
            if (sl >= 14 && memcmp(s, "JFIF", 5) == 0) saw_jfif = 1;     /* libjpeg takes a shorter APP0 for no JFIF marker */
        } else if (m == 0xE1) {
            if (sl >= 6 && memcmp(s, "Exif\0", 6) == 0) {
                if (saw_exif) return ASEP_JPEG_REFUSED;
                saw_exif = 1;
                const int o = exif_orientation(s + 6, sl - 6);
                if (o != 0 && o != 1) return ASEP_JPEG_REFUSED;      /* the loaders apply it (exif_transpose) */
            } else if (contains(s, sl, "Orientation")) {
                return ASEP_JPEG_REFUSED;                            /* an XMP packet's tiff:Orientation counts where EXIF has none */
            }
        } else if (m == 0xE2) {
            if (sl >= 4 && memcmp(s, "MPF", 4) == 0) return ASEP_JPEG_REFUSED;   /* multi-picture files */
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
                saw_adobe = 1;
                adobe_transform = s[11];
            }
        } else if (m == 0xDA) {                                      /* SOS: the one scan */
            if (!saw_sof) return ASEP_JPEG_DAMAGED;
            if (sl < 1) return ASEP_JPEG_DAMAGED;
            if (s[0] != in->ncomp) return ASEP_JPEG_REFUSED;         /* one of several scans */
            if (sl != 4 + 2 * (size_t)in->ncomp) return ASEP_JPEG_DAMAGED;
            for (int c = 0; c < in->ncomp; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return ASEP_JPEG_REFUSED;        /* another component order */
                h->td[c] = s[2 + 2 * c] >> 4;
                h->ta[c] = s[2 + 2 * c] & 15;
                if (h->td[c] > 3 || h->ta[c] > 3) return ASEP_JPEG_DAMAGED;
                if (!h->dc[h->td[c]].defined || !h->ac[h->ta[c]].defined || !h->qt_defined[in->qt_index[c]]) return ASEP_JPEG_DAMAGED;
            }
            const uint8_t* t = s + 1 + 2 * in->ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return ASEP_JPEG_REFUSED;
            break;
        }
        /* COM and the other APPn segments: skipped */
    }
    if (in->ncomp == 3) {
        if (saw_adobe && adobe_transform != 1) return ASEP_JPEG_REFUSED;
        if (!saw_jfif && !saw_adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return ASEP_JPEG_REFUSED;
    }
    const int32_t mcu_w = 8 * in->hs, mcu_h = 8 * in->vs;
    in->mcus_w = (in->width + mcu_w - 1) / mcu_w;
    in->mcus_h = (in->height + mcu_h - 1) / mcu_h;
    int64_t blocks = 0;
    for (int c = 0; c < in->ncomp; ++c) {
        in->blocks_w[c] = in->mcus_w * (c == 0 ? in->hs : 1);
        in->blocks_h[c] = in->mcus_h * (c == 0 ? in->vs : 1);
        blocks += (int64_t)in->blocks_w[c] * in->blocks_h[c];
    }
    in->coef_bytes = blocks * 64 * (int64_t)sizeof(int16_t);
    h->scan_begin = pos;
    /* a block takes at least two bits (one DC code, one end-of-block code): a frame the file cannot hold is a damaged or crafted header */
    if (blocks > 4 * (int64_t)(n - pos)) return ASEP_JPEG_DAMAGED;
    return 0;
}

int asep_jpeg_probe(const uint8_t* bytes, size_t n, asep_jpeg_info* info) {
    if (!bytes || !info) return ASEP_JPEG_ARG;
    jpeg_header h;
    const int rc = parse_header(bytes, n, &h);
    if (rc) {
        memset(info, 0, sizeof *info);
        return rc;
    }
    *info = h.info;
    return 0;
}

/* ---- the entropy-coded segment ---------------------------------------------------------------------------------------------- */
typedef struct {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;                    /* the next bits, left-aligned; below the `bits` real ones it holds zeros */
    int bits;
} bit_reader;

/* Takes bytes until 57 bits are there, a marker stands in front, or the file ends; 0xFF00 is the byte 0xFF. */
static void fill(bit_reader* r) {
    while (r->bits <= 56) {
        if (r->p >= r->end) return;
        unsigned v = *r->p;
        if (v == 0xFF) {
            if (r->end - r->p < 2 || r->p[1] != 0) return;           /* a marker (or fill bytes in front of one), or the end */
            r->p += 2;
        } else {
            r->p += 1;
        }
        r->acc |= (uint64_t)v << (56 - r->bits);
        r->bits += 8;
    }
}

static inline int take(bit_reader* r, int k) {                       /* drops k bits; -1 if the segment does not hold them */
    if (k > r->bits) return -1;
    r->acc <<= k;
    r->bits -= k;
    return 0;
}

static inline int decode_symbol(bit_reader* r, const huff_table* t) {
    const unsigned e = t->look[r->acc >> (64 - LOOK_BITS)];
    if (e) return take(r, (int)(e >> 8)) ? -1 : (int)(e & 255);
    for (int l = LOOK_BITS + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(r->acc >> (64 - l));
        if (code <= t->maxcode[l]) {
            const int32_t i = code + t->valoff[l];
            if (i < 0 || i >= t->nsym || take(r, l)) return -1;
            return t->sym[i];
        }
    }
    return -1;                                                       /* a code that the table does not hold */
}

static inline int receive_extend(bit_reader* r, int s, int* out) {   /* T.81 F.2.2.1: s further bits as a signed value */
    const int v = (int)(r->acc >> (64 - s));
    if (take(r, s)) return -1;
    *out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    return 0;
}

/* The largest sum of squared dequantised coefficients a block may have.  The judge is libjpeg-turbo's SIMD inverse DCT, which keeps the
 * dequantised values, the values between its two passes and their pairwise sums in 16-bit lanes; the device kernel works in int32.  Both
 * are exact, and so equal, while nothing leaves its lanes.  With E the sum of squares: a value between the passes is 4 sqrt(8) times an
 * entry of the half-transformed block, whose norm is sqrt(E) (the transform is orthonormal), so it stays below 11.32 sqrt(E) and a sum
 * of two of them below 16 sqrt(E); for sqrt(E) <= 2000 that is 32000 < 2^15, and the int32 sums stay below 2.83 * 11.32 * 2000 * 25172
 * < 2^31.  Samples of 8 bits give sqrt(E) <= 1024 plus the quantisation error of at most 4 q, so every block an encoder can produce with
 * table entries up to 244 passes; what does not pass is left to Pillow like any other refused file. */
#define MAX_BLOCK_ENERGY 4000000

static int decode_block(bit_reader* r, const huff_table* dc, const huff_table* ac, const uint16_t* q, int* pred, int16_t* blk) {
    int64_t energy;
    memset(blk, 0, 64 * sizeof(int16_t));
    if (r->bits < 32) fill(r);
    int s = decode_symbol(r, dc);
    if (s < 0 || s > 11) return -1;
    if (s) {
        int d;
        if (receive_extend(r, s, &d)) return -1;
        *pred += d;
        if (*pred < -2048 || *pred > 2047) return -1;                /* beyond what 8-bit samples can give */
    }
    blk[0] = (int16_t)*pred;
    energy = (int64_t)*pred * q[0] * *pred * q[0];
    for (int k = 1; k < 64;) {
        if (r->bits < 32) fill(r);
        const int rs = decode_symbol(r, ac);
        if (rs < 0) return -1;
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (run == 0) break;                                     /* end of block */
            if (run != 15) return -1;                                /* end-of-band runs belong to progressive scans */
            k += 16;
            if (k > 64) return -1;
            continue;
        }
        k += run;
        if (k > 63 || s > 10) return -1;
        int v;
        if (receive_extend(r, s, &v)) return -1;
        blk[NATURAL[k]] = (int16_t)v;
        energy += (int64_t)v * q[NATURAL[k]] * v * q[NATURAL[k]];
        ++k;
    }
    if (energy > MAX_BLOCK_ENERGY) return -2;                        /* beyond what 8-bit samples give: see MAX_BLOCK_ENERGY */
    return 0;
}

/* The marker in front of the reader, fill bytes skipped; -1 if there is none.  At most 7 padding bits may be left in the reader. */
static int next_marker(bit_reader* r) {
    fill(r);
    if (r->bits >= 8) return -1;                                     /* whole bytes where the marker belongs */
    r->acc = 0;
    r->bits = 0;
    if (r->end - r->p < 2 || r->p[0] != 0xFF) return -1;
    while (r->end - r->p >= 2 && r->p[1] == 0xFF) ++r->p;
    if (r->end - r->p < 2) return -1;
    const int m = r->p[1];
    r->p += 2;
    return m;
}

int asep_jpeg_entropy_decode(const uint8_t* bytes, size_t n, const asep_jpeg_info* info, int16_t* coef, uint16_t qt[4][64]) {
    if (!bytes || !info || !coef || !qt) return ASEP_JPEG_ARG;
    jpeg_header h;
    int rc = parse_header(bytes, n, &h);
    if (rc) return rc;
    if (memcmp(&h.info, info, sizeof *info) != 0) return ASEP_JPEG_ARG;      /* not the probe of these bytes */
    const asep_jpeg_info* in = &h.info;
    int16_t* plane[3];
    int64_t off = 0;
    for (int c = 0; c < in->ncomp; ++c) {
        plane[c] = coef + off;
        off += (int64_t)in->blocks_w[c] * in->blocks_h[c] * 64;
    }
    bit_reader r = {bytes + h.scan_begin, bytes + n, 0, 0};
    int pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)in->mcus_w * in->mcus_h;
    int64_t to_restart = in->restart_interval;
    int expect = 0;
    rc = 0;
    int32_t mx = 0, my = 0;
    for (int64_t i = 0; i < mcus && !rc; ++i) {
        if (in->restart_interval && to_restart == 0) {
            if (next_marker(&r) != 0xD0 + expect) { rc = ASEP_JPEG_DAMAGED; break; }
            expect = (expect + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
            to_restart = in->restart_interval;
        }
        --to_restart;
        for (int c = 0; c < in->ncomp && !rc; ++c) {
            const int ch = c == 0 ? in->hs : 1, cv = c == 0 ? in->vs : 1;
            for (int v = 0; v < cv && !rc; ++v)
                for (int u = 0; u < ch; ++u) {
                    const int64_t blk = ((int64_t)my * cv + v) * in->blocks_w[c] + (int64_t)mx * ch + u;
                    if (blk < 0 || (blk + 1) * 64 * (int64_t)sizeof(int16_t) > in->coef_bytes) { rc = ASEP_JPEG_DAMAGED; break; }
                    const int e = decode_block(&r, &h.dc[h.td[c]], &h.ac[h.ta[c]], h.qt[in->qt_index[c]], &pred[c], plane[c] + blk * 64);
                    if (e) { rc = e == -2 ? ASEP_JPEG_REFUSED : ASEP_JPEG_DAMAGED; break; }
                }
        }
        if (++mx == in->mcus_w) mx = 0, ++my;
    }
    if (!rc) {
        const int m = next_marker(&r);
        if (m == 0xDA || m == 0xDC || m == 0xC4 || m == 0xDB || m == 0xDD) rc = ASEP_JPEG_REFUSED;   /* further scans, DNL */
        else if (m != 0xD9) rc = ASEP_JPEG_DAMAGED;
    }
    if (rc) {                                                        /* no partial output */
        memset(coef, 0, (size_t)in->coef_bytes);
        memset(qt, 0, 4 * 64 * sizeof(uint16_t));
        return rc;
    }
    memcpy(qt, h.qt, sizeof h.qt);
    return 0;
}

/* ---- the scan prepared for the device's entropy decode (csrc/jpeg_huffman_kernels.h) ------------------------------------------------ */
#define MAX_SCAN_FILE ((size_t)1 << 28)                              /* bit positions are 32-bit on the device */

static int64_t segments_of(const asep_jpeg_info* in) {
    const int64_t mcus = (int64_t)in->mcus_w * in->mcus_h;
    return in->restart_interval > 0 ? (mcus + in->restart_interval - 1) / in->restart_interval : 1;
}

int asep_jpeg_scan_sizes(const asep_jpeg_info* info, size_t n, size_t* scan_capacity, size_t* n_segments) {
    if (!info || !scan_capacity || !n_segments) return ASEP_JPEG_ARG;
    *scan_capacity = 0, *n_segments = 0;
    if (info->mcus_w < 1 || info->mcus_h < 1 || info->mcus_w > 8192 || info->mcus_h > 8192 || info->restart_interval < 0) return ASEP_JPEG_ARG;
    if (n >= MAX_SCAN_FILE) return ASEP_JPEG_REFUSED;
    *scan_capacity = (n + 3) & ~(size_t)3;                           /* the scan is a part of the file */
    *n_segments = (size_t)segments_of(info);
    return 0;
}

static void copy_table(asep_jpeg_huff* d, const huff_table* t) {
    memset(d, 0, sizeof *d);
    memcpy(d->look, t->look, sizeof d->look);
    memcpy(d->maxcode, t->maxcode, sizeof d->maxcode);
    memcpy(d->valoff, t->valoff, sizeof t->valoff);                  /* [0..16]; [17] stays 0 */
    memcpy(d->sym, t->sym, sizeof d->sym);
    d->nsym = t->nsym;
}

static int scan_prepare(const uint8_t* b, size_t n, const asep_jpeg_info* info, uint8_t* scan, size_t cap, size_t* scan_bytes,
                        asep_jpeg_segment* segments, size_t max_segments, size_t* n_segments, asep_jpeg_scan_tables* tables) {
    jpeg_header h;
    int rc = parse_header(b, n, &h);
    if (rc) return rc;
    if (memcmp(&h.info, info, sizeof *info) != 0) return ASEP_JPEG_ARG;      /* not the probe of these bytes */
    if (n >= MAX_SCAN_FILE) return ASEP_JPEG_REFUSED;
    const asep_jpeg_info* in = &h.info;
    const int64_t mcus = (int64_t)in->mcus_w * in->mcus_h, nseg = segments_of(in);
    const int64_t per_mcu = in->ncomp == 1 ? 1 : in->hs * in->vs + 2;
    if ((uint64_t)nseg > max_segments) return ASEP_JPEG_ARG;
    size_t pos = h.scan_begin, out = 0;
    int expect = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const size_t first = out;
        while (pos < n) {                                            /* up to a marker, fill bytes in front of one, or the end */
            const uint8_t v = b[pos];
            if (v == 0xFF) {
                if (n - pos < 2 || b[pos + 1] != 0) break;
                pos += 2;
            } else {
                pos += 1;
            }
            if (out >= cap) return ASEP_JPEG_ARG;
            scan[out++] = v;
        }
        if (n - pos < 2) return ASEP_JPEG_DAMAGED;                   /* b[pos] is 0xFF here */
        while (n - pos >= 2 && b[pos + 1] == 0xFF) ++pos;
        if (n - pos < 2) return ASEP_JPEG_DAMAGED;
        const int m = b[pos + 1];
        pos += 2;
        const int64_t first_mcu = s * (int64_t)in->restart_interval;
        const int64_t n_mcus = s == nseg - 1 ? mcus - first_mcu : in->restart_interval;
        /* a block takes at least two bits, and the decoder wants the last of them in the segment's last byte */
        if (out == first || (int64_t)(out - first) * 8 < n_mcus * per_mcu * 2) return ASEP_JPEG_DAMAGED;
        segments[s].byte_offset = (uint32_t)first;
        segments[s].byte_length = (uint32_t)(out - first);
        segments[s].first_mcu = (uint32_t)first_mcu;
        segments[s].n_mcus = (uint32_t)n_mcus;
        if (s == nseg - 1) {
            if (m == 0xDA || m == 0xDC || m == 0xC4 || m == 0xDB || m == 0xDD) return ASEP_JPEG_REFUSED;   /* further scans, DNL */
            if (m != 0xD9) return ASEP_JPEG_DAMAGED;
        } else {
            if (m != 0xD0 + expect) return ASEP_JPEG_DAMAGED;
            expect = (expect + 1) & 7;
        }
    }
    *scan_bytes = out;
    while (out & 3) {                                                /* whole 32-bit words for the kernels */
        if (out >= cap) return ASEP_JPEG_ARG;
        scan[out++] = 0;
    }
    *n_segments = (size_t)nseg;
    for (int c = 0; c < 3; ++c) {
        const int k = c < in->ncomp ? c : 0;
        copy_table(&tables->dc[c], &h.dc[h.td[k]]);
        copy_table(&tables->ac[c], &h.ac[h.ta[k]]);
    }
    memcpy(tables->qt, h.qt, sizeof h.qt);
    return 0;
}

int asep_jpeg_scan_prepare(const uint8_t* bytes, size_t n, const asep_jpeg_info* info, uint8_t* scan, size_t scan_capacity,
                           size_t* scan_bytes, asep_jpeg_segment* segments, size_t max_segments, size_t* n_segments,
                           asep_jpeg_scan_tables* tables) {
    if (!bytes || !info || !scan || !scan_bytes || !segments || !n_segments || !tables) return ASEP_JPEG_ARG;
    const int rc = scan_prepare(bytes, n, info, scan, scan_capacity, scan_bytes, segments, max_segments, n_segments, tables);
    if (rc) *scan_bytes = 0, *n_segments = 0;
    return rc;
}
