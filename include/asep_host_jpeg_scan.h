/* Part of include/asep_host_jpeg.h (libasep_host.so, plain C, no GPU): a JPEG scan prepared for the device's entropy decode,
 * csrc/host_jpeg.c.  image_io.py binds it with ctypes; the decode itself is asep_jpeg_entropy_dev of asep_hip.h. */
#ifndef ASEP_HOST_JPEG_SCAN_H
#define ASEP_HOST_JPEG_SCAN_H
#include "asep_host_jpeg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the scan prepared for the device's entropy decode (asep_hip.h, asep_jpeg_entropy_dev): the one pass over the file that stays on
 * the host.  The entropy-coded bytes are written back to back with 0xFF00 stuffing, fill bytes and restart markers dropped; a SEGMENT is one
 * restart interval, or the whole scan where the file has none. */
#define ASEP_JPEG_LOOK_BITS 9
typedef struct asep_jpeg_huff {          /* one Huffman table in the form the kernels index (1432 bytes; six of them fit LDS many times) */
    uint16_t look[1 << ASEP_JPEG_LOOK_BITS]; /* (length << 8) | symbol of the code that starts with these bits, 0 = longer than LOOK_BITS */
    int32_t maxcode[18];                 /* largest code of each length 1..16, -1 = none; [17] = 0x7fffffff */
    int32_t valoff[18];                  /* index of a length's first symbol minus its first code */
    uint8_t sym[256];
    int32_t nsym;
    int32_t reserved;                    /* 0 */
} asep_jpeg_huff;

typedef struct asep_jpeg_scan_tables {
    asep_jpeg_huff dc[3], ac[3];         /* per component of the scan: its DC and its AC table */
    uint16_t qt[4][64];                  /* the four quantisation tables, natural order, zeros where the file defines none */
} asep_jpeg_scan_tables;

typedef struct asep_jpeg_segment {
    uint32_t byte_offset;                /* of its first byte in the unstuffed buffer */
    uint32_t byte_length;                /* >= 1 */
    uint32_t first_mcu;                  /* in scan order */
    uint32_t n_mcus;                     /* restart_interval, less for the last segment; all MCUs where there is no interval */
} asep_jpeg_segment;

/* The sizes asep_jpeg_scan_prepare writes at most, from the probe's `info` and the file's length alone: *scan_capacity bytes (a multiple of
 * 4: the kernels read 32-bit words) and *n_segments entries (exactly as many as the prepared scan has).  0, ASEP_JPEG_ARG, or
 * ASEP_JPEG_REFUSED for a file of 2^28 bytes or more (bit positions are 32-bit on the device). */
int asep_jpeg_scan_sizes(const asep_jpeg_info* info, size_t n, size_t* scan_capacity, size_t* n_segments);

/* For the file that asep_jpeg_probe filled `info` from.  Writes *scan_bytes unstuffed bytes into scan (zeros up to the next multiple of 4),
 * the segments and the tables.  Applies the structural rules of asep_jpeg_entropy_decode: restart markers in sequence, EOI behind the last
 * segment (another scan or DNL: ASEP_JPEG_REFUSED), no empty segment, every read checked against n and every write against scan_capacity
 * and max_segments (too small: ASEP_JPEG_ARG).  0, or the negative code with *scan_bytes and *n_segments zero. */
int asep_jpeg_scan_prepare(const uint8_t* bytes, size_t n, const asep_jpeg_info* info, uint8_t* scan, size_t scan_capacity,
                           size_t* scan_bytes, asep_jpeg_segment* segments, size_t max_segments, size_t* n_segments,
                           asep_jpeg_scan_tables* tables);

#ifdef __cplusplus
}
#endif
#endif
