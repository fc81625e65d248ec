/* Part of include/asep_host.h (libasep_host.so, plain C, no GPU): the sequential half of a JPEG decode, csrc/host_jpeg.c.  image_io.py binds
 * it with ctypes; the parallel half is asep_jpeg_pixels_dev of asep_hip.h. */
#ifndef ASEP_HOST_JPEG_H
#define ASEP_HOST_JPEG_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- JPEG: the entropy decode of a baseline scan (csrc/host_jpeg.c); the pixels are computed on the device (asep_hip.h, asep_jpeg_pixels_dev).
 * Accepted: SOF0 / SOF1 (Huffman, 8-bit samples), one component, or three components Y, Cb, Cr with chroma 1x1 and luma 1x1, 2x1 or
 * 2x2 in one interleaved scan.  Everything else is refused with ASEP_JPEG_REFUSED (progressive, arithmetic, lossless, 12-bit, four
 * components, other samplings, several scans, DNL, 16-bit quantisation tables, an Adobe transform other than 1 or component ids R, G, B
 * without JFIF on a three-component file, an EXIF or XMP orientation other than 1, an EXIF block that cannot be parsed, multi-picture
 * files, a block whose dequantised coefficients carry more energy than 8-bit samples can give: sum of squares above 4 000 000, the range in which
 * libjpeg-turbo's 16-bit SIMD lanes and the device's int32 arithmetic are both exact) and a stream that ends early or contradicts itself with ASEP_JPEG_DAMAGED: the caller hands such a file to its general decoder. */
#define ASEP_JPEG_REFUSED (-1)
#define ASEP_JPEG_DAMAGED (-2)
#define ASEP_JPEG_ARG (-3)

typedef struct asep_jpeg_info {
    int32_t width, height;           /* of the image */
    int32_t ncomp;                   /* 1 (gray) or 3 (Y, Cb, Cr) */
    int32_t hs, vs;                  /* luma sampling: 1x1, 2x1 or 2x2 (chroma is 1x1) */
    int32_t mcus_w, mcus_h;          /* MCU grid: ceil(width / (8 hs)), ceil(height / (8 vs)) */
    int32_t blocks_w[3], blocks_h[3];/* per component: 8x8 blocks, padded to whole MCUs */
    int32_t qt_index[3];             /* per component: its quantisation table */
    int32_t restart_interval;        /* MCUs between restart markers, 0 = none */
    int32_t reserved;                /* 0 */
    int64_t coef_bytes;              /* of all coefficients: sum of blocks_h * blocks_w * 64 * sizeof(int16_t) */
} asep_jpeg_info;

/* Parses the markers up to the scan.  0 and *info filled, or a negative code and *info zeroed. */
int asep_jpeg_probe(const uint8_t* bytes, size_t n, asep_jpeg_info* info);

/* Huffman decode of the scan of the file that asep_jpeg_probe filled `info` from.  coef (info->coef_bytes bytes): per component in order,
 * int16 [blocks_h][blocks_w][64], each block in natural (row-major) order, quantised, DC prediction undone; qt: the four quantisation tables
 * in natural order (zeros for a table the file does not define).  Handles 0xFF00 stuffing, fill bytes and restart markers.  0, or a negative
 * code with coef and qt zeroed: the segment must hold every bit that is read, restart markers must come in sequence, and EOI must follow. */
int asep_jpeg_entropy_decode(const uint8_t* bytes, size_t n, const asep_jpeg_info* info, int16_t* coef, uint16_t qt[4][64]);

#ifdef __cplusplus
}
#endif

#include "asep_host_jpeg_scan.h" /* the scan prepared for the device's entropy decode */
#endif
