/* csrc/host_jpeg.c under the address and undefined-behaviour sanitizers, as a stand-alone program (tests/test_jpeg_sanitize.py builds and
 * runs it; nothing is loaded into Python).  Every input lives in a heap block of exactly its length and the coefficients in a heap block
 * of exactly the size the probe returned, so a read past the file or a write past the probe's size is a sanitizer report.
 *
 *   host_jpeg_check FILE...          every file: probe + decode; each call returns success or one of the refusals
 *   host_jpeg_check --fuzz FILE      every prefix of FILE and 2000 seeded single-byte mutations of it, the same way */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/asep_host.h"

static long n_ok = 0, n_refused = 0;

static int run(const uint8_t* data, size_t n) {
    uint8_t* bytes = (uint8_t*)malloc(n ? n : 1);                    /* exactly n bytes (one for the empty prefix, never read) */
    if (!bytes) return 1;
    memcpy(bytes, data, n);
    asep_jpeg_info info;
    int rc = asep_jpeg_probe(bytes, n, &info);
    if (rc != 0 && rc != ASEP_JPEG_REFUSED && rc != ASEP_JPEG_DAMAGED) {
        fprintf(stderr, "probe returned %d\n", rc);
        return 1;
    }
    if (rc == 0) {
        if (info.coef_bytes <= 0 || info.coef_bytes > ((int64_t)1 << 32)) {
            fprintf(stderr, "probe accepted a frame of %lld coefficient bytes over %zu file bytes\n", (long long)info.coef_bytes, n);
            return 1;
        }
        int16_t* coef = (int16_t*)malloc((size_t)info.coef_bytes);
        uint16_t(*qt)[64] = (uint16_t(*)[64])malloc(4 * 64 * sizeof(uint16_t));
        if (!coef || !qt) return 1;
        rc = asep_jpeg_entropy_decode(bytes, n, &info, coef, qt);
        if (rc != 0 && rc != ASEP_JPEG_REFUSED && rc != ASEP_JPEG_DAMAGED) {
            fprintf(stderr, "decode returned %d\n", rc);
            return 1;
        }
        if (rc != 0) {                                               /* no partial output */
            for (int64_t i = 0; i < info.coef_bytes / 2; ++i)
                if (coef[i]) {
                    fprintf(stderr, "a refused decode left coefficients behind\n");
                    return 1;
                }
        }
        free(coef);
        free(qt);
    }
    if (rc == 0) ++n_ok;
    else ++n_refused;
    free(bytes);
    return 0;
}

static uint8_t* read_file(const char* path, size_t* n) {
    FILE* f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* p = (uint8_t*)malloc(size > 0 ? (size_t)size : 1);
    if (p && size > 0 && fread(p, 1, (size_t)size, f) != (size_t)size) {
        free(p);
        p = NULL;
    }
    fclose(f);
    *n = (size_t)size;
    return p;
}

int main(int argc, char** argv) {
    if (argc >= 3 && strcmp(argv[1], "--fuzz") == 0) {
        size_t n;
        uint8_t* data = read_file(argv[2], &n);
        if (!data) return 2;
        if (run(data, n) || n_ok != 1) {
            fprintf(stderr, "%s itself is not accepted\n", argv[2]);
            return 1;
        }
        for (size_t k = 0; k < n; ++k)
            if (run(data, k)) return 1;
        uint64_t state = 0x9E3779B97F4A7C15ull;                      /* seeded: the same mutations on every run */
        for (int i = 0; i < 2000; ++i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const size_t at = (size_t)((state >> 33) % n);
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const uint8_t old = data[at];
            data[at] = (uint8_t)(state >> 40);
            if (run(data, n)) return 1;
            data[at] = old;
        }
        free(data);
        printf("host jpeg ok: fuzz, %ld accepted, %ld refused\n", n_ok, n_refused);
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        size_t n;
        uint8_t* data = read_file(argv[i], &n);
        if (!data) return 2;
        const long before = n_ok;
        if (run(data, n)) return 1;
        free(data);
        if (n_ok != before + 1) {
            fprintf(stderr, "%s is not accepted\n", argv[i]);
            return 1;
        }
    }
    printf("host jpeg ok: files, %ld accepted, %ld refused\n", n_ok, n_refused);
    return 0;
}
