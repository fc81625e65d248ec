/* asep_jpeg_scan_prepare of csrc/host_jpeg.c under the address and undefined-behaviour sanitizers, as a stand-alone program
 * (tests/test_jpeg_scan_host.py builds and runs it; nothing is loaded into Python).  Every input lives in a heap block of exactly its
 * length, the unstuffed bytes and the segments in heap blocks of exactly the sizes asep_jpeg_scan_sizes returned, so a read past the
 * file or a write past a size is a sanitizer report.
 *
 *   host_jpeg_scan_check FILE...     every file (must be accepted), every prefix of every file (must be refused) and 2000 seeded
 *                                    single-byte mutations dealt over the files (success or a refusal) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/asep_host.h"

static long n_ok = 0, n_refused = 0;

static int is_refusal(int rc) { return rc == ASEP_JPEG_REFUSED || rc == ASEP_JPEG_DAMAGED; }

/* 0 if the calls behaved (success or a refusal, sizes kept, segments consistent), 1 otherwise */
static int run(const uint8_t* data, size_t n) {
    uint8_t* bytes = (uint8_t*)malloc(n ? n : 1);                    /* exactly n bytes (one for the empty prefix, never read) */
    if (!bytes) return 1;
    memcpy(bytes, data, n);
    asep_jpeg_info info;
    int rc = asep_jpeg_probe(bytes, n, &info);
    if (rc != 0 && !is_refusal(rc)) {
        fprintf(stderr, "probe returned %d\n", rc);
        return 1;
    }
    if (rc == 0) {
        size_t cap = 0, nseg = 0, used = 0, got = 0;
        rc = asep_jpeg_scan_sizes(&info, n, &cap, &nseg);
        if (rc != 0 || cap < n || cap > n + 3 || nseg < 1 || nseg > (size_t)info.mcus_w * (size_t)info.mcus_h) {
            fprintf(stderr, "sizes returned %d: %zu bytes, %zu segments for a file of %zu bytes\n", rc, cap, nseg, n);
            return 1;
        }
        uint8_t* scan = (uint8_t*)malloc(cap);
        asep_jpeg_segment* segs = (asep_jpeg_segment*)malloc(nseg * sizeof *segs);
        asep_jpeg_scan_tables* tables = (asep_jpeg_scan_tables*)malloc(sizeof *tables);
        if (!scan || !segs || !tables) return 1;
        rc = asep_jpeg_scan_prepare(bytes, n, &info, scan, cap, &used, segs, nseg, &got, tables);
        if (rc != 0 && !is_refusal(rc)) {
            fprintf(stderr, "prepare returned %d\n", rc);
            return 1;
        }
        if (rc == 0) {
            size_t next = 0, mcu = 0;
            if (got != nseg || used > cap) return 1;
            for (size_t i = 0; i < got; ++i) {
                if (segs[i].byte_offset != next || segs[i].byte_length == 0 || segs[i].first_mcu != mcu) {
                    fprintf(stderr, "segment %zu does not continue the scan\n", i);
                    return 1;
                }
                next += segs[i].byte_length, mcu += segs[i].n_mcus;
            }
            if (next != used || mcu != (size_t)info.mcus_w * (size_t)info.mcus_h) {
                fprintf(stderr, "the segments cover %zu of %zu bytes and %zu MCUs\n", next, used, mcu);
                return 1;
            }
            for (int c = 0; c < 3; ++c)
                if (tables->dc[c].nsym < 0 || tables->dc[c].nsym > 256 || tables->ac[c].nsym < 0 || tables->ac[c].nsym > 256) return 1;
        } else if (used != 0 || got != 0) {
            fprintf(stderr, "a refused prepare left sizes behind\n");
            return 1;
        }
        free(scan);
        free(segs);
        free(tables);
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
    const int n_files = argc - 1;
    long n_prefixes = 0, n_mutations = 0;
    uint64_t state = 0x9E3779B97F4A7C15ull;                          /* seeded: the same mutations on every run */
    if (n_files < 1) return 2;
    for (int i = 0; i < n_files; ++i) {
        size_t n;
        uint8_t* data = read_file(argv[1 + i], &n);
        if (!data) return 2;
        long before = n_ok;
        if (run(data, n) || n_ok != before + 1) {
            fprintf(stderr, "%s is not accepted\n", argv[1 + i]);
            return 1;
        }
        before = n_ok;
        for (size_t k = 0; k < n; ++k, ++n_prefixes)
            if (run(data, k)) return 1;
        if (n_ok != before) {
            fprintf(stderr, "a prefix of %s is accepted\n", argv[1 + i]);
            return 1;
        }
        for (int m = i; m < 2000; m += n_files, ++n_mutations) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const size_t at = (size_t)((state >> 33) % n);
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const uint8_t old = data[at];
            data[at] = (uint8_t)(state >> 40);
            if (run(data, n)) return 1;
            data[at] = old;
        }
        free(data);
    }
    printf("host jpeg scan ok: %d files, %ld prefixes, %ld mutations, %ld accepted, %ld refused\n", n_files, n_prefixes, n_mutations, n_ok,
           n_refused);
    return 0;
}
