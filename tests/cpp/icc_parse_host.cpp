// The ICC parser and builders (codec-eval_amd/csrc/ce_icc.cpp, which needs nothing but the public header) in a stand-alone
// program.  Built with -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_icc_parse_host_cpu.py: every input
// is copied into a malloc of exactly its length, so a read one byte outside the profile stops the run, and so does any
// undefined arithmetic on what a hostile profile's fields hold.
//
// usage: icc_parse_host INPUTS OUT.  INPUTS holds, per input, its length as a little-endian u32 and then its bytes.  OUT
// receives, per input, three int32 - the kind ce_icc_describe found and what ce_icc_build_matrix and ce_icc_build_tables
// (depth 8) returned - and, for kind 0, the nine floats of the matrix and the 3 x 256 floats of the tables.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ce_metrics.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 64;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 65;
    uint32_t len;
    int inputs = 0;
    while (fread(&len, 4, 1, in) == 1) {
        uint8_t *bytes = static_cast<uint8_t *>(malloc(len ? len : 1));
        if (!bytes || (len && fread(bytes, 1, len, in) != len)) return 66;
        ce_icc_description d;
        if (ce_icc_describe(bytes, len, &d) != CE_OK) return 67;
        if (d.kind < 0 || d.kind > 3 || (d.kind != 0) != (d.reason[0] != 0) || !memchr(d.reason, 0, sizeof d.reason)) return 68;
        float m[9] = {}, t[3 * 256] = {};
        const int32_t rc[3] = {d.kind, ce_icc_build_matrix(bytes, len, m), ce_icc_build_tables(bytes, len, 8, t, 3 * 256)};
        if ((rc[1] == CE_OK) != (d.kind == 0) || (rc[2] == CE_OK) != (d.kind == 0)) return 69;
        fwrite(rc, 4, 3, out);
        if (d.kind == 0) {
            // the deeper tables read the same curves at more points: run them for the sanitizers' sake
            float *deep = static_cast<float *>(malloc(sizeof(float) * (3u << 12)));
            if (!deep || ce_icc_build_tables(bytes, len, 12, deep, (size_t)3 << 12) != CE_OK) return 70;
            free(deep);
            fwrite(m, 4, 9, out);
            fwrite(t, 4, 3 * 256, out);
        }
        free(bytes);
        inputs++;
    }
    fclose(in);
    fclose(out);
    printf("%d\n", inputs);
    return 0;
}
