/* Reader of weights.bin (written by tests/test_gpu_cabi.py): every tensor goes to demfi_load_weight.
 *   int32 n; n x { int32 name_len; char name[name_len]; int32 ndim; int64 dims[ndim]; float data[prod] }
 * Returns 0, or 1 with a message on stderr. */
#ifndef DEMFI_TESTS_WEIGHTS_BIN_H
#define DEMFI_TESTS_WEIGHTS_BIN_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "demfi_hip.h"

static int load_weights_bin(demfi_ctx* ctx, const char* path)
{
    FILE* fw = fopen(path, "rb");
    if (!fw) { perror(path); return 1; }
    int32_t nt = 0;
    int bad = fread(&nt, 4, 1, fw) != 1;
    for (int i = 0; i < nt && !bad; ++i) {
        int32_t nl = 0, nd = 0;
        char key[256];
        int64_t dims[5];
        if (fread(&nl, 4, 1, fw) != 1 || nl <= 0 || nl >= (int)sizeof(key) || fread(key, 1, nl, fw) != (size_t)nl) { bad = 1; break; }
        key[nl] = 0;
        if (fread(&nd, 4, 1, fw) != 1 || nd < 1 || nd > 5 || fread(dims, 8, nd, fw) != (size_t)nd) { bad = 1; break; }
        size_t n = 1;
        for (int k = 0; k < nd; ++k) n *= (size_t)dims[k];
        float* w = (float*)malloc(n * 4);
        if (fread(w, 4, n, fw) != n) bad = 1;
        else if (demfi_load_weight(ctx, key, w, dims, nd) < 0) {
            fprintf(stderr, "demfi_load_weight(%s): %s\n", key, demfi_last_error());
            bad = 1;
        }
        free(w);
    }
    fclose(fw);
    if (bad) fprintf(stderr, "%s: truncated or rejected\n", path);
    return bad;
}
#endif
