/* The host side of a context from plain C, with no GPU: for each path dtype create a 32x64 context with three per-t contexts (so the
 * batched plan exists), load the state_dict, bind it to HOST memory, read every launch op and every descriptor back, destroy it.
 * Nothing is launched.  It exists to run the plan builder, the layout / arena planner and the descriptor builder under host sanitizers
 * as a stand-alone program (tests/c/plan_walk_san.sh).
 *
 *   plan_walk <weights.bin>          "plan walk OK" and exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "demfi_hip.h"
#include "weights_bin.h"

#define CHECK(call)                                                                         \
    do {                                                                                    \
        int st__ = (call);                                                                  \
        if (st__ < 0) { fprintf(stderr, "%s failed (%d): %s\n", #call, st__, demfi_last_error()); return 1; } \
    } while (0)

enum { H = 32, W = 64, N = 2, NCTX = 3 };

/* reads every op of one segment; returns their number (< 0: error) and adds the descriptor indices they name to *sum */
static int walk(const demfi_ctx* ctx, int segment, int c, int iter, int64_t* sum)
{
    const int n = demfi_ctx_num_ops(ctx, segment, 0, c, iter);
    for (int i = 0; i < n; ++i) {
        demfi_op op;
        if (demfi_ctx_get_op(ctx, segment, 0, c, iter, i, &op) < 0) return -1;
        if (op.kind == DEMFI_OP_CONV) *sum += op.conv;
    }
    return n;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s weights.bin\n", argv[0]); return 2; }
    for (int dtype = DEMFI_F16; dtype <= DEMFI_F32; ++dtype) {
        demfi_ctx* ctx = NULL;
        CHECK(demfi_ctx_create(H, W, N, dtype, NULL, 1, NCTX, &ctx));
        if (load_weights_bin(ctx, argv[1]) != 0) return 1;
        const int64_t bytes = demfi_ctx_workspace_bytes(ctx);
        char* raw = (char*)calloc((size_t)bytes + 256, 1);
        if (!raw) { fprintf(stderr, "out of memory\n"); return 1; }
        char* ws = raw + (256 - (uintptr_t)raw % 256) % 256;
        CHECK(demfi_ctx_bind(ctx, ws, bytes, 1, NULL));
        int64_t sum = 0;
        int n_ops = 0, n;
        CHECK(n = walk(ctx, DEMFI_SEG_TRUNK, 0, 0, &sum)); n_ops += n;
        for (int c = 0; c < NCTX; ++c) {
            CHECK(n = walk(ctx, DEMFI_SEG_T_HEAD, c, 0, &sum)); n_ops += n;
            for (int it = 0; it < N; ++it) { CHECK(n = walk(ctx, DEMFI_SEG_ITER, c, it, &sum)); n_ops += n; }
        }
        CHECK(n = walk(ctx, DEMFI_SEG_TB_HEAD, 0, 0, &sum)); n_ops += n;
        for (int it = 0; it < N; ++it) { CHECK(n = walk(ctx, DEMFI_SEG_TB_ITER, 0, it, &sum)); n_ops += n; }
        const int n_descs = demfi_ctx_num_convs(ctx);
        int owners[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n_descs; ++i) {
            const demfi_conv* d = demfi_ctx_conv_desc(ctx, i);
            const int o = d ? demfi_conv_owner(d) : -1;
            if (o < 0 || o > DEMFI_OWNER_GENERAL) { fprintf(stderr, "descriptor %d: owner %d\n", i, o); return 1; }
            /* the weights and the zero page must lie inside the workspace that was bound */
            if ((const char*)d->wpack < ws || (const char*)d->wpack >= ws + bytes || (const char*)d->zero_page < ws) return 1;
            owners[o]++;
        }
        printf("%s: %d ops, %d descriptors (general %d), workspace %lld B, conv index sum %lld\n", dtype == DEMFI_F16 ? "fp16" : "fp32",
               n_ops, n_descs, owners[DEMFI_OWNER_GENERAL], (long long)bytes, (long long)sum);
        CHECK(demfi_ctx_destroy(ctx));
        free(raw);
    }
    printf("plan walk OK\n");
    return 0;
}
