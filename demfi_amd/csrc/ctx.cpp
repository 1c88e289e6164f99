// Forward context of libdemfi_hip.so: the life cycle of a context, the C ABI entry points and the op interpreter (demfi_run_op).
//
// Host logic only.  demfi_ctx_create sizes the plan (plan.cpp) and lays every activation buffer out inside ONE caller-owned workspace
// (layout.cpp); demfi_ctx_bind builds the plan on that workspace and uploads packed weights and descriptors (conv_build.cpp).
#include "plan.h"
#include <stdlib.h>
#include <string.h>

using namespace plan;

namespace {

int run_ops(demfi_ctx* c, const OpList& ops, void* stream)
{
    for (const demfi_op& op : ops) {
        const int st = demfi_run_op(c, &op, stream);
        if (st < 0) return st;
    }
    return DEMFI_OK;
}

bool check_idx(const demfi_ctx* c, int trunk, int q)
{
    return c && trunk >= 0 && trunk < c->n_trunk && q >= 0 && q < c->n_ctx;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
// What every kind of context does once its fields are set: the layer table, the sizing pass, the arena, the final layout.  Owns c on failure.
static int size_context(demfi_ctx* c, demfi_ctx** out)
{
    layer_table(c);
    // sizing pass: lay the buffers out, walk the plan without weights to learn the exact size of the packed blob and the
    // number of descriptors, then lay everything out for real
    compute_layout(c, 0, 0);
    int st = run_builder(c, true);
    if (st < 0) { delete c; return st; }
    // the workspace arena: buffers of a set that are never alive together share memory (DEMFI_ARENA=0: one region per buffer,
    // the layout of rounds 1-4; results are bit-identical either way)
    static const bool arena_on = !(getenv("DEMFI_ARENA") && atoi(getenv("DEMFI_ARENA")) == 0);
    if (arena_on && !c->op_kind) {
        std::vector<const OpList*> per_t = {&c->head_ops[0][0]}, tr = {&c->tr_ops[0]}, none;
        for (int it = 0; it < c->N; ++it) per_t.push_back(&c->iter_ops[0][0][it]);
        std::vector<const OpList*> per_t_all = per_t;
        if (c->n_ctx > 1) { per_t_all.push_back(&c->tb_head_ops[0]); for (int it = 0; it < c->N; ++it) per_t_all.push_back(&c->tb_iter_ops[0][it]); }
        const ArenaPlan pt = plan_arena(c, c->t_bufs[0][0], c->n_ctx, per_t, none,
                                        {"Ft", "u1", "u2", "u3", "d0", "d1", "d2", "rF", "dec_a", "dec_t", "dec_b", "frec0", "frec1", "re1", "rd64", "de1",
                                         "bl1", "xb", "zb", "rh", "h1", "fo1", "g_a", "g_t", "g_b", "g_p2", "misc16", "ref16", "ref32", "agg3s"});
        const ArenaPlan ptr_ = plan_arena(c, c->tr_bufs[0], 0, tr, per_t_all,
                                          {"s2d", "f1", "x0", "grow", "gffcat", "g0", "g1", "up", "enc_a", "enc_t", "enc_b", "rk", "skk", "rkp", "skp",
                                           "smp", "E", "wg"});
        c->arena_t = pt;
        c->arena_tr = ptr_;
        if (getenv("DEMFI_ARENA_DEBUG")) {
            for (auto* pl : {&c->arena_t, &c->arena_tr}) {
                fprintf(stderr, "arena %s: %.1f MB\n", pl == &c->arena_t ? "per-t (all contexts)" : "trunk", pl->size / 1e6);
                for (auto& kv : pl->off) fprintf(stderr, "   %-8s at %.1f MB\n", kv.first.c_str(), kv.second / 1e6);
            }
        }
    }
    compute_layout(c, c->blob_fill, (int64_t)c->descs.size());
    c->descs.clear();
    *out = c;
    return DEMFI_OK;
}

extern "C" int demfi_ctx_create(int H, int W, int max_updates, int dtype, const demfi_hparams* hp, int n_trunk, int n_ctx, demfi_ctx** out)
{
    if (!out) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_create: null out");
    if (H <= 0 || W <= 0 || H % 8 || W % 8)
        return demfi_set_error(DEMFI_ERR_ARG, "DeMFI-Net needs H, W multiples of 8 (the harness pads to 32): got %dx%d", H, W);
    if (max_updates < 1 || max_updates > 64 || (dtype != DEMFI_F16 && dtype != DEMFI_F32) || n_trunk < 1 || n_ctx < 1 || n_trunk > 8 || n_ctx > 16)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_create: max_updates / dtype / context counts");
    demfi_hparams h = {64, 2, 5, 5, 1, 0, 0, 0};
    if (hp) h = *hp;
    if (h.nf != 64 || h.scale_factor != 2)
        return demfi_set_error(DEMFI_ERR_ARG, "the HIP path is built for nf=64, scale_factor=2 (the released configuration)");
    if (h.num_resb_facfb < 0 || h.num_resb_dec < 0 || h.num_resb_facfb > 32 || h.num_resb_dec > 32)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_create: residual block counts");
    // fgac_rr / fgac_sr: the radii hard-coded to 0 at DeMFInet.py:401-402; > 0 selects the generalised window FGAC
    // (demfi_fgac_window, both path dtypes; flags bit 0 = index map: 0 reference code, 1 pixel-centred window)
    if (h.fgac_rr < 0 || h.fgac_rr > 2 || h.fgac_sr < 0 || h.fgac_sr > 4 || (h.flags & ~(DEMFI_HP_FGAC_CENTRED | DEMFI_HP_EXTRAS)))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_create: fgac_rr in 0..2, fgac_sr in 0..4, map in {0,1}");
    if (h.fgac_rr == 0 && h.fgac_sr != 0)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_create: fgac_sr > 0 needs fgac_rr > 0 (the pooled point-wise form is not built)");
    demfi_ctx* c = new demfi_ctx();
    c->H = H; c->W = W; c->N = max_updates; c->dtype = dtype; c->n_trunk = n_trunk; c->n_ctx = n_ctx; c->hp = h;
    return size_context(c, out);
}

// ---- single-call operator contexts (ABI v7; SURVEY.md 8b names demfi_gru_sep / demfi_fgac) --------------------------------------
static int operator_create(int kind, int batch, int H, int W, int dtype, demfi_ctx** out)
{
    if (!out) return demfi_set_error(DEMFI_ERR_ARG, "operator context: null out");
    if (batch < 1 || batch > 64 || H < 8 || W < 8 || (dtype != DEMFI_F16 && dtype != DEMFI_F32))
        return demfi_set_error(DEMFI_ERR_ARG, "operator context: batch 1..64, H, W >= 8, dtype F16 / F32");
    demfi_ctx* c = new demfi_ctx();
    c->H = H; c->W = W; c->N = 1; c->dtype = dtype; c->n_trunk = 1; c->n_ctx = 1; c->op_kind = kind; c->op_batch = batch;
    c->hp = {64, 2, 0, 0, 1, 0, 0, 0};
    return size_context(c, out);
}

extern "C" int demfi_gru_sep_create(int batch, int H, int W, int dtype, demfi_ctx** out) { return operator_create(1, batch, H, W, dtype, out); }
extern "C" int demfi_fgac_create(int batch, int H, int W, int dtype, demfi_ctx** out) { return operator_create(2, batch, H, W, dtype, out); }

extern "C" int demfi_operator_run(demfi_ctx* c, void* stream)
{
    if (!c || !c->op_kind || !c->bound || c->on_host)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_operator_run: not an operator context bound to device memory");
    return run_ops(c, c->tr_ops[0], stream);
}

extern "C" int demfi_ctx_destroy(demfi_ctx* c)
{
    delete c;
    return DEMFI_OK;
}

extern "C" int demfi_load_weight(demfi_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim)
{
    if (!c || !name || !host || !shape || ndim < 1 || ndim > 5) return demfi_set_error(DEMFI_ERR_ARG, "demfi_load_weight: bad arguments");
    if (c->bound) return demfi_set_error(DEMFI_ERR_ARG, "demfi_load_weight: context already bound (create a new one to change weights)");
    std::string n(name);
    const bool is_w = n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0;
    const bool is_b = n.size() > 5 && n.compare(n.size() - 5, 5, ".bias") == 0;
    if (!is_w && !is_b) return demfi_set_error(DEMFI_ERR_ARG, "demfi_load_weight: '%s' is neither a .weight nor a .bias key", name);
    const std::string layer = n.substr(0, n.size() - (is_w ? 7 : 5));
    auto it = c->table.find(layer);
    if (it == c->table.end()) return demfi_set_error(DEMFI_ERR_ARG, "demfi_load_weight: unknown state_dict key '%s'", name);
    const Layer& l = it->second;
    int64_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= shape[i];
    bool ok;
    if (is_b) ok = ndim == 1 && shape[0] == l.cout;
    else if (ndim == 4) ok = shape[0] == l.cout && shape[1] == l.cin && shape[2] == l.kh && shape[3] == l.kw;
    else ok = ndim == 5 && shape[0] == l.cout && shape[1] == l.cin && shape[2] == 1 && shape[3] == l.kh && shape[4] == l.kw;   // Conv3d (1,k,k)
    if (!ok) return demfi_set_error(DEMFI_ERR_ARG, "demfi_load_weight: shape of '%s' does not match [%d,%d,%d,%d]", name, l.cout, l.cin, l.kh, l.kw);
    Weight& w = c->weights[n];
    w.data.assign(host, host + numel);
    w.shape.assign(shape, shape + ndim);
    return DEMFI_OK;
}

extern "C" int64_t demfi_ctx_workspace_bytes(const demfi_ctx* c) { return c ? c->total : 0; }

extern "C" int64_t demfi_workspace_bytes(int H, int W, int max_updates, int dtype, int n_trunk, int n_ctx)
{
    demfi_ctx* c = nullptr;
    if (demfi_ctx_create(H, W, max_updates, dtype, nullptr, n_trunk, n_ctx, &c) < 0) return -1;
    const int64_t n = c->total;
    delete c;
    return n;
}

extern "C" int demfi_ctx_bind(demfi_ctx* c, void* workspace, int64_t bytes, int on_host, void* stream)
{
    if (!c || !workspace) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_bind: null argument");
    if (c->bound) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_bind: already bound");
    if (bytes < c->total) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_bind: workspace of %lld B < %lld B", (long long)bytes, (long long)c->total);
    if (((uintptr_t)workspace) & 255) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_bind: workspace must be 256-byte aligned");
    c->base = (char*)workspace;
    c->on_host = on_host != 0;
    c->host_blob.assign(c->w_bytes, 0);
    const int st = run_builder(c, false);
    if (st < 0) return st;
    const int64_t desc_bytes = (int64_t)c->descs.size() * (int64_t)sizeof(demfi_conv);
    if ((int64_t)c->descs.size() != c->n_descs || c->blob_fill > c->w_bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_bind: plan differs from the sizing pass (%d descriptors, %lld B of weights)",
                               (int)c->descs.size(), (long long)c->blob_fill);
    if (c->on_host) {
        memcpy(c->base + c->w_region, c->host_blob.data(), c->w_bytes);
        memcpy(c->base + c->desc_off, c->descs.data(), desc_bytes);
    } else {
        hipStream_t st = (hipStream_t)stream;
        DEMFI_HIP_CHECK(hipMemcpyAsync(c->base + c->w_region, c->host_blob.data(), c->w_bytes, hipMemcpyHostToDevice, st));
        DEMFI_HIP_CHECK(hipMemcpyAsync(c->base + c->desc_off, c->descs.data(), desc_bytes, hipMemcpyHostToDevice, st));
        DEMFI_HIP_CHECK(hipStreamSynchronize(st));
    }
    c->host_blob.clear();
    c->host_blob.shrink_to_fit();
    c->weights.clear();                                          // the fp32 copies are not needed once packed
    c->bound = true;
    return DEMFI_OK;
}

extern "C" int demfi_ctx_weight_region(const demfi_ctx* c, int64_t* offset, int64_t* bytes)
{
    if (!c || !offset || !bytes) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_weight_region: null argument");
    *offset = c->w_region;
    *bytes = c->w_bytes;
    return DEMFI_OK;
}

extern "C" int demfi_ctx_buffer(const demfi_ctx* c, int trunk, int q, const char* name, int64_t* offset, int32_t* kind, int32_t dims[4])
{
    if (!c || !name || !offset || trunk < 0 || trunk >= c->n_trunk || q < -1 || q >= c->n_ctx)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_buffer: bad arguments");
    const BufSet& s = q < 0 ? c->tr_bufs[trunk] : c->t_bufs[trunk][q];
    auto it = s.find(name);
    if (it == s.end()) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_buffer: no buffer '%s' in %s context", name, q < 0 ? "the trunk" : "the per-t");
    *offset = it->second.off;
    if (kind) *kind = it->second.kind;
    if (dims) for (int i = 0; i < 4; ++i) dims[i] = it->second.d[i];
    return DEMFI_OK;
}

extern "C" int demfi_ingest_u8(demfi_ctx* c, int trunk, const uint8_t* const* frames, int h, int w, void* stream)
{
    if (!c || !c->bound || c->on_host || trunk < 0 || trunk >= c->n_trunk)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ingest_u8: context not bound to device memory / bad trunk index");
    BufSet& B = c->tr_bufs[trunk];
    return demfi_u8_ingest(frames, h, w, (float*)(c->base + B["x"].off), c->base + B["s2d"].off, (float*)(c->base + B["overlay"].off),
                           c->dtype, c->H, c->W, stream);
}

extern "C" int demfi_ingest_u16(demfi_ctx* c, int trunk, const uint16_t* const* frames, int h, int w, int depth, void* stream)
{
    if (!c || !c->bound || c->on_host || trunk < 0 || trunk >= c->n_trunk)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ingest_u16: context not bound to device memory / bad trunk index");
    BufSet& B = c->tr_bufs[trunk];
    return demfi_u16_ingest(frames, h, w, depth, (float*)(c->base + B["x"].off), c->base + B["s2d"].off,
                            (float*)(c->base + B["overlay"].off), c->dtype, c->H, c->W, stream);
}

extern "C" int demfi_ingest_u16_rect(demfi_ctx* c, int trunk, const uint16_t* const* frames, int fh, int fw, int y0, int x0, int h, int w,
                                     int depth, void* stream)
{
    if (!c || !c->bound || c->on_host || trunk < 0 || trunk >= c->n_trunk)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_ingest_u16_rect: context not bound to device memory / bad trunk index");
    BufSet& B = c->tr_bufs[trunk];
    return demfi_u16_ingest_rect(frames, fh, fw, y0, x0, h, w, depth, (float*)(c->base + B["x"].off), c->base + B["s2d"].off,
                                 (float*)(c->base + B["overlay"].off), c->dtype, c->H, c->W, stream);
}

extern "C" int demfi_forward_trunk_body(demfi_ctx* c, int trunk, void* stream)
{
    if (!c || !c->bound || c->on_host || trunk < 0 || trunk >= c->n_trunk)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_forward_trunk_body: context not bound to device memory / bad trunk index");
    const OpList& ops = c->tr_ops[trunk];                        // ops 0, 1 = s2d, overlay: done by demfi_ingest_u8
    for (size_t i = 2; i < ops.size(); ++i) {
        const int st = demfi_run_op(c, &ops[i], stream);
        if (st < 0) return st;
    }
    return DEMFI_OK;
}

extern "C" int demfi_forward_trunk(demfi_ctx* c, int trunk, const float* x, void* stream)
{
    if (!c || !c->bound || c->on_host || trunk < 0 || trunk >= c->n_trunk)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_forward_trunk: context not bound to device memory / bad trunk index");
    const Tensor& xb = c->tr_bufs[trunk]["x"];
    if (x && (const char*)x != c->base + xb.off)
        DEMFI_HIP_CHECK(hipMemcpyAsync(c->base + xb.off, x, xb.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return run_ops(c, c->tr_ops[trunk], stream);
}

extern "C" int demfi_forward_t(demfi_ctx* c, int trunk, int q, int n_updates, void* stream)
{
    if (!c || !c->bound || c->on_host || !check_idx(c, trunk, q))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_forward_t: context not bound to device memory / bad context index");
    if (n_updates < 1 || n_updates > c->N)
        return demfi_set_error(DEMFI_ERR_ARG, "num_update=%d outside 1..%d the context was built for", n_updates, c->N);
    int st = run_ops(c, c->head_ops[trunk][q], stream);
    for (int it = 0; it < n_updates && st >= 0; ++it) st = run_ops(c, c->iter_ops[trunk][q][it], stream);
    return st;
}

extern "C" int demfi_forward_tb(demfi_ctx* c, int trunk, int n_updates, void* stream)
{
    if (!c || !c->bound || c->on_host || trunk < 0 || trunk >= c->n_trunk)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_forward_tb: context not bound to device memory / bad trunk index");
    if (c->n_ctx < 2) return demfi_set_error(DEMFI_ERR_ARG, "demfi_forward_tb: the context has one per-t context (use demfi_forward_t)");
    if (n_updates < 1 || n_updates > c->N)
        return demfi_set_error(DEMFI_ERR_ARG, "num_update=%d outside 1..%d the context was built for", n_updates, c->N);
    int st = run_ops(c, c->tb_head_ops[trunk], stream);
    for (int it = 0; it < n_updates && st >= 0; ++it) st = run_ops(c, c->tb_iter_ops[trunk][it], stream);
    return st;
}

// In a recursion the PWB + D2 tail (warp_thin .. Dec_last2_2) only produces that recursion's frames: the state the next
// recursion reads is F_rec and the flow / occlusion logits (DeMFInet.py:130-137; Agg3 and D2, 146-165, feed Sharps_final only).
static size_t d2_start(const OpList& ops)
{
    for (size_t i = 0; i < ops.size(); ++i)
        if (ops[i].kind == DEMFI_OP_WARP && ops[i].nch == 3) return i;
    return ops.size();
}

extern "C" int demfi_forward_tb_final(demfi_ctx* c, int trunk, int n_updates, void* stream)
{
    if (!c || !c->bound || c->on_host || trunk < 0 || trunk >= c->n_trunk)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_forward_tb_final: context not bound to device memory / bad trunk index");
    if (c->n_ctx < 2) return demfi_set_error(DEMFI_ERR_ARG, "demfi_forward_tb_final: the context has one per-t context");
    if (n_updates < 1 || n_updates > c->N)
        return demfi_set_error(DEMFI_ERR_ARG, "num_update=%d outside 1..%d the context was built for", n_updates, c->N);
    int st = run_ops(c, c->tb_head_ops[trunk], stream);
    for (int it = 0; it < n_updates && st >= 0; ++it) {
        const OpList& ops = c->tb_iter_ops[trunk][it];
        const size_t n = it + 1 < n_updates ? d2_start(ops) : ops.size();
        for (size_t i = 0; i < n && st >= 0; ++i) st = demfi_run_op(c, &ops[i], stream);
    }
    return st;
}

static const OpList* seg_ops(const demfi_ctx* c, int segment, int trunk, int q, int iter)
{
    if (!c || !c->bound || trunk < 0 || trunk >= c->n_trunk) return nullptr;
    if (segment == DEMFI_SEG_TRUNK) return &c->tr_ops[trunk];
    if (segment == DEMFI_SEG_TB_HEAD) return &c->tb_head_ops[trunk];
    if (segment == DEMFI_SEG_TB_ITER && iter >= 0 && iter < c->N) return &c->tb_iter_ops[trunk][iter];
    if (q < 0 || q >= c->n_ctx) return nullptr;
    if (segment == DEMFI_SEG_T_HEAD) return &c->head_ops[trunk][q];
    if (segment == DEMFI_SEG_ITER && iter >= 0 && iter < c->N) return &c->iter_ops[trunk][q][iter];
    return nullptr;
}

extern "C" int demfi_ctx_num_ops(const demfi_ctx* c, int segment, int trunk, int q, int iter)
{
    const OpList* o = seg_ops(c, segment, trunk, q, iter);
    if (!o) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_num_ops: bad segment / context (or context not bound)");
    return (int)o->size();
}

extern "C" int demfi_ctx_get_op(const demfi_ctx* c, int segment, int trunk, int q, int iter, int index, demfi_op* out)
{
    const OpList* o = seg_ops(c, segment, trunk, q, iter);
    if (!o || !out || index < 0 || index >= (int)o->size()) return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_get_op: bad arguments");
    *out = (*o)[index];
    return DEMFI_OK;
}

extern "C" int demfi_ctx_num_convs(const demfi_ctx* c) { return c ? (int)c->descs.size() : 0; }

extern "C" const demfi_conv* demfi_ctx_conv_desc(const demfi_ctx* c, int index)
{
    if (!c || index < 0 || index >= (int)c->descs.size()) return nullptr;
    return &c->descs[index];
}

extern "C" int demfi_run_op(demfi_ctx* c, const demfi_op* op, void* stream)
{
    if (!c || !op || !c->bound || c->on_host) return demfi_set_error(DEMFI_ERR_ARG, "demfi_run_op: context not bound to device memory");
    const int H = c->H, W = c->W;
    switch (op->kind) {
    case DEMFI_OP_CONV:
        if (op->conv < 0 || op->conv >= (int)c->descs.size()) return demfi_set_error(DEMFI_ERR_ARG, "demfi_run_op: descriptor index");
        return demfi_conv2d(&c->descs[op->conv], (const demfi_conv*)(c->base + c->desc_off) + op->conv, stream);
    case DEMFI_OP_RESBLOCK:
        if (op->conv < 0 || op->conv >= (int)c->descs.size() || op->nch < 0 || op->nch >= (int)c->descs.size())
            return demfi_set_error(DEMFI_ERR_ARG, "demfi_run_op: descriptor index");
        return demfi_resblock3x3_c64(&c->descs[op->conv], &c->descs[op->nch], stream);
    case DEMFI_OP_GRU_R:
        if (op->conv < 0 || op->conv >= (int)c->descs.size()) return demfi_set_error(DEMFI_ERR_ARG, "demfi_run_op: descriptor index");
        return demfi_gru_r(&c->descs[op->conv], stream);
    case DEMFI_OP_GRU_ZQ:
        if (op->conv < 0 || op->conv >= (int)c->descs.size() || op->nch < 0 || op->nch >= (int)c->descs.size())
            return demfi_set_error(DEMFI_ERR_ARG, "demfi_run_op: descriptor index");
        return demfi_gru_zq(&c->descs[op->conv], &c->descs[op->nch], stream);
    case DEMFI_OP_PACK:
        if (op->bt.nb > 1)
            return demfi_pack_planes_batched((const float* const*)op->p, op->nch, op->o.ptr, c->dtype, op->o.sx, H, W, &op->bt, stream);
        return demfi_pack_planes((const float* const*)op->p, op->nch, op->o.ptr, c->dtype, op->o.sx, H, W, stream);
    case DEMFI_OP_VIZ:
        if (op->conv == 0) return demfi_absmean_map(&op->a, op->b.ptr ? &op->b : nullptr, (float*)op->p[0], op->nch, H, W, stream);
        if (op->conv == 1) return demfi_minmax_normalize((float*)op->p[0], (int64_t)H * W, (float*)op->p[1], stream);
        if (op->conv == 2) return demfi_one_minus((const float*)op->p[1], (float*)op->p[0], (int64_t)H * W, stream);
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_run_op: visualisation sub-op %d", op->conv);
    case DEMFI_OP_S2D:
        return demfi_space_to_depth((const float*)op->p[0], (void*)op->p[1], c->dtype, H, W, stream);
    case DEMFI_OP_OVERLAY:
        return demfi_overlay_mean((const float*)op->p[0], (float*)op->p[1], H, W, stream);
    case DEMFI_OP_FGAC:
        return demfi_fgac_gather(&op->a, (const float*)op->p[0], &op->o, op->nch, H, W, nullptr, stream);
    case DEMFI_OP_FGAC_WINDOW:
        return demfi_fgac_window(&op->a, &op->b, (const float*)op->p[0], &op->o, op->nch, H, W, op->conv, op->_pad, nullptr, stream);
    case DEMFI_OP_AVG_POOL:
        return demfi_avg_pool_fat(&op->a, &op->o, op->nch, H, W, op->conv, stream);
    case DEMFI_OP_GATE:
        return demfi_gate_blend((const float*)op->p[0], &op->a, &op->b, &op->o, op->nch, H, W, stream);
    case DEMFI_OP_CFR:
        if (op->p[5])
            return demfi_cfr_flow_align_pack((const float*)op->p[0], (const float*)op->p[1], (const float*)op->p[4], (const float*)op->t, H, W,
                                             (int64_t*)op->p[2], (float*)op->p[3], (void*)op->p[5], c->dtype, op->bt.nb > 1 ? &op->bt : nullptr, stream);
        if (op->bt.nb > 1)
            return demfi_cfr_flow_align_batched((const float*)op->p[0], (const float*)op->p[1], (const float*)op->t, H, W, (int64_t*)op->p[2],
                                                (float*)op->p[3], &op->bt, stream);
        return demfi_cfr_flow_align((const float*)op->p[0], (const float*)op->p[1], (const float*)op->t, H, W, (int64_t*)op->p[2],
                                    (float*)op->p[3], nullptr, stream);
    case DEMFI_OP_WARP:
        if (op->bt.nb > 1)
            return demfi_warp_blend_batched(&op->a, (const float*)op->p[0], &op->b, (const float*)op->p[1], (const float*)op->p[2],
                                            (const float*)op->t, &op->o, op->nch, H, W, (float*)op->p[3], (void*)op->p[4], c->dtype, &op->bt, stream);
        if (op->p[4])
            return demfi_warp_blend_pack(&op->a, (const float*)op->p[0], &op->b, (const float*)op->p[1], (const float*)op->p[2],
                                         (const float*)op->t, &op->o, H, W, (float*)op->p[3], (void*)op->p[4], c->dtype, stream);
        return demfi_warp_blend(&op->a, (const float*)op->p[0], &op->b, (const float*)op->p[1], (const float*)op->p[2],
                                (const float*)op->t, &op->o, op->nch, H, W, (float*)op->p[3], nullptr, stream);
    }
    return demfi_set_error(DEMFI_ERR_ARG, "demfi_run_op: unknown op kind %d", op->kind);
}
