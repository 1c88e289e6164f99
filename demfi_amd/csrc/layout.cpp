// Where every buffer of a context lives inside the ONE caller-owned workspace: the layout, and the liveness arena that lets buffers of a
// set that are never alive together share memory.  Host logic only.
#include "plan.h"
#include <algorithm>
#include <stdlib.h>

namespace plan {

namespace {

// ---- buffer layout ---------------------------------------------------------------------------------------------
struct Layout {
    demfi_ctx* c;
    int64_t cur;
    int rep = 0;               // > 0: per-t buffers, `rep` copies of every buffer back to back (copy q at off + q * cstride)
    const ArenaPlan* plan = nullptr;   // buffers named in it live at arena_base + their planned offset
    int64_t arena_base = 0;
    int64_t take(int64_t bytes) { const int64_t o = cur; cur = (cur + bytes + 255) & ~255ll; return o; }
    static int64_t footprint(const Tensor& t, int rep) { return rep > 0 ? ((t.bytes + 15) & ~15ll) * rep : t.bytes; }
    void place(Tensor& t, const char* n)
    {
        if (rep > 0) t.cstride = (t.bytes + 15) & ~15ll;
        const int64_t fp = footprint(t, rep);
        auto it = plan && plan->on ? plan->off.find(n) : std::map<std::string, int64_t>::const_iterator();
        if (plan && plan->on && it != plan->off.end()) {
            t.off = arena_base + it->second;
            if (rep > 0) t.cstride = plan->cstride;              // arena members of a per-t set: copy q sits q SLOTS further (see plan_arena)
        } else t.off = take(fp);
        t.id = (int)c->id_cstride.size();
        c->id_cstride.push_back(t.cstride);
    }
    void begin_set(const ArenaPlan* pl)
    {
        plan = pl;
        if (pl && pl->on) arena_base = take(pl->size);
    }
    void fat(BufSet& s, const char* n, int h, int w, int ch, int b = 1)
    {
        Tensor t; t.kind = 0; t.d[0] = b; t.d[1] = h; t.d[2] = w; t.d[3] = ch;
        t.bytes = (int64_t)b * h * w * ch * esz_of(c); place(t, n); s[n] = t;
    }
    void thin(BufSet& s, const char* n, int ch, int h, int w)
    {
        Tensor t; t.kind = 1; t.d[0] = ch; t.d[1] = h; t.d[2] = w; t.d[3] = 1;
        t.bytes = (int64_t)ch * h * w * 4; place(t, n); s[n] = t;
    }
    void raw(BufSet& s, const char* n, int64_t bytes)
    {
        Tensor t; t.kind = 2; t.d[0] = (int)(bytes / 8); t.d[1] = t.d[2] = t.d[3] = 1;
        t.bytes = bytes; place(t, n); s[n] = t;
    }
};

void alloc_trunk(Layout& L, BufSet& s)
{
    const int H = L.c->H, W = L.c->W, H2 = H / 2, W2 = W / 2;
    L.thin(s, "x", 12, H, W);                       // module input [3,4,H,W], batch 1
    L.fat(s, "s2d", H2, W2, 48);
    L.fat(s, "f1", H2, W2, 96);
    L.fat(s, "x0", H2, W2, 96);
    L.fat(s, "grow", H2, W2, 128);
    L.fat(s, "gffcat", H2, W2, 1152);
    L.fat(s, "g0", H2, W2, 96);
    L.fat(s, "g1", H2, W2, 96);
    L.fat(s, "up", H, W, 64);
    L.fat(s, "F01", H, W, 64, 2);
    L.thin(s, "ffo", 5, H, W);                      // flow_01 (2), flow_10 (2), occ_0 logit (1)
    L.fat(s, "enc_a", H, W, 64, 2);
    L.fat(s, "enc_t", H, W, 64, 2);
    L.fat(s, "enc_b", H, W, 64, 2);
    L.fat(s, "rk", H, W, 64, 2);
    if (L.c->hp.fgac_rr > 0) {
        L.fat(s, "skk", H, W, 64, 2);               // conv_source_k(source): live only in the generalised FGAC
        if (L.c->hp.fgac_sr > 0) { L.fat(s, "rkp", H, W, 64, 2); L.fat(s, "skp", H, W, 64, 2); }
    }
    L.fat(s, "smp", H, W, 64, 2);
    L.fat(s, "E", H, W, 64, 2);
    L.fat(s, "wg", H, W, 64, 2);
    L.thin(s, "gate", 2, H, W);
    L.fat(s, "aF", H, W, 64, 2);
    L.thin(s, "overlay", 3, H, W);
    if (L.c->hp.flags & DEMFI_HP_EXTRAS) {
        // per FGAC direction b (0: F1 -> F0, 1: F0 -> F1), planes 6 b + {0: 1 - w_sr, 1: source_v, 2: init_ref_k, 3: E_s, 4: bolstered_F_s,
        // 5: diff}: the min-max normalised channel means of DeMFInet.py:454-494 (w_sr itself is the "gate" buffer)
        L.thin(s, "viz", 12, H, W);
        L.thin(s, "vizs", 1, 1, (int)demfi_minmax_scratch_floats());
    }
    if (L.c->dtype == DEMFI_F16) {
        L.fat(s, "u1a", H2, W2, 64);                // t-independent part of Refine_Module.enc1 (see build_trunk)
        L.fat(s, "xff16", H, W, 16);                // window-constant planes of the Mixer / D2 inputs: 4 frames x 3 colours | flow_10, flow_01
        L.fat(s, "re1w", H, W, 32);                 // their share of Mixer.conv_ref1 ...
        L.fat(s, "g_pw", H, W, 64);                 // ... and of Dec_first_2
    }
}

// buffers of a single-call operator context (all in the "trunk" set: demfi_ctx_buffer(ctx, 0, -1, name, ...))
void alloc_operator(Layout& L, BufSet& s)
{
    const int H = L.c->H, W = L.c->W, B = L.c->op_batch;
    if (L.c->op_kind == 1) {
        for (const char* n : {"h", "x", "z", "rh", "h1", "out"}) L.fat(s, n, H, W, 64, B);
    } else {
        for (const char* n : {"ref", "source", "ref_k", "sampled", "e_s", "hid", "out"}) L.fat(s, n, H, W, 64, B);
        L.thin(s, "flow", 2 * B, H, W);                          // flow_s2r [B,2,H,W] fp32 (absolute sampling coordinates)
        L.thin(s, "w", B, H, W);                                 // the gate w_sr [B,1,H,W]
    }
}

void alloc_t(Layout& L, BufSet& s)
{
    const int H = L.c->H, W = L.c->W, N = L.c->N;
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
    L.thin(s, "t", 1, 1, 1);
    L.raw(s, "sink", 256);                          // demfi_u8_sink record (zero = disabled: iter 0 with NULL frames writes nothing)
    L.raw(s, "cfr_acc", demfi_cfr_workspace_bytes(H, W));
    L.thin(s, "ft", 4, H, W);                       // flow_t0, flow_t1
    L.fat(s, "Ft", H, W, 64);
    L.fat(s, "u1", H2, W2, 64);
    L.fat(s, "u2", H4, W4, 128);
    L.fat(s, "u3", H8, W8, 256);
    L.fat(s, "d0", H8, W8, 256);
    L.fat(s, "d1", H4, W4, 128);
    L.fat(s, "d2", H2, W2, 64);
    L.fat(s, "rF", H, W, 64, 3);                    // rF0, rF1, rFt
    L.thin(s, "delta", 5 * (N + 1), H, W);          // (flow_t0, flow_t1, occ logit) per step
    L.thin(s, "occ", N + 1, H, W);                  // sigmoid(occ logit) per step
    L.fat(s, "dec_a", H, W, 64, 3);
    L.fat(s, "dec_t", H, W, 64, 3);
    L.fat(s, "dec_b", H, W, 64, 3);
    L.thin(s, "sharp1", 9, H, W);                   // S0p, S1p, Stp
    L.fat(s, "frec0", H, W, 64);
    L.fat(s, "frec1", H, W, 64);
    L.fat(s, "re1", H, W, 32);
    // Mixer.conv_ref2 | conv_delta2 outputs as the two 32-channel halves of ONE 64-channel buffer: conv_blend1 (cat[ref, delta],
    // DeMFInet.py:826-827) then stages a single 128-byte record per pixel (the narrow kernel's fast DMA path) instead of two pieces
    L.fat(s, "rd64", H, W, 64);
    L.fat(s, "de1", H, W, 32);
    L.fat(s, "bl1", H, W, 32);
    L.fat(s, "xb", H, W, 64);
    L.fat(s, "zb", H, W, 64);
    L.fat(s, "rh", H, W, 64);
    L.fat(s, "h1", H, W, 64);
    L.fat(s, "fo1", H, W, 32);
    L.thin(s, "stnew", 3, H, W);
    // planar flows / logits / frames packed to NHWC once, so the consuming convs stage them with vector loads
    L.fat(s, "misc16", H, W, 16);
    if (L.c->dtype == DEMFI_F16) L.fat(s, "ref16", H, W, 16);     // per-t planes only (fp16 plan): S0p, S1p, Stp | rflow_t0, rflow_t1, occ logit | occ_0 | 0
    else { L.fat(s, "ref32", H, W, 32); L.fat(s, "agg3s", H, W, 32); }
    L.fat(s, "agg3d", H, W, 8);
    L.fat(s, "delta16", H, W, 16);               // 5 flow / occlusion planes + 11 zero channels: a full 32-byte record (one DMA piece)
    L.fat(s, "g_a", H, W, 64);
    L.fat(s, "g_t", H, W, 64);
    L.fat(s, "g_b", H, W, 64);
    if (L.c->dtype == DEMFI_F16) L.fat(s, "g_p2", H, W, 64);     // partial sum of Dec_first_2 (everything but the F_rec part)
    L.thin(s, "finals", 9 * N, H, W);               // [N][3 frames][3 colours]
}

}  // namespace

void compute_layout(demfi_ctx* c, int64_t w_bytes, int64_t n_descs)
{
    Layout L{c, 0};
    c->w_region = L.take(0);
    c->w_bytes = (w_bytes + 255) & ~255ll;
    L.take(c->w_bytes);
    c->zero_off = L.take(256);
    c->n_descs = n_descs;
    c->desc_off = L.take(n_descs * (int64_t)sizeof(demfi_conv));
    c->tr_bufs.assign(c->n_trunk, BufSet());
    c->t_bufs.assign(c->n_trunk, std::vector<BufSet>(c->n_ctx));
    c->id_cstride.assign(1, 0);
    if (c->op_kind) {
        alloc_operator(L, c->tr_bufs[0]);
        c->total = L.cur;
        return;
    }
    for (int k = 0; k < c->n_trunk; ++k) {
        L.begin_set(&c->arena_tr);
        alloc_trunk(L, c->tr_bufs[k]);
        // tensor-major: the n_ctx copies of a per-t buffer are contiguous, so a convolution over "batch x n_ctx" addresses
        // all of them with one batch stride (demfi_forward_tb)
        L.rep = c->n_ctx;
        L.begin_set(&c->arena_t);
        alloc_t(L, c->t_bufs[k][0]);
        L.rep = 0;
        L.begin_set(nullptr);
        for (int q = 1; q < c->n_ctx; ++q) {
            c->t_bufs[k][q] = c->t_bufs[k][0];
            for (auto& kv : c->t_bufs[k][q]) kv.second.off += q * kv.second.cstride;
        }
    }
    c->total = L.cur;
}

namespace {

// ---- workspace arena (round 5) -----------------------------------------------------------------------------------
// Every pointer an op reads / writes (write = true).  The scratch buffer between the two convolutions of a fused residual block is
// not touched by the fused launch.
void op_accesses(const demfi_ctx* c, const demfi_op& op, std::vector<std::pair<const void*, bool>>& out)
{
    auto rd = [&](const void* p) { if (p) out.push_back({p, false}); };
    auto wr = [&](const void* p) { if (p) out.push_back({p, true}); };
    auto conv_in = [&](const demfi_conv& d) { for (int i = 0; i < d.n_pieces; ++i) rd(d.pieces[i].v.ptr); };
    auto conv_out = [&](const demfi_conv& d) {
        for (int i = 0; i < d.n_segs; ++i) { rd(d.segs[i].res.ptr); rd(d.segs[i].aux.ptr); wr(d.segs[i].dst.ptr); }
        wr(d.pack.ptr);
    };
    switch (op.kind) {
    case DEMFI_OP_CONV: conv_in(c->descs[op.conv]); conv_out(c->descs[op.conv]); break;
    case DEMFI_OP_RESBLOCK: conv_in(c->descs[op.conv]); conv_out(c->descs[op.nch]); break;
    case DEMFI_OP_GRU_R: conv_in(c->descs[op.conv]); conv_out(c->descs[op.conv]); break;
    case DEMFI_OP_GRU_ZQ: {                                      // reads h, x, r*h; writes h'; the z buffer (convz's dst == convq's aux) is not touched
        const demfi_conv& dq = c->descs[op.nch];
        conv_in(c->descs[op.conv]); conv_in(dq);
        for (int i = 0; i < dq.n_segs; ++i) { rd(dq.segs[i].res.ptr); wr(dq.segs[i].dst.ptr); }
        break;
    }
    case DEMFI_OP_PACK: for (int i = 0; i < 32; ++i) rd(op.p[i]); wr(op.o.ptr); break;
    case DEMFI_OP_VIZ: rd(op.a.ptr); rd(op.b.ptr); rd(op.p[1]); if (op.conv == 1) { rd(op.p[0]); wr(op.p[1]); } wr(op.p[0]); break;
    case DEMFI_OP_S2D: case DEMFI_OP_OVERLAY: rd(op.p[0]); wr(op.p[1]); break;
    case DEMFI_OP_FGAC: rd(op.a.ptr); rd(op.p[0]); wr(op.o.ptr); break;
    case DEMFI_OP_FGAC_WINDOW: rd(op.a.ptr); rd(op.b.ptr); rd(op.p[0]); wr(op.o.ptr); break;
    case DEMFI_OP_AVG_POOL: rd(op.a.ptr); wr(op.o.ptr); break;
    case DEMFI_OP_GATE: rd(op.p[0]); rd(op.a.ptr); rd(op.b.ptr); wr(op.o.ptr); break;
    case DEMFI_OP_CFR: rd(op.p[0]); rd(op.p[1]); rd(op.p[2]); rd(op.p[4]); wr(op.p[2]); wr(op.p[3]); wr(op.p[5]); rd(op.t); break;
    case DEMFI_OP_WARP: rd(op.a.ptr); rd(op.b.ptr); rd(op.p[0]); rd(op.p[1]); rd(op.p[2]); rd(op.t); wr(op.o.ptr); wr(op.p[3]); wr(op.p[4]); break;
    default: break;
    }
}

// Liveness plan of one buffer set from its launch sequence (built on the UNALIASED layout of the sizing pass, where an address
// names one buffer).  Candidates: the buffers in `allow` whose first access is a write by an op of `seq` and which no op of
// `foreign` (another segment) touches; a candidate lives from its first to its last access (buffers that carry state from one
// recursion to the next are accessed in several: their interval spans them).  Everything else keeps memory of its own: inputs,
// outputs the host reads, buffers that rely on the zero-filled workspace (the CFR accumulator, zero-padded records).  Footprints
// (all n_ctx copies of a buffer: the tensor-major layout stays) are packed first-fit, largest first.
// does op (re)write EVERY element of tensor t (all images, all channels)?  Then whatever t held before is dead: its live range
// may end at the previous access and a new one starts here (per-recursion scratch is alive only inside each recursion).
bool op_overwrites(const demfi_ctx* c, const demfi_op& op, const Tensor& t, int64_t t_addr)
{
    if (t.kind != 0) return false;
    auto conv_full = [&](const demfi_conv& d) {
        if (d.H != t.d[1] || d.W != t.d[2] || d.batch != t.d[0]) return false;
        for (int sg = 0; sg < d.n_segs; ++sg) {
            const demfi_seg& g = d.segs[sg];
            if ((int64_t)(intptr_t)g.dst.ptr != t_addr || g.mode != DEMFI_MODE_STORE && g.mode != DEMFI_MODE_MUL && g.mode != DEMFI_MODE_GRU) continue;
            if (g.scale != 1 || g.dst.sc != 1 || g.dst.sx != t.d[3]) continue;
            int n = 0;
            for (int o = 0; o < d.cout_pad / 8; ++o) if (d.oct_seg[o] == sg) n += d.oct_n[o];
            if (n == t.d[3]) return true;
        }
        return false;
    };
    if (op.kind == DEMFI_OP_CONV) return conv_full(c->descs[op.conv]);
    if (op.kind == DEMFI_OP_RESBLOCK || op.kind == DEMFI_OP_GRU_ZQ) return conv_full(c->descs[op.nch]);
    if (op.kind == DEMFI_OP_GRU_R) return conv_full(c->descs[op.conv]);
    if (op.kind == DEMFI_OP_PACK) return (int64_t)(intptr_t)op.o.ptr == t_addr && op.nch == t.d[3] && t.d[0] == 1;
    return false;
}

}  // namespace

ArenaPlan plan_arena(const demfi_ctx* c, const BufSet& set, int rep, const std::vector<const OpList*>& seq,
                     const std::vector<const OpList*>& foreign, const std::vector<std::string>& allow)
{
    struct Iv { std::string name; int64_t size; std::vector<std::pair<int, int>> live; bool ok = true; int64_t off = -1; };
    std::vector<Iv> iv;
    const char* only = getenv("DEMFI_ARENA_ONLY");              // debugging: restrict the arena to the named buffers ("a,b,c")
    for (const auto& n : allow) {
        if (only && (std::string(",") + only + ",").find("," + n + ",") == std::string::npos) continue;
        auto it = set.find(n);
        if (it != set.end()) iv.push_back({n, (Layout::footprint(it->second, rep) + 255) & ~255ll});
    }
    auto find = [&](const void* p) -> Iv* {
        const int64_t a = (int64_t)(intptr_t)p;                  // sizing pass: base == nullptr, pointers are offsets
        for (auto& x : iv) {
            const Tensor& t = set.find(x.name)->second;
            if (a >= t.off && a < t.off + t.bytes) return &x;
        }
        return nullptr;
    };
    std::vector<std::pair<const void*, bool>> acc;
    int idx = 0;
    for (const OpList* ops : seq)
        for (const demfi_op& op : *ops) {
            acc.clear();
            op_accesses(c, op, acc);
            for (int pass = 0; pass < 2; ++pass)                 // an op's reads come before its writes
                for (auto& a : acc) {
                    if ((int)a.second != pass) continue;
                    Iv* x = find(a.first);
                    if (!x) continue;
                    const Tensor& t = set.find(x->name)->second;
                    if (x->live.empty()) {
                        if (!a.second) x->ok = false;             // read before any write: it relies on what the workspace held
                        x->live.push_back({idx, idx});
                    } else if (a.second && x->live.back().second < idx && op_overwrites(c, op, t, t.off)) {
                        x->live.push_back({idx, idx});            // everything it held is replaced: a new live range
                    } else x->live.back().second = idx;
                }
            ++idx;
        }
    for (const OpList* ops : foreign)
        for (const demfi_op& op : *ops) {
            acc.clear();
            op_accesses(c, op, acc);
            for (auto& a : acc) if (Iv* x = find(a.first)) x->ok = false;
        }
    ArenaPlan pl;
    std::vector<Iv*> todo;
    for (auto& x : iv) {
        if (x.live.empty()) { pl.off[x.name] = 0; continue; }    // never touched (the scratch of fused residual blocks): no memory
        if (x.ok) todo.push_back(&x);
    }
    std::sort(todo.begin(), todo.end(), [](const Iv* a, const Iv* b) { return a->size != b->size ? a->size > b->size : a->live[0].first < b->live[0].first; });
    auto together = [](const Iv* a, const Iv* b) {
        for (auto& p : a->live) for (auto& q : b->live) if (!(p.second < q.first || q.second < p.first)) return true;
        return false;
    };
    std::vector<Iv*> placed;
    if (rep > 0) {
        // Per-t set: the arena is a row of SLOTS.  A slot holds, per context, S bytes (S = the largest member: the 3-image buffers
        // of D1); context q's share of slot j is [j * rep * S + q * S, + S).  A member lives at (slot, offset < S) with context stride
        // S, so everything context q ever touches lies inside ITS shares: per-t contexts stay independent of one another (they
        // may run concurrently on different streams, demfi_forward_t) while buffers of one context that are never alive together
        // share memory.  A multi-image member fills a slot exactly (its images tile the context stride, as the batched plan needs).
        int64_t S = 0;
        for (Iv* x : todo) x->size = (Layout::footprint(set.find(x->name)->second, 1) + 255) & ~255ll;     // bytes per context
        for (Iv* x : todo) S = std::max(S, x->size);
        std::vector<Iv*> keep;
        for (Iv* x : todo) {
            const Tensor& t = set.find(x->name)->second;
            if (t.kind == 0 && t.d[0] > 1 && ((t.bytes + 15) & ~15ll) != S) { x->ok = false; continue; }   // its images would not tile the slot stride
            keep.push_back(x);
        }
        todo.swap(keep);
        std::sort(todo.begin(), todo.end(), [](const Iv* a, const Iv* b) { return a->size != b->size ? a->size > b->size : a->live[0].first < b->live[0].first; });
        std::vector<int> slot_of;
        int n_slots = 0;
        for (Iv* x : todo) {
            int64_t o = -1;
            int sj = 0;
            for (; o < 0; ++sj) {
                std::vector<std::pair<int64_t, int64_t>> busy;
                for (size_t i = 0; i < placed.size(); ++i)
                    if (slot_of[i] == sj && together(x, placed[i])) busy.push_back({placed[i]->off, placed[i]->off + placed[i]->size});
                std::sort(busy.begin(), busy.end());
                int64_t f = 0;
                for (auto& b : busy) { if (f + x->size <= b.first) break; f = std::max(f, b.second); }
                if (f + x->size <= S) { o = f; break; }
            }
            x->off = o;
            placed.push_back(x);
            slot_of.push_back(sj);
            n_slots = std::max(n_slots, sj + 1);
            pl.off[x->name] = (int64_t)sj * rep * S + o;
        }
        pl.cstride = S;
        pl.size = (int64_t)n_slots * rep * S;
        for (size_t i = 0; i < placed.size(); ++i) placed[i]->off += (int64_t)slot_of[i] * rep * S;      // for the debug print
    } else
    for (Iv* x : todo) {
        std::vector<std::pair<int64_t, int64_t>> busy;           // address ranges of placed buffers alive at the same time
        for (Iv* y : placed) if (together(x, y)) busy.push_back({y->off, y->off + y->size});
        std::sort(busy.begin(), busy.end());
        int64_t o = 0;
        for (auto& b : busy) { if (o + x->size <= b.first) break; o = std::max(o, b.second); }
        x->off = o;
        placed.push_back(x);
        pl.off[x->name] = o;
        pl.size = std::max(pl.size, o + x->size);
    }
    if (getenv("DEMFI_ARENA_DEBUG"))
        for (auto& x : iv) {
            fprintf(stderr, "   %-8s ok=%d off=%8.1f MB size=%7.1f MB live", x.name.c_str(), (int)x.ok, x.off / 1e6, x.size / 1e6);
            for (auto& p : x.live) fprintf(stderr, " [%d,%d]", p.first, p.second);
            fprintf(stderr, "\n");
        }
    pl.size = std::max<int64_t>(pl.size, 256);                   // never-touched members point at the arena's first bytes
    pl.on = !placed.empty();
    if (!pl.on) pl.off.clear();
    return pl;
}

}  // namespace plan
