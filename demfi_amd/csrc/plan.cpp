// The launch plan of the DeMFI-Net_rb inference forward: one demfi_conv descriptor per convolution call site, the state_dict repacked
// into MFMA fragment order (each layer once, shared by all contexts) and the launch sequence of the kernels of conv.hip / pointwise.hip.
// Host logic only.
//
// The plan follows the data flow of DeMFInet.forward (the reference's DeMFInet.py:46-179) but not its execution shape:
//   * every torch.cat is a multi-piece input of the consuming convolution (no concat buffers);
//   * RDB dense blocks grow in place, LFF outputs land directly in the 1152-channel GFF input;
//   * PixelShuffle / NN-upsample / tanh / sigmoid / ReLU / residual adds / GRU gate math are epilogues or fused loads;
//   * the t-independent trunk (FF_RDB + FAC-FB, 37 % of the MACs) is its own segment;
//   * Mixer.conv_ref1/2 do not depend on the recursion index and are hoisted out of the boosting loop.
// Flows, occlusion logits and 3-channel frames stay fp32 planar ("thin"); features are NHWC in the path dtype ("fat").
#include "plan.h"
#include <algorithm>
#include <string.h>

namespace plan {

void layer_table(demfi_ctx* c)
{
    // the reference's registration order and shapes (DeMFInet.py:15-44, 189-231, 319-333, 361-378, 566-584, 770-868;
    // SURVEY.md Appendix A/B) -- mirrored by demfi_amd/spec.py for the module surface
    auto& t = c->table;
    if (c->op_kind == 1) {                                       // SepConvGRU (DeMFInet.py:830-836): keys of the reference module
        for (const char* g : {"z", "r", "q"}) t[std::string("conv") + g + "1"] = {64, 128, 1, 5};
        for (const char* g : {"z", "r", "q"}) t[std::string("conv") + g + "2"] = {64, 128, 5, 1};
        return;
    }
    if (c->op_kind == 2) {                                       // FGAC (DeMFInet.py:369-380); conv_source_k is accepted and dead at rr = 0
        t["conv_ref_k"] = {64, 64, 1, 1}; t["conv_source_k"] = {64, 64, 1, 1}; t["fusion"] = {64, 64, 1, 1};
        t["w_gen"] = {64, 128, 3, 3}; t["w_gen_2"] = {1, 64, 3, 3};
        return;
    }
    const int nf = c->hp.nf, r2 = c->hp.scale_factor * c->hp.scale_factor;
    const int G0 = 96, G = 32, Cn = 4, D = 12;
    auto add = [&](const std::string& n, int cout, int cin, int kh, int kw) { t[n] = {cout, cin, kh, kw}; };
    std::string p = "FF_RDB_Module.";
    add(p + "SFENet1", G0, 12 * r2, 5, 5);
    add(p + "SFENet2", G0, G0, 3, 3);
    for (int i = 0; i < D; ++i) {
        for (int k = 0; k < Cn; ++k) add(p + "RDBs." + std::to_string(i) + ".convs." + std::to_string(k) + ".conv.0", G, G0 + k * G, 3, 3);
        add(p + "RDBs." + std::to_string(i) + ".LFF", G0, G0 + Cn * G, 1, 1);
    }
    add(p + "GFF.0", G0, D * G0, 1, 1);
    add(p + "GFF.1", G0, G0, 3, 3);
    add(p + "UPNet.0", 256, G0, 3, 3);
    add(p + "UPNet.2", 2 * nf + 5, 64, 3, 3);
    p = "FAC_FB_Module.";
    add(p + "conv_first", nf, nf, 3, 3);
    for (int i = 0; i < c->hp.num_resb_facfb; ++i) {
        add(p + "feature_extraction." + std::to_string(i) + ".conv1", nf, nf, 3, 3);
        add(p + "feature_extraction." + std::to_string(i) + ".conv2", nf, nf, 3, 3);
    }
    std::vector<std::string> fg = c->hp.shared_fgac ? std::vector<std::string>{"shared_FGAC"}
                                                    : std::vector<std::string>{"FGAC_F1toF0", "FGAC_F0toF1"};
    for (auto& f : fg) {
        add(p + f + ".conv_ref_k", nf, nf, 1, 1);
        add(p + f + ".conv_source_k", nf, nf, 1, 1);
        add(p + f + ".w_gen", nf, 2 * nf, 3, 3);
        add(p + f + ".w_gen_2", 1, nf, 3, 3);
        add(p + f + ".fusion", nf, nf, 1, 1);
    }
    p = "Refine_Module.";
    add(p + "enc1", nf, 3 * nf + 9, 4, 4);
    add(p + "enc2", 2 * nf, nf, 4, 4);
    add(p + "enc3", 4 * nf, 2 * nf, 4, 4);
    add(p + "dec0", 4 * nf, 4 * nf, 3, 3);
    add(p + "dec1", 2 * nf, 6 * nf, 3, 3);
    add(p + "dec2", nf, 3 * nf, 3, 3);
    add(p + "dec3", 2 * nf + 5, nf, 3, 3);
    add("Dec_first", nf, nf, 3, 3);
    for (int i = 0; i < c->hp.num_resb_dec; ++i) {
        add("Decoder_res." + std::to_string(i) + ".conv1", nf, nf, 3, 3);
        add("Decoder_res." + std::to_string(i) + ".conv2", nf, nf, 3, 3);
    }
    add("Dec_last1", nf, nf, 3, 3);
    add("Dec_last2", 3, nf, 3, 3);
    add("Ch_Reducer", nf, 3 * nf, 7, 7);
    p = "Booster_Module.";
    add(p + "Mixer.conv_ref1", nf / 2, 30, 7, 7);
    add(p + "Mixer.conv_ref2", nf / 2, nf / 2, 3, 3);
    add(p + "Mixer.conv_delta1", nf / 2, 5, 7, 7);
    add(p + "Mixer.conv_delta2", nf / 2, nf / 2, 3, 3);
    add(p + "Mixer.conv_blend1", nf / 2, nf, 3, 3);
    add(p + "Mixer.conv_blend2", nf, nf / 2, 3, 3);
    for (const char* g : {"z", "r", "q"}) add(p + "GB.conv" + g + "1", nf, 2 * nf, 1, 5);
    for (const char* g : {"z", "r", "q"}) add(p + "GB.conv" + g + "2", nf, 2 * nf, 5, 1);
    add(p + "flow_occ.conv1", nf / 2, nf, 3, 3);
    add(p + "flow_occ.conv2", 5, nf / 2, 3, 3);
    add("Dec_first_2", nf, 9 + nf + 9 + 5 + 12, 3, 3);
    for (int i = 0; i < c->hp.num_resb_dec; ++i) {
        add("Decoder_res_2." + std::to_string(i) + ".conv1", nf, nf, 3, 3);
        add("Decoder_res_2." + std::to_string(i) + ".conv2", nf, nf, 3, 3);
    }
    add("Dec_last1_2", nf, nf, 3, 3);
    add("Dec_last2_2", 9, nf, 3, 3);
}

namespace {

// ---- plan builder ----------------------------------------------------------------------------------------------
struct Src { demfi_view v; int fat, up; std::vector<int32_t> cin; };
struct Dst { demfi_view dst, res, aux; int act, mode, scale, dy, dx; std::vector<int32_t> couts; };

std::vector<int32_t> range(int a, int b) { std::vector<int32_t> r; for (int i = a; i < b; ++i) r.push_back(i); return r; }
const demfi_view NOVIEW = {nullptr, 0, 0, 0, 0, 0, 0};

// Weights of a call site that are not one whole layer.  Sub-convolution over some input channels of a layer: a convolution is linear
// in its input channels, so conv(cat[A, B]) = conv_A(A) + conv_B(B); the fp16 plan uses it to hoist the part of a layer whose inputs do
// not change (per window / per recursion) and to bring the rest onto the persistent kernels.  Empty w / b in the sizing pass.
struct SubW { std::vector<float> w, b; Layer shape; };

// What a conv() call site may ask for besides sources and destinations.
struct ConvOpt {
    int stride = 1, batch = 1, pad_y = -1, pad_x = -1;       // pads < 0: the layer's own
    const SubW* sub = nullptr;                               // weights of its own instead of layer `name`'s
    const demfi_u8_sink* sink = nullptr;                     // uint8 sink record (the frame-producing layer Dec_last2_2 only) ...
    int sink_iter = 0;                                       // ... and the recursion it writes for
    // packed copy of the thin outputs (demfi_conv.pack): NHWC view + channel of each octet (-1 = not packed)
    demfi_view pack = {nullptr, 0, 0, 0, 0, 0, 0};
    int pack_ch[4] = {-1, -1, -1, -1};
    ConvOpt& strided(int s) { stride = s; return *this; }
    ConvOpt& batched(int n) { batch = n; return *this; }
    ConvOpt& weights(const SubW& w) { sub = &w; return *this; }
    ConvOpt& to_sink(const void* record, int iter) { sink = (const demfi_u8_sink*)record; sink_iter = iter; return *this; }
    ConvOpt& packed(demfi_view v, int c0, int c1 = -1, int c2 = -1, int c3 = -1)
    {
        pack = v;
        pack_ch[0] = c0; pack_ch[1] = c1; pack_ch[2] = c2; pack_ch[3] = c3;
        return *this;
    }
};

struct Builder {
    demfi_ctx* c;
    int esz;
    bool f32;
    bool dry;                  // sizing pass of demfi_ctx_create: no weights, nothing is written
    int status = DEMFI_OK;
    // ---- batched per-t plan (demfi_forward_tb): build_t on context 0 of trunk set tb_k with tb = n_ctx -----------------
    int tb = 1, tb_k = 0;
    // the buffer a device pointer lies in: per-t buffer of context 0 (returns its context stride in bytes), trunk buffer (0),
    // or neither (-1: weights, zero page, NULL)
    int64_t ctx_stride_of(const void* p) const
    {
        if (!p) return -1;
        const int64_t off = (const char*)p - c->base;
        for (const auto& kv : c->t_bufs[tb_k][0])
            if (off >= kv.second.off && off < kv.second.off + kv.second.bytes) return kv.second.cstride;
        for (const auto& kv : c->tr_bufs[tb_k])
            if (off >= kv.second.off && off < kv.second.off + kv.second.bytes) return 0;
        return -1;
    }
    // context stride of a view: by the id of the tensor it was built from (buffers of the arena share addresses, so an address does
    // not name a buffer any more); raw pointers (thin planes: never in the arena) by address
    int64_t view_stride(const demfi_view& v) const
    {
        if (v._pad > 0 && v._pad < (int)c->id_cstride.size()) return c->id_cstride[v._pad];
        return ctx_stride_of(v.ptr);
    }
    // view of a convolution of the batched plan: the conv runs with batch nb * tb, image index = q * nb + f
    bool tb_view(demfi_view& v, int nb, const char* name)
    {
        if (!v.ptr) return true;
        const int64_t cs = view_stride(v), elt = v.is_f32 ? 4 : 2;
        v._pad = 0;
        if (cs < 0) { status = demfi_set_error(DEMFI_ERR_ARG, "%s: view outside the context's buffers in the batched plan", name); return false; }
        if (cs == 0) {                                           // trunk buffer: the same image for every context
            if (nb != 1 && v.sb != 0) { status = demfi_set_error(DEMFI_ERR_ARG, "%s: batched trunk view in a batch-%d layer", name, nb); return false; }
            v.sb = 0;
        } else if (nb == 1) v.sb = cs / elt;                     // one image per context
        else if (v.sb * nb * elt != cs) {                        // nb images per context: they must tile the context stride
            status = demfi_set_error(DEMFI_ERR_ARG, "%s: %d images of stride %lld do not tile the context stride %lld", name, nb,
                                     (long long)(v.sb * elt), (long long)cs);
            return false;
        }
        return true;
    }
    const void* tb_ptr(const void* p, int q) const
    {
        const int64_t cs = ctx_stride_of(p);
        return cs > 0 ? (const char*)p + q * cs : p;
    }

    char* ptr(const Tensor& t) const { return c->base + t.off; }
    // input piece from a fat buffer [B,h,w,C]: channels [c0, c0+nch) feed original cin [cin0, cin0+nch); b < 0 keeps the
    // batch stride (batched conv), b >= 0 pins image b
    Src fsrc(const Tensor& t, int cin0, int c0 = 0, int nch = -1, int b = -1, int up = 0) const
    {
        if (nch < 0) nch = t.d[3] - c0;
        return Src{fview(t, c0, b), 1, up, range(cin0, cin0 + nch)};
    }
    // ALL channels of a fat buffer with an explicit channel -> original-cin list (-1 = unused padding channel)
    Src fsrc_map(const Tensor& t, const std::vector<int32_t>& cin, int b = 0) const
    {
        return Src{fview(t, 0, b), 1, 0, cin};
    }
    demfi_view fview(const Tensor& t, int c0 = 0, int b = -1) const
    {
        const int h = t.d[1], w = t.d[2], Ct = t.d[3];
        return {ptr(t) + ((int64_t)c0 + (b < 0 ? 0 : (int64_t)b * h * w * Ct)) * esz, Ct, (int64_t)w * Ct, 1,
                b < 0 ? (int64_t)h * w * Ct : 0, f32 ? 1 : 0, t.id};
    }
    demfi_view tview(const Tensor& t, int c0 = 0, int64_t sb = 0) const
    {
        const int h = t.d[1], w = t.d[2];
        return {ptr(t) + (int64_t)c0 * h * w * 4, 1, w, (int64_t)h * w, sb, 1, t.id};
    }
    const float* plane(const Tensor& t, int ch) const { return (const float*)(ptr(t) + (int64_t)ch * t.d[1] * t.d[2] * 4); }
    static Dst D(demfi_view v, std::vector<int32_t> couts, int act = DEMFI_ACT_NONE, int mode = DEMFI_MODE_STORE,
                 demfi_view res = NOVIEW, demfi_view aux = NOVIEW, int scale = 1, int dy = 0, int dx = 0)
    {
        return Dst{v, res, aux, act, mode, scale, dy, dx, std::move(couts)};
    }

    int64_t blob_put(const void* p, int64_t n)
    {
        const int64_t off = c->blob_fill;
        if (!dry) {
            if (off + n > c->w_bytes) { status = demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_bind: weight region too small"); return 0; }
            memcpy(c->host_blob.data() + off, p, n);
        }
        c->blob_fill = (off + n + 255) & ~255ll;
        return off;
    }

    // A layer's shape, weight [cout,cin,kh,kw] and bias [cout]; in the sizing pass the shape and no data (w = b = nullptr).
    struct Found { Layer l; const std::vector<float>*w, *b; };
    bool lookup(const std::string& name, Found& f)
    {
        auto it = c->table.find(name);
        auto iw = c->weights.find(name + ".weight"), ib = c->weights.find(name + ".bias");
        if (it == c->table.end() || (!dry && (iw == c->weights.end() || ib == c->weights.end()))) {
            status = demfi_set_error(DEMFI_ERR_ARG, it == c->table.end() ? "unknown layer '%s'" : "demfi_ctx_bind: weight '%s' was not loaded", name.c_str());
            return false;
        }
        f = {it->second, dry ? nullptr : &iw->second.data, dry ? nullptr : &ib->second.data};
        return true;
    }

    // rows [co0, co0 + n) of a weight / bias of shape l: one launch per group of output channels (UPNet.2, the dec3 phases)
    SubW rows(const Layer& l, const std::vector<float>* w, const std::vector<float>* b, int co0, int n) const
    {
        SubW o;
        o.shape = {n, l.cin, l.kh, l.kw};
        if (dry) return o;
        const size_t row = (size_t)l.cin * l.kh * l.kw;
        o.w.assign(w->begin() + co0 * row, w->begin() + (co0 + n) * row);
        o.b.assign(b->begin() + co0, b->begin() + co0 + n);
        return o;
    }
    SubW sub_weight_cout(const std::string& name, int co0, int n)
    {
        Found f;
        return lookup(name, f) ? rows(f.l, f.w, f.b, co0, n) : SubW();
    }
    // the original input channels `sel` (in that order) of a layer
    SubW sub_weight(const std::string& name, const std::vector<int32_t>& sel, bool with_bias)
    {
        SubW o;
        Found f;
        if (!lookup(name, f)) return o;
        const Layer& l = f.l;
        o.shape = {l.cout, (int)sel.size(), l.kh, l.kw};
        if (dry) return o;
        const int taps = l.kh * l.kw;
        o.w.resize((size_t)l.cout * sel.size() * taps);
        for (int co = 0; co < l.cout; ++co)
            for (size_t k = 0; k < sel.size(); ++k)
                memcpy(&o.w[((size_t)co * sel.size() + k) * taps], &(*f.w)[((size_t)co * l.cin + sel[k]) * taps], taps * sizeof(float));
        o.b.assign(l.cout, 0.0f);
        if (with_bias) o.b = *f.b;
        return o;
    }
    // the output-channel rows of several layers over one input, one after the other (z | r of a GRU step as one 128-cout layer)
    SubW concat_cout(const std::vector<std::string>& names)
    {
        SubW o;
        o.shape = {0, 0, 0, 0};
        for (const std::string& n : names) {
            Found f;
            if (!lookup(n, f)) return o;
            o.shape = {o.shape.cout + f.l.cout, f.l.cin, f.l.kh, f.l.kw};
            if (dry) continue;
            o.w.insert(o.w.end(), f.w->begin(), f.w->end());
            o.b.insert(o.b.end(), f.b->begin(), f.b->end());
        }
        return o;
    }

    void conv(OpList& seg, const std::string& name, const std::vector<Src>& srcs, const std::vector<Dst>& dsts, int H, int W,
              const ConvOpt& o = ConvOpt())
    {
        if (status < 0) return;
        Found f;
        if (o.sub) f = {o.sub->shape, &o.sub->w, &o.sub->b};
        else if (!lookup(name, f)) return;
        std::vector<demfi_conv_src> cs(srcs.size());
        for (size_t i = 0; i < srcs.size(); ++i) cs[i] = {srcs[i].v, srcs[i].fat, srcs[i].up, (int32_t)srcs[i].cin.size(), 0, srcs[i].cin.data()};
        std::vector<demfi_conv_dst> cd(dsts.size());
        for (size_t i = 0; i < dsts.size(); ++i)
            cd[i] = {dsts[i].dst, dsts[i].res, dsts[i].aux, dsts[i].act, dsts[i].mode, dsts[i].scale, dsts[i].dy, dsts[i].dx,
                     (int32_t)dsts[i].couts.size(), dsts[i].couts.data()};
        demfi_view pack_v = o.pack;
        int batch = o.batch;
        if (tb > 1) {
            if (!tb_view(pack_v, batch, name.c_str())) return;
            for (auto& x : cs) if (!tb_view(x.v, batch, name.c_str())) return;
            for (auto& x : cd) if (!tb_view(x.dst, batch, name.c_str()) || !tb_view(x.res, batch, name.c_str()) || !tb_view(x.aux, batch, name.c_str())) return;
            batch *= tb;
        }
        pack_v._pad = 0;                                         // the tensor ids are the builder's business, not the descriptors'
        for (auto& x : cs) x.v._pad = 0;
        for (auto& x : cd) x.dst._pad = x.res._pad = x.aux._pad = 0;
        ConvShape sh;
        status = conv_shape(c->dtype, H, W, o.stride, batch, f.l, cs.data(), (int)cs.size(), cd.data(), (int)cd.size(), sh, name.c_str(),
                            o.pad_y, o.pad_x, tb);
        if (status < 0) return;
        // the packed blob of a call site depends on its channel maps only (not on buffer addresses): per-t contexts and
        // the two FGAC directions share one copy
        std::string sig = name + "|";
        for (auto& s : srcs) { sig += s.fat ? 'F' : 'T'; for (int32_t ch : s.cin) sig += std::to_string(ch) + ","; sig += ';'; }
        sig += "|";
        for (auto& d : dsts) { for (int32_t ch : d.couts) sig += std::to_string(ch) + ","; sig += ';'; }
        // which kernel owns the layer decides the packed cout order; the record size / cout blocking (they depend on the grid,
        // i.e. on the batch: the batched plan may choose differently) decide the chunk order of the blob
        sig += sh.d.cout_perm ? "|P" : "|N";
        sig += "|r" + std::to_string(sh.d.rec_bytes) + "n" + std::to_string(sh.d.nco);
        auto hit = c->pack_cache.find(sig);
        int64_t w_off, b_off;
        if (hit != c->pack_cache.end()) { w_off = hit->second.first; b_off = hit->second.second; }
        else {
            std::vector<uint8_t> wp;
            std::vector<float> bp;
            if (!dry) status = conv_pack(sh, f.l, f.w->data(), f.b->data(), wp, bp);
            if (status < 0) return;
            w_off = blob_put(wp.data(), sh.wbytes);
            b_off = blob_put(bp.data(), (int64_t)sh.d.cout_pad * 4);
            if (status < 0) return;
            c->pack_cache[sig] = {w_off, b_off};
        }
        sh.d.wpack = c->base + c->w_region + w_off;
        sh.d.bias = (const float*)(c->base + c->w_region + b_off);
        sh.d.zero_page = c->base + c->zero_off;
        sh.d.u8_sink = o.sink;
        sh.d.u8_iter = o.sink_iter;
        sh.d.pack = pack_v;
        // The plan's bytes stay what they have always been: a descriptor without a sink / a packed copy repeats the u8_iter / the view
        // strides of the descriptor before it.  Nothing reads either without its pointer (conv_narrow.hip); it keeps the plan digest
        // (tools/plan_digest.py) equal to that of the builder this one replaced.
        if (!c->descs.empty()) {
            const demfi_conv& prev = c->descs.back();
            if (!o.sink) sh.d.u8_iter = prev.u8_iter;
            if (!pack_v.ptr) { sh.d.pack = prev.pack; sh.d.pack.ptr = nullptr; }
        }
        for (int g = 0; g < 4; ++g) sh.d.pack_oct_ch[g] = pack_v.ptr ? o.pack_ch[g] : -1;
        c->descs.push_back(sh.d);
        demfi_op op = blank();
        op.kind = DEMFI_OP_CONV;
        op.conv = (int)c->descs.size() - 1;
        op.macs = sh.macs;
        strncpy(op.name, name.c_str(), sizeof(op.name) - 1);
        seg.push_back(op);
    }

    void simple(OpList& seg, int kind, const char* name, demfi_op op)
    {
        op.kind = kind;
        strncpy(op.name, name, sizeof(op.name) - 1);
        const int64_t cs_a = op.a.ptr ? view_stride(op.a) : -1, cs_b = op.b.ptr ? view_stride(op.b) : -1, cs_o = op.o.ptr ? view_stride(op.o) : -1;
        op.a._pad = op.b._pad = op.o._pad = 0;
        if (tb <= 1) { seg.push_back(op); return; }
        // batched plan.  CFR and the thin (3-channel) warps: ONE launch for all tb per-t contexts (ABI v5, demfi_batch): the pointers
        // are those of context 0, every pointer gets the byte stride of the buffer it lies in (per-t buffers: their context stride;
        // window-level buffers of the trunk set: 0).  Measured in sequence at 720p x 7 contexts (profiles/r03_notes.md): cfr 81 -> 67 us
        // and warp_thin 37 -> 35 us per time instant.  The fat warp and the plane packs stay one launch per context: batched they
        // were SLOWER (pack 23 -> 31 us per context; fat warp with the contexts innermost per tile 85 -> 73 / 90 us: the gathered
        // neighbourhoods of a tile do not survive in the 4 MB L2 across seven time instants with these incoherent flows).
        // Round 5: the fat warps too, as ONE launch with one grid slice per context (demfi_batch._pad = 1): the same tiles in the same
        // order as tb launches, without their launch gaps and tails (a launch is ~80 us).  The plane packs too, grid.y = context
        // (22 -> 4 launches per window: -0.1 ms)
        if (kind == DEMFI_OP_CFR || kind == DEMFI_OP_WARP || kind == DEMFI_OP_PACK) {
            op.bt._pad = kind == DEMFI_OP_WARP && op.nch != 3 ? 1 : 0;
            auto stride = [&](const void* p) { const int64_t cs = ctx_stride_of(p); return cs > 0 ? cs : (int64_t)0; };
            op.bt.nb = tb;
            op.bt.a = cs_a > 0 ? cs_a : 0; op.bt.b = cs_b > 0 ? cs_b : 0; op.bt.o = cs_o > 0 ? cs_o : 0; op.bt.t = stride(op.t);
            for (int i = 0; i < 32; ++i) op.bt.p[i] = stride(op.p[i]);
            seg.push_back(op);
            return;
        }
        for (int q = 0; q < tb; ++q) {                          // one launch per context, pointers rebased
            demfi_op o = op;
            if (op.a.ptr && cs_a > 0) o.a.ptr = (char*)op.a.ptr + q * cs_a;
            if (op.b.ptr && cs_b > 0) o.b.ptr = (char*)op.b.ptr + q * cs_b;
            if (op.o.ptr && cs_o > 0) o.o.ptr = (char*)op.o.ptr + q * cs_o;
            for (int i = 0; i < 32; ++i) o.p[i] = tb_ptr(op.p[i], q);
            o.t = tb_ptr(op.t, q);
            seg.push_back(o);
        }
    }
    static demfi_op blank() { demfi_op o; memset(&o, 0, sizeof(o)); return o; }

    void pack(OpList& seg, const std::vector<const float*>& planes, const Tensor& dst)
    {
        demfi_op op = blank();
        op.nch = dst.d[3];
        for (int i = 0; i < 32; ++i) op.p[i] = i < (int)planes.size() ? planes[i] : nullptr;
        op.o = fview(dst);
        simple(seg, DEMFI_OP_PACK, "pack", op);
    }

    // Round 5: the two launches conv() has just appended (conv1 -> ReLU -> t, conv2 + identity) become ONE launch of the fused
    // residual-block kernel when the pair qualifies (fp16 plan, 3x3 64 -> 64, persistent-kernel packing): the intermediate stays in
    // LDS, the scratch buffer t is not touched -- and under the workspace arena it has NO memory (its views point at the arena's first
    // bytes, which belong to a live tenant): a RESBLOCK op must never be executed as its two convolutions on the bound workspace.  Both
    // descriptors are kept as they are for the CPU plan interpreter (which gives the intermediate private memory, tests/plan_sim.py).
    void fuse_resblock(OpList& seg, const std::string& name)
    {
        if (status < 0 || seg.size() < 2) return;
        const demfi_op o2 = seg[seg.size() - 1], o1 = seg[seg.size() - 2];
        if (o1.kind != DEMFI_OP_CONV || o2.kind != DEMFI_OP_CONV) return;
        demfi_conv h1 = c->descs[o1.conv], h2 = c->descs[o2.conv];
        if (dry) {                                               // sizing pass: the blobs are not placed yet
            static const char some = 0;
            h1.wpack = h2.wpack = h1.zero_page = h2.zero_page = &some;
            h1.bias = h2.bias = (const float*)&some;
        }
        if (!demfi_resblock_eligible(&h1, &h2)) return;
        demfi_op op = blank();
        op.kind = DEMFI_OP_RESBLOCK;
        op.conv = o1.conv;
        op.nch = o2.conv;
        op.macs = o1.macs + o2.macs;
        strncpy(op.name, name.c_str(), sizeof(op.name) - 1);
        seg.pop_back();
        seg.pop_back();
        seg.push_back(op);
        c->fused_now.push_back("resblock:" + name);
    }

    // Round 6: one SepConvGRU half-step (DeMFInet.py:844-849 / 851-856).  conv() has just appended the three plain 64-cout layers
    //     convr: [h, x] -> r*h (MUL)     convz: [h, x] -> z (sigmoid, into the z buffer)     convq: [r*h, x] -> h' (GRU epilogue, aux = z)
    // The first becomes a launch of the round-6 kernel's R mode, the other two ONE launch of its ZQ mode (gru.hip: z stays on chip, the z
    // buffer is never touched) when they qualify (fp16 plan).  The descriptors stay as they are: the CPU plan interpreter runs the
    // three layers through demfi_conv2d (the round-5 kernel at 64 couts).
    void fuse_gru(OpList& seg, const std::string& name)
    {
        if (status < 0 || seg.size() < 3) return;
        const demfi_op oq = seg[seg.size() - 1], oz = seg[seg.size() - 2], orr = seg[seg.size() - 3];
        if (oq.kind != DEMFI_OP_CONV || oz.kind != DEMFI_OP_CONV || orr.kind != DEMFI_OP_CONV) return;
        demfi_conv hq = c->descs[oq.conv], hz = c->descs[oz.conv], hr = c->descs[orr.conv];
        if (dry) {                                               // sizing pass: the blobs are not placed yet
            static const char some = 0;
            for (demfi_conv* h : {&hq, &hz, &hr}) { h->wpack = h->zero_page = &some; h->bias = (const float*)&some; }
        }
        if (!demfi_gru_r_eligible(&hr) || !demfi_gru_zq_eligible(&hz, &hq)) return;
        demfi_op r = orr, zq = blank();
        r.kind = DEMFI_OP_GRU_R;
        zq.kind = DEMFI_OP_GRU_ZQ;
        zq.conv = oz.conv;
        zq.nch = oq.conv;
        zq.macs = oz.macs + oq.macs;
        strncpy(zq.name, (name + ".convzq").c_str(), sizeof(zq.name) - 1);
        seg.pop_back(); seg.pop_back(); seg.pop_back();
        seg.push_back(r);
        seg.push_back(zq);
        c->fused_now.push_back("gru:" + name);
    }

    // x_{k+1} = x_k + conv2(relu(conv1(x_k))) ping-ponging between buffers a and b (t = scratch); returns the result buffer
    const Tensor* resblocks(OpList& seg, const std::string& prefix, int n, const Tensor& a, const Tensor& t, const Tensor& b,
                            int H, int W, int batch)
    {
        const Tensor *cur = &a, *other = &b;
        for (int i = 0; i < n; ++i) {
            const std::string p = prefix + "." + std::to_string(i);
            conv(seg, p + ".conv1", {fsrc(*cur, 0)}, {D(fview(t), range(0, 64), DEMFI_ACT_RELU)}, H, W, ConvOpt().batched(batch));
            conv(seg, p + ".conv2", {fsrc(t, 0)}, {D(fview(*other), range(0, 64), DEMFI_ACT_NONE, DEMFI_MODE_STORE, fview(*cur))},
                 H, W, ConvOpt().batched(batch));
            fuse_resblock(seg, p);
            std::swap(cur, other);
        }
        return cur;
    }

    // ---- single-call operators: the launch sequences demfi_amd/ops.py composes, behind the C ABI --------------------
    void build_operator()
    {
        BufSet& B = c->tr_bufs[0];
        OpList& tr = c->tr_ops[0];
        const int H = c->H, W = c->W, nb = c->op_batch;
        const int R = DEMFI_ACT_RELU, S = DEMFI_ACT_SIGMOID;
        if (c->op_kind == 1) {
            // SepConvGRU.forward (DeMFInet.py:838-857): horizontal then vertical GRU step; z | r as one 128-cout convolution
            // (sigmoid; sigmoid * h), q with the GRU blend (1 - z) h + z tanh(.) in its epilogue
            const Tensor* h = &B["h"];
            for (int s2 = 0; s2 < 2 && status >= 0; ++s2) {
                const std::string sfx = std::to_string(s2 + 1);
                const Tensor& hnext = s2 == 0 ? B["h1"] : B["out"];
                if (c->dtype == DEMFI_F16) {         // round 6: r*h, then z + q + blend in one launch (fuse_gru)
                    conv(tr, "convr" + sfx, {fsrc(*h, 0), fsrc(B["x"], 64)}, {D(fview(B["rh"]), range(0, 64), DEMFI_ACT_NONE, DEMFI_MODE_MUL, fview(*h))}, H, W, ConvOpt().batched(nb));
                    conv(tr, "convz" + sfx, {fsrc(*h, 0), fsrc(B["x"], 64)}, {D(fview(B["z"]), range(0, 64), S)}, H, W, ConvOpt().batched(nb));
                    conv(tr, "convq" + sfx, {fsrc(B["rh"], 0), fsrc(B["x"], 64)},
                         {D(fview(hnext), range(0, 64), DEMFI_ACT_NONE, DEMFI_MODE_GRU, fview(*h), fview(B["z"]))}, H, W, ConvOpt().batched(nb));
                    fuse_gru(tr, "step" + sfx);
                    h = &hnext;
                    continue;
                }
                const SubW zr = concat_cout({"convz" + sfx, "convr" + sfx});
                conv(tr, "convzr" + sfx, {fsrc(*h, 0), fsrc(B["x"], 64)},
                     {D(fview(B["z"]), range(0, 64), S), D(fview(B["rh"]), range(64, 128), DEMFI_ACT_NONE, DEMFI_MODE_MUL, fview(*h))}, H, W,
                     ConvOpt().batched(nb).weights(zr));
                conv(tr, "convq" + sfx, {fsrc(B["rh"], 0), fsrc(B["x"], 64)},
                     {D(fview(hnext), range(0, 64), DEMFI_ACT_NONE, DEMFI_MODE_GRU, fview(*h), fview(B["z"]))}, H, W, ConvOpt().batched(nb));
                h = &hnext;
            }
            return;
        }
        // FGAC.forward at rr = sr = 0 (DeMFInet.py:386-452): conv_ref_k -> bilinear sample at the absolute flow coordinates -> fusion ->
        // w = sigmoid(w_gen_2(relu(w_gen(cat[source, E_s])))) -> w source + (1 - w) E_s
        const int64_t hw4 = (int64_t)H * W * 4;
        conv(tr, "conv_ref_k", {fsrc(B["ref"], 0)}, {D(fview(B["ref_k"]), range(0, 64))}, H, W, ConvOpt().batched(nb));
        for (int b = 0; b < nb; ++b) {
            demfi_op o = blank();
            o.nch = 64;
            o.a = fview(B["ref_k"], 0, b); o.o = fview(B["sampled"], 0, b);
            o.p[0] = ptr(B["flow"]) + 2 * b * hw4;
            simple(tr, DEMFI_OP_FGAC, "fgac", o);
        }
        conv(tr, "fusion", {fsrc(B["sampled"], 0)}, {D(fview(B["e_s"]), range(0, 64))}, H, W, ConvOpt().batched(nb));
        conv(tr, "w_gen", {fsrc(B["source"], 0), fsrc(B["e_s"], 64)}, {D(fview(B["hid"]), range(0, 64), R)}, H, W, ConvOpt().batched(nb));
        conv(tr, "w_gen_2", {fsrc(B["hid"], 0)}, {D(tview(B["w"], 0, (int64_t)H * W), {0}, S)}, H, W, ConvOpt().batched(nb));
        for (int b = 0; b < nb; ++b) {
            demfi_op o = blank();
            o.nch = 64;
            o.a = fview(B["source"], 0, b); o.b = fview(B["e_s"], 0, b); o.o = fview(B["out"], 0, b);
            o.p[0] = ptr(B["w"]) + b * hw4;
            simple(tr, DEMFI_OP_GATE, "gate", o);
        }
    }

    void build_trunk(int k)
    {
        BufSet& B = c->tr_bufs[k];
        OpList& tr = c->tr_ops[k];
        const int H = c->H, W = c->W, H2 = H / 2, W2 = W / 2;
        const int R = DEMFI_ACT_RELU, T = DEMFI_ACT_TANH, S = DEMFI_ACT_SIGMOID;
        const int64_t hw4 = (int64_t)H * W * 4;
        // ============================ trunk: FF_RDB (DeMFInet.py:233-253) ==========================================
        std::string p = "FF_RDB_Module.";
        { demfi_op o = blank(); o.p[0] = ptr(B["x"]); o.p[1] = ptr(B["s2d"]); simple(tr, DEMFI_OP_S2D, "s2d", o); }
        { demfi_op o = blank(); o.p[0] = ptr(B["x"]); o.p[1] = ptr(B["overlay"]); simple(tr, DEMFI_OP_OVERLAY, "overlay", o); }
        conv(tr, p + "SFENet1", {fsrc(B["s2d"], 0)}, {D(fview(B["f1"]), range(0, 96))}, H2, W2);
        conv(tr, p + "SFENet2", {fsrc(B["f1"], 0)}, {D(fview(B["x0"]), range(0, 96))}, H2, W2);
        for (int i = 0; i < 12; ++i) {
            auto xin = [&]() { return i == 0 ? fsrc(B["x0"], 0) : fsrc(B["gffcat"], 0, 96 * (i - 1), 96); };
            const demfi_view xres = i == 0 ? fview(B["x0"]) : fview(B["gffcat"], 96 * (i - 1));
            const std::string rp = p + "RDBs." + std::to_string(i);
            for (int q = 0; q < 4; ++q) {
                std::vector<Src> s{xin()};
                if (q) s.push_back(fsrc(B["grow"], 96, 0, 32 * q));
                conv(tr, rp + ".convs." + std::to_string(q) + ".conv.0", s, {D(fview(B["grow"], 32 * q), range(0, 32), R)}, H2, W2);
            }
            conv(tr, rp + ".LFF", {xin(), fsrc(B["grow"], 96, 0, 128)},
                 {D(fview(B["gffcat"], 96 * i), range(0, 96), DEMFI_ACT_NONE, DEMFI_MODE_STORE, xres)}, H2, W2);
        }
        conv(tr, p + "GFF.0", {fsrc(B["gffcat"], 0)}, {D(fview(B["g0"]), range(0, 96))}, H2, W2);
        conv(tr, p + "GFF.1", {fsrc(B["g0"], 0)}, {D(fview(B["g1"]), range(0, 96), DEMFI_ACT_NONE, DEMFI_MODE_STORE, fview(B["f1"]))}, H2, W2);
        // UPNet.0 + PixelShuffle(2): out[c, 2h+i, 2w+j] = conv[c*4 + i*2 + j, h, w]
        {
            std::vector<Dst> ds;
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    std::vector<int32_t> co;
                    for (int ch = 0; ch < 64; ++ch) co.push_back(ch * 4 + i * 2 + j);
                    ds.push_back(D(fview(B["up"]), co, DEMFI_ACT_NONE, DEMFI_MODE_STORE, NOVIEW, NOVIEW, 2, i, j));
                }
            conv(tr, p + "UPNet.0", {fsrc(B["g1"], 0)}, ds, H2, W2);
        }
        // UPNet.2 (3x3, 64 -> 133 = F0 | F1 | flow_01, flow_10, occlusion logit; DeMFInet.py:231, 247-253).  Round 6, fp16 plan: one launch per
        // output group -- the two tanh feature halves on the staged-store 64 -> 64 kernel, the 5 planes on the thin-output kernel -- instead
        // of ONE 160-cout launch of the general kernel (0.32 ms at 0.18 of the matrix peak).
        if (c->dtype == DEMFI_F16) {
            SubW w0 = sub_weight_cout(p + "UPNet.2", 0, 64), w1 = sub_weight_cout(p + "UPNet.2", 64, 64), w2 = sub_weight_cout(p + "UPNet.2", 128, 5);
            conv(tr, p + "UPNet.2#F0", {fsrc(B["up"], 0)}, {D(fview(B["F01"], 0, 0), range(0, 64), T)}, H, W, ConvOpt().weights(w0));
            conv(tr, p + "UPNet.2#F1", {fsrc(B["up"], 0)}, {D(fview(B["F01"], 0, 1), range(0, 64), T)}, H, W, ConvOpt().weights(w1));
            conv(tr, p + "UPNet.2#f", {fsrc(B["up"], 0)}, {D(tview(B["ffo"]), range(0, 5))}, H, W, ConvOpt().weights(w2));
        } else
        conv(tr, p + "UPNet.2", {fsrc(B["up"], 0)},
             {D(fview(B["F01"], 0, 0), range(0, 64), T), D(fview(B["F01"], 0, 1), range(64, 128), T), D(tview(B["ffo"]), range(128, 133))}, H, W);
        // ============================ trunk: FAC-FB (DeMFInet.py:335-358, 386-452) ================================
        p = "FAC_FB_Module.";
        conv(tr, p + "conv_first", {fsrc(B["F01"], 0)}, {D(fview(B["enc_a"]), range(0, 64), R)}, H, W, ConvOpt().batched(2));
        const Tensor* enc = resblocks(tr, p + "feature_extraction", c->hp.num_resb_facfb, B["enc_a"], B["enc_t"], B["enc_b"], H, W, 2);
        B["enc"] = *enc;                                             // alias: the buffer holding the encoder output
        for (int b = 0; b < 2; ++b) {          // b = 0: F1 -> F0 with flow_01 ; b = 1: F0 -> F1 with flow_10 (346-349)
            const std::string fg = p + (c->hp.shared_fgac ? "shared_FGAC" : (b == 0 ? "FGAC_F1toF0" : "FGAC_F0toF1"));
            const int ref = 1 - b, src = b;
            conv(tr, fg + ".conv_ref_k", {fsrc(*enc, 0, 0, -1, ref)}, {D(fview(B["rk"], 0, b), range(0, 64))}, H, W);
            if (c->hp.fgac_rr > 0) {
                // generalised FGAC (DeMFInet.py:401-445): conv_source_k is live, optional PxP average pooling of both key
                // maps, then the window kernel (correlation, softmax, weighted sum)
                conv(tr, fg + ".conv_source_k", {fsrc(*enc, 0, 0, -1, src)}, {D(fview(B["skk"], 0, b), range(0, 64))}, H, W);
                const char *rkn = "rk", *skn = "skk";
                if (c->hp.fgac_sr > 0) {
                    for (int q = 0; q < 2; ++q) {
                        demfi_op o = blank();
                        o.nch = 64; o.conv = c->hp.fgac_sr;
                        o.a = fview(B[q ? "skk" : "rk"], 0, b); o.o = fview(B[q ? "skp" : "rkp"], 0, b);
                        simple(tr, DEMFI_OP_AVG_POOL, "avg_pool", o);
                    }
                    rkn = "rkp"; skn = "skp";
                }
                demfi_op o = blank();
                o.nch = 64; o.conv = c->hp.fgac_rr; o._pad = c->hp.flags & DEMFI_HP_FGAC_CENTRED;
                o.a = fview(B[rkn], 0, b); o.b = fview(B[skn], 0, b); o.o = fview(B["smp"], 0, b);
                o.p[0] = ptr(B["ffo"]) + (b == 0 ? 0 : 2) * hw4;
                simple(tr, DEMFI_OP_FGAC_WINDOW, "fgac_window", o);
            } else {
                demfi_op o = blank();
                o.nch = 64;
                o.a = fview(B["rk"], 0, b); o.o = fview(B["smp"], 0, b);
                o.p[0] = ptr(B["ffo"]) + (b == 0 ? 0 : 2) * hw4;
                simple(tr, DEMFI_OP_FGAC, "fgac", o);
            }
            conv(tr, fg + ".fusion", {fsrc(B["smp"], 0, 0, -1, b)}, {D(fview(B["E"], 0, b), range(0, 64))}, H, W);
            conv(tr, fg + ".w_gen", {fsrc(*enc, 0, 0, -1, src), fsrc(B["E"], 64, 0, -1, b)}, {D(fview(B["wg"], 0, b), range(0, 64), R)}, H, W);
            conv(tr, fg + ".w_gen_2", {fsrc(B["wg"], 0, 0, -1, b)}, {D(tview(B["gate"], b), {0}, S)}, H, W);
            {
                demfi_op o = blank();
                o.nch = 64;
                o.a = fview(*enc, 0, b); o.b = fview(B["E"], 0, b); o.o = fview(B["aF"], 0, b);
                o.p[0] = ptr(B["gate"]) + b * hw4;
                simple(tr, DEMFI_OP_GATE, "gate", o);
            }
            if (c->hp.flags & DEMFI_HP_EXTRAS) {
                // the maps FGAC.forward returns besides its output (DeMFInet.py:454-496): diff (always computed by the reference, returned
                // in the training / visualisation tuples of DeMFInet.forward 167-176) and the four visualisation maps + (1 - w_sr)
                auto vz = [&](int k) { return ptr(B["viz"]) + (6 * b + k) * hw4; };
                auto absmean = [&](int k, demfi_view a, demfi_view bb) {
                    demfi_op o = blank();
                    o.conv = 0; o.nch = 64; o.a = a; o.b = bb; o.p[0] = vz(k);
                    simple(tr, DEMFI_OP_VIZ, "viz_absmean", o);
                    demfi_op n = blank();
                    n.conv = 1; n.p[0] = vz(k); n.p[1] = ptr(B["vizs"]);
                    simple(tr, DEMFI_OP_VIZ, "viz_normalize", n);
                };
                { demfi_op o = blank(); o.conv = 2; o.p[0] = vz(0); o.p[1] = ptr(B["gate"]) + b * hw4; simple(tr, DEMFI_OP_VIZ, "viz_one_minus", o); }
                absmean(1, fview(*enc, 0, src), NOVIEW);                    // source_v
                absmean(2, fview(B["rk"], 0, b), NOVIEW);                   // init_ref_k = conv_ref_k(ref)
                absmean(3, fview(B["E"], 0, b), NOVIEW);                    // E_s
                absmean(4, fview(B["aF"], 0, b), NOVIEW);                   // bolstered_F_s
                absmean(5, fview(B["aF"], 0, b), fview(*enc, 0, src));      // diff = bolstered_F_s - source_v
            }
        }
        if (c->dtype == DEMFI_F16) {
            // Refine_Module.enc1 = conv4x4s2(cat[aF0, aF1 | Ft, flows ...]) (DeMFInet.py:77, 588): the aF0 | aF1 half (128 of
            // 201 input channels, 64 % of the layer) does not depend on t -> computed once per window, added as a residual
            SubW wa = sub_weight("Refine_Module.enc1", range(0, 128), true);
            conv(tr, "Refine_Module.enc1#aF", {fsrc(B["aF"], 0, 0, -1, 0), fsrc(B["aF"], 64, 0, -1, 1)},
                 {D(fview(B["u1a"]), range(0, 64))}, H2, W2, ConvOpt().strided(2).weights(wa));
            // Mixer.conv_ref1 (7x7 over 30 planes) and Dec_first_2 read the 4 input frames and flow_10 | flow_01: 16 planes that do
            // not change within a window.  Packed once (xff16) and their share of both layers computed once per window; the
            // per-t parts then fit the narrow persistent kernels (16-channel records) and take these as residuals.
            std::vector<const float*> pl;
            for (int f = 0; f < 4; ++f)
                for (int col = 0; col < 3; ++col) pl.push_back(plane(B["x"], col * 4 + f));
            for (int i : {2, 3, 0, 1}) pl.push_back(plane(B["ffo"], i));
            pack(tr, pl, B["xff16"]);
            SubW w1 = sub_weight("Booster_Module.Mixer.conv_ref1", range(9, 25), false);
            conv(tr, "Booster_Module.Mixer.conv_ref1#win", {fsrc_map(B["xff16"], range(0, 16))}, {D(fview(B["re1w"]), range(0, 32))}, H, W, ConvOpt().weights(w1));
            std::vector<int32_t> sel = range(87, 99);                    // frames, then flow_10 | flow_01 (Agg3 order, DeMFInet.py:151-155)
            for (int i = 78; i < 82; ++i) sel.push_back(i);
            SubW w2 = sub_weight("Dec_first_2", sel, false);
            conv(tr, "Dec_first_2#win", {fsrc_map(B["xff16"], range(0, 16))}, {D(fview(B["g_pw"]), range(0, 64))}, H, W, ConvOpt().weights(w2));
        }
    }

    void warp(OpList& seg, const char* name, int C, demfi_view A, demfi_view Bv, demfi_view O, const void* fa, const void* fb,
              const void* logit, const void* occ_out, const void* t, const void* pack8 = nullptr)
    {
        demfi_op o = blank();
        o.nch = C; o.a = A; o.b = Bv; o.o = O;
        o.p[0] = fa; o.p[1] = fb; o.p[2] = logit; o.p[3] = occ_out; o.p[4] = pack8; o.t = t;
        simple(seg, DEMFI_OP_WARP, name, o);
    }

    void build_t(int k, int q)
    {
        BufSet& TB = c->tr_bufs[k];
        BufSet& B = c->t_bufs[k][q];
        OpList& th = tb > 1 ? c->tb_head_ops[k] : c->head_ops[k][q];
        const int H = c->H, W = c->W, N = c->N;
        const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
        const int R = DEMFI_ACT_RELU, T = DEMFI_ACT_TANH;
        const int64_t hw4 = (int64_t)H * W * 4;
        const Tensor& ffo = TB["ffo"];
        const Tensor& aF = TB["aF"];
        const Tensor& x = TB["x"];
        const void* tp = ptr(B["t"]);
        auto delta_v = [&](int step, int ch) { return tview(B["delta"], 5 * step + ch); };
        auto delta_p = [&](int step, int ch) { return plane(B["delta"], 5 * step + ch); };
        // ============================ per-t head: CFR, FWB, refinement, D1, Ch_Reducer ==============================
        {
            demfi_op o = blank();
            o.p[0] = ptr(ffo); o.p[1] = ptr(ffo) + 2 * hw4; o.p[2] = ptr(B["cfr_acc"]); o.p[3] = ptr(B["ft"]); o.t = tp;
            // round 6: the finish also writes misc16 = [flow_t0, flow_t1 | flow_01, flow_10, occ logit | 0] (the thin members of Agg1, 77) as the
            // NHWC record enc1 stages: one plane-pack launch per window less
            o.p[4] = ptr(ffo) + 4 * hw4; o.p[5] = ptr(B["misc16"]);
            simple(th, DEMFI_OP_CFR, "cfr", o);
        }
        warp(th, "warp_fat", 64, fview(TB["F01"], 0, 0), fview(TB["F01"], 0, 1), fview(B["Ft"], 0, 0), ptr(B["ft"]), ptr(B["ft"]) + 2 * hw4,
             ptr(ffo) + 4 * hw4, nullptr, tp);
        std::string p = "Refine_Module.";
        // Agg1 = cat[aF0, aF1, Ft, flow_t0, flow_t1, flow_01, flow_10, occ_0_logit] (DeMFInet.py:77)
        {
            std::vector<int32_t> m = range(192, 201);
            m.insert(m.end(), 7, -1);
            if (c->dtype == DEMFI_F16) {
                // the t-dependent 73 channels only; + the hoisted aF part (trunk) as residual, then ReLU
                std::vector<int32_t> sel = range(128, 201), m2 = range(64, 73);
                m2.insert(m2.end(), 7, -1);
                SubW wb = sub_weight(p + "enc1", sel, false);
                conv(th, p + "enc1#t", {fsrc(B["Ft"], 0), fsrc_map(B["misc16"], m2)},
                     {D(fview(B["u1"]), range(0, 64), R, DEMFI_MODE_STORE, fview(TB["u1a"]))}, H2, W2, ConvOpt().strided(2).weights(wb));
            } else
            conv(th, p + "enc1", {fsrc(aF, 0, 0, -1, 0), fsrc(aF, 64, 0, -1, 1), fsrc(B["Ft"], 128), fsrc_map(B["misc16"], m)},
                 {D(fview(B["u1"]), range(0, 64), R)}, H2, W2, ConvOpt().strided(2));
        }
        conv(th, p + "enc2", {fsrc(B["u1"], 0)}, {D(fview(B["u2"]), range(0, 128), R)}, H4, W4, ConvOpt().strided(2));
        conv(th, p + "enc3", {fsrc(B["u2"], 0)}, {D(fview(B["u3"]), range(0, 256), R)}, H8, W8, ConvOpt().strided(2));
        conv(th, p + "dec0", {fsrc(B["u3"], 0)}, {D(fview(B["d0"]), range(0, 256), R)}, H8, W8);
        conv(th, p + "dec1", {fsrc(B["d0"], 0, 0, -1, -1, 1), fsrc(B["u2"], 256)}, {D(fview(B["d1"]), range(0, 128), R)}, H4, W4);
        conv(th, p + "dec2", {fsrc(B["d1"], 0, 0, -1, -1, 1), fsrc(B["u1"], 128)}, {D(fview(B["d2"]), range(0, 64), R)}, H2, W2);
        // + cat[flow_t0, flow_t1, occ_0_logit, aF0, aF1] (78-80), tanh on the feature part (86-87)
        if (c->dtype == DEMFI_F16) {
            // dec3 = conv3x3(NN-upsample x2 (d2)) (DeMFInet.py:600-602).  A 3x3 filter over a 2x nearest-neighbour upsampled image
            // reads, for the output pixels of parity (dy, dx), only 2x2 DISTINCT low-resolution pixels: rows {y-1, y} with weights
            // {W[0], W[1]+W[2]} for dy = 0, rows {y, y+1} with {W[0]+W[1], W[2]} for dy = 1 (columns alike).  Four 2x2 convolutions
            // on the half-resolution grid, each writing its parity of the full-resolution outputs (views with doubled strides),
            // do 4 taps per output instead of 9: 2.25x fewer MACs, no upsampled gather.
            Found f3;
            if (!lookup(p + "dec3", f3)) return;
            const Layer l3 = f3.l;
            auto phase_view = [&](demfi_view v, int dy, int dx) {           // pixels (2y+dy, 2x+dx) of a full-resolution view
                const int64_t elt = v.is_f32 ? 4 : 2;
                v.ptr = (char*)v.ptr + ((int64_t)dy * v.sy + (int64_t)dx * v.sx) * elt;
                v.sx *= 2; v.sy *= 2;
                return v;
            };
            // Round 3: each parity runs as THREE launches of the fast 64-input-channel kernels instead of one 160-cout launch of the
            // general kernel (0.50 ms per parity at 0.09 of the MFMA peak): the 2x2 filter is embedded in a 3x3 one (taps outside the
            // 2x2 footprint are zero: the 2.25x MAC saving is given back, the layer is memory-bound either way), so that the two
            // 64-channel feature halves (tanh + residual aF0 / aF1) go to the staged-store 64 -> 64 kernel and the 5 flow / occlusion
            // planes to a 32-cout launch.
            // round 6: the flow / occlusion planes of the two column parities of a row parity in ONE launch (10 couts = 4 live octets of a
            // 32-cout subtile that the per-parity launches filled with 5): 4 -> 2 launches of the thin kernel
            for (int dy = 0; dy < 2 && status >= 0; ++dy) {
                SubW wf2;
                wf2.shape = {10, l3.cin, 3, 3};
                for (int dx = 0; dx < 2 && status >= 0; ++dx) {
                    std::vector<float> w9e;
                    if (!dry) {
                        w9e.assign((size_t)l3.cout * l3.cin * 9, 0.0f);
                        for (int co = 0; co < l3.cout; ++co)
                            for (int ci = 0; ci < l3.cin; ++ci) {
                                const float* w9 = &(*f3.w)[((size_t)co * l3.cin + ci) * 9];
                                float* we = &w9e[((size_t)co * l3.cin + ci) * 9];
                                for (int ky = 0; ky < 3; ++ky)
                                    for (int kx = 0; kx < 3; ++kx) {
                                        // source row of tap ky for output parity dy: rows {y-1, y} (dy = 0) or {y, y+1} (dy = 1) of the low-res image
                                        const int a = dy == 0 ? (ky >= 1) : (ky >= 2), b = dx == 0 ? (kx >= 1) : (kx >= 2);
                                        we[(a + dy) * 3 + (b + dx)] += w9[ky * 3 + kx];      // embedded position: low-res row y - 1 + (a + dy)
                                    }
                            }
                    }
                    const std::string nm = p + "dec3#p" + std::to_string(dy) + std::to_string(dx);
                    // every output channel of a call's weight must be routed: slice the embedded filter per launch
                    const Layer l9 = {l3.cout, l3.cin, 3, 3};
                    const SubW wa = rows(l9, &w9e, f3.b, 5, 64), wb = rows(l9, &w9e, f3.b, 69, 64), wf = rows(l9, &w9e, f3.b, 0, 5);
                    conv(th, nm + "a", {fsrc(B["d2"], 0)},
                         {D(phase_view(fview(B["rF"], 0, 0), dy, dx), range(0, 64), T, DEMFI_MODE_STORE, phase_view(fview(aF, 0, 0), dy, dx))},
                         H2, W2, ConvOpt().weights(wa));
                    conv(th, nm + "b", {fsrc(B["d2"], 0)},
                         {D(phase_view(fview(B["rF"], 0, 1), dy, dx), range(0, 64), T, DEMFI_MODE_STORE, phase_view(fview(aF, 0, 1), dy, dx))},
                         H2, W2, ConvOpt().weights(wb));
                    wf2.w.insert(wf2.w.end(), wf.w.begin(), wf.w.end());
                    wf2.b.insert(wf2.b.end(), wf.b.begin(), wf.b.end());
                }
                if (status >= 0) {
                    // couts 0..4: column parity 0, 5..9: column parity 1; the 5 planes also go, as fp16, into the record Mixer.conv_delta1
                    // stages (delta16): no plane-packing launch.  The packed copy of parity 1 lies one pixel (16 channels) further in delta16
                    conv(th, p + "dec3#p" + std::to_string(dy) + "xf", {fsrc(B["d2"], 0)},
                         {D(phase_view(delta_v(0, 0), dy, 0), range(0, 4), DEMFI_ACT_NONE, DEMFI_MODE_STORE, phase_view(tview(B["ft"]), dy, 0)),
                          D(phase_view(delta_v(0, 4), dy, 0), {4}, DEMFI_ACT_NONE, DEMFI_MODE_STORE, phase_view(tview(ffo, 4), dy, 0)),
                          D(phase_view(delta_v(0, 0), dy, 1), range(5, 9), DEMFI_ACT_NONE, DEMFI_MODE_STORE, phase_view(tview(B["ft"]), dy, 1)),
                          D(phase_view(delta_v(0, 4), dy, 1), {9}, DEMFI_ACT_NONE, DEMFI_MODE_STORE, phase_view(tview(ffo, 4), dy, 1))},
                         H2, W2, ConvOpt().weights(wf2).packed(phase_view(fview(B["delta16"]), dy, 0), 0, 4, 16, 20));
                }
            }
        } else
        conv(th, p + "dec3", {fsrc(B["d2"], 0, 0, -1, -1, 1)},
             {D(fview(B["rF"], 0, 0), range(5, 69), T, DEMFI_MODE_STORE, fview(aF, 0, 0)),
              D(fview(B["rF"], 0, 1), range(69, 133), T, DEMFI_MODE_STORE, fview(aF, 0, 1)),
              D(delta_v(0, 0), range(0, 4), DEMFI_ACT_NONE, DEMFI_MODE_STORE, tview(B["ft"])),
              D(delta_v(0, 4), {4}, DEMFI_ACT_NONE, DEMFI_MODE_STORE, tview(ffo, 4))}, H, W);
        warp(th, "warp_fat", 64, fview(B["rF"], 0, 0), fview(B["rF"], 0, 1), fview(B["rF"], 0, 2), delta_p(0, 0), delta_p(0, 2),
             delta_p(0, 4), plane(B["occ"], 0), tp);                 // rFt -> rF[2], occ[0]
        // D1 on the three frames (Conv3d depth = batch), DeMFInet.py:95-101
        conv(th, "Dec_first", {fsrc(B["rF"], 0)}, {D(fview(B["dec_a"]), range(0, 64), R)}, H, W, ConvOpt().batched(3));
        const Tensor* cur = resblocks(th, "Decoder_res", c->hp.num_resb_dec, B["dec_a"], B["dec_t"], B["dec_b"], H, W, 3);
        conv(th, "Dec_last1", {fsrc(*cur, 0)}, {D(fview(B["dec_t"]), range(0, 64), R)}, H, W, ConvOpt().batched(3));
        conv(th, "Dec_last2", {fsrc(B["dec_t"], 0)}, {D(tview(B["sharp1"], 0, 3ll * H * W), range(0, 3))}, H, W, ConvOpt().batched(3));
        conv(th, "Ch_Reducer", {fsrc(B["rF"], 0, 0, -1, 0), fsrc(B["rF"], 64, 0, -1, 1), fsrc(B["rF"], 128, 0, -1, 2)},
             {D(fview(B["frec0"]), range(0, 64), T)}, H, W);
        // Mixer reference branch (iteration-invariant, hoisted): cat[S0p,S1p,Stp,B0,B1,B-1,B2 | flow_10,flow_01 | t_ref]
        p = "Booster_Module.";
        std::vector<const float*> xpl;                              // B0, B1, B-1, B2 colour planes (cat order)
        for (int f = 0; f < 4; ++f)
            for (int col = 0; col < 3; ++col) xpl.push_back(plane(x, col * 4 + f));
        std::vector<int32_t> agg3s_cin = range(0, 6);                // fp32 plan: channel map of the 27-plane pack
        if (c->dtype == DEMFI_F16) {
            // per-t planes only; the window-constant 16 planes were done in the trunk (xff16 -> re1w, g_pw)
            std::vector<const float*> pl;
            for (int i = 0; i < 9; ++i) pl.push_back(plane(B["sharp1"], i));
            for (int i = 0; i < 5; ++i) pl.push_back(delta_p(0, i));
            // round 6: channel 14 = occ_0, so that this ONE record also serves Dec_first_2's recursion-invariant per-t planes (rounds 2-5
            // packed a second record, agg16 = S0p, S1p | occ_0 | rflow, from the same planes: one more launch per window, 0.29 ms)
            pl.push_back(plane(B["occ"], 0));
            pack(th, pl, B["ref16"]);
            std::vector<int32_t> sel = range(0, 9), m = range(0, 14);
            for (int i = 25; i < 30; ++i) sel.push_back(i);
            m.insert(m.end(), 2, -1);
            SubW w1 = sub_weight(p + "Mixer.conv_ref1", sel, true);
            conv(th, p + "Mixer.conv_ref1#t", {fsrc_map(B["ref16"], m)}, {D(fview(B["re1"]), range(0, 32), R, DEMFI_MODE_STORE, fview(TB["re1w"]))},
                 H, W, ConvOpt().weights(w1));
            // the iteration-invariant, t-dependent part of Agg3 (DeMFInet.py:151-155: S0p,S1p | occ_0 | rflow_t0,t1) is read from ref16
            // through a channel map (dyn_m16 below)
        } else {
            {
                std::vector<const float*> pl;
                for (int i = 0; i < 9; ++i) pl.push_back(plane(B["sharp1"], i));
                pl.insert(pl.end(), xpl.begin(), xpl.end());
                for (int i : {2, 3, 0, 1}) pl.push_back(plane(ffo, i));
                for (int i = 0; i < 5; ++i) pl.push_back(delta_p(0, i));
                pack(th, pl, B["ref32"]);
                std::vector<int32_t> m = range(0, 30);
                m.insert(m.end(), 2, -1);
                conv(th, p + "Mixer.conv_ref1", {fsrc_map(B["ref32"], m)}, {D(fview(B["re1"]), range(0, 32), R)}, H, W);
            }
            // iteration-invariant part of Agg3 (DeMFInet.py:151-155): S0p,S1p | occ_0 | rflow_t0,t1 | flow_10,flow_01 | frames
            std::vector<const float*> pl;
            for (int i = 0; i < 6; ++i) pl.push_back(plane(B["sharp1"], i));
            pl.push_back(plane(B["occ"], 0));
            for (int i = 0; i < 4; ++i) pl.push_back(delta_p(0, i));
            for (int i : {2, 3, 0, 1}) pl.push_back(plane(ffo, i));
            pl.insert(pl.end(), xpl.begin(), xpl.end());
            pack(th, pl, B["agg3s"]);
            agg3s_cin.push_back(73);
            for (int i = 74; i < 82; ++i) agg3s_cin.push_back(i);
            for (int i = 87; i < 99; ++i) agg3s_cin.push_back(i);
            agg3s_cin.insert(agg3s_cin.end(), 5, -1);
        }
        conv(th, p + "Mixer.conv_ref2", {fsrc(B["re1"], 0)}, {D(fview(B["rd64"], 0), range(0, 32), R)}, H, W);
        // Dec_first_2 = relu(conv3x3(Agg3)) with Agg3 = cat[F_rec (64, changes per recursion) | 27 recursion-invariant planes |
        // 8 planes of the current recursion] (DeMFInet.py:151-157), split by linearity in the fp16 plan (see below).
        const std::vector<int32_t> a3d_sel = {6, 7, 8, 82, 83, 84, 85, 86};
        SubW w_dyn, w_rec;
        std::vector<int32_t> dyn_m16 = range(0, 11);
        if (c->dtype == DEMFI_F16) {
            // per recursion: ONE narrow launch over [ref16 (its 11 planes Agg3 holds: t-dependent, recursion-invariant) | agg3d (8 planes of this
            // recursion)] + bias + the window-constant share (g_pw, trunk) -> g_p2; then the F_rec part on the 64 -> 64 kernel.  ONE launch
            // on wsconv.hip with g_pw as the residual was measured slower (0.98 ms against 0.44 + 0.51 ms, profiles/r06_notes.md section 6)
            std::vector<int32_t> sel = range(0, 6);                  // S0p, S1p | occ_0 | rflow_t0, rflow_t1 (agg16 order)
            for (int i = 73; i < 78; ++i) sel.push_back(i);
            sel.insert(sel.end(), a3d_sel.begin(), a3d_sel.end());
            w_dyn = sub_weight("Dec_first_2", sel, true);
            w_rec = sub_weight("Dec_first_2", range(9, 73), false);
            // ref16 channel -> input channel of the sub-layer (sel order): S0p, S1p -> 0..5; Stp unused; rflow_t0, rflow_t1 -> 7..10; the
            // occlusion logit unused; occ_0 (channel 14) -> 6
            dyn_m16 = {0, 1, 2, 3, 4, 5, -1, -1, -1, 7, 8, 9, 10, -1, 6, -1};
        }
        // ============================ recursive boosting, one list per iteration ====================================
        // SepConvGRU (838-857): z | r share their input -> one 128-cout conv (fp32 plan); round 6, fp16: see fuse_gru
        const bool gru6 = c->dtype == DEMFI_F16;
        SubW zr[2];
        for (int s = 0; s < 2 && !gru6; ++s) zr[s] = concat_cout({p + "GB.convz" + std::to_string(s + 1), p + "GB.convr" + std::to_string(s + 1)});
        for (int it = 0; it < N; ++it) {
            OpList& sg = tb > 1 ? c->tb_iter_ops[k][it] : c->iter_ops[k][q][it];
            const Tensor& hin = B[it % 2 ? "frec1" : "frec0"];
            const Tensor& hout = B[it % 2 ? "frec0" : "frec1"];
            {
                // delta16 = the 5 flow / occlusion planes of step `it` as one NHWC record (+ 11 zero channels).  fp16 plan: written by
                // the producer's thin epilogue (dec3#f for step 0, flow_occ.conv2 of the previous recursion otherwise: demfi_conv.pack);
                // fp32 plan (general kernel): a plane-packing launch
                if (c->dtype != DEMFI_F16) {
                    std::vector<const float*> pl;
                    for (int i = 0; i < 5; ++i) pl.push_back(delta_p(it, i));
                    pack(sg, pl, B["delta16"]);
                }
                // the first 8 channels of the record as the piece (5 planes + 3 unused), the other 8 of the k-step as zero padding: the shape
                // the 7x7 kernel's paired-tap mode takes (conv_narrow.hip, P7); the fp32 plan (general kernel) is indifferent
                std::vector<int32_t> m = range(0, 5);
                m.insert(m.end(), 3, -1);
                conv(sg, p + "Mixer.conv_delta1", {fsrc_map(B["delta16"], m)}, {D(fview(B["de1"]), range(0, 32), R)}, H, W);
            }
            conv(sg, p + "Mixer.conv_delta2", {fsrc(B["de1"], 0)}, {D(fview(B["rd64"], 32), range(0, 32), R)}, H, W);
            conv(sg, p + "Mixer.conv_blend1", {fsrc(B["rd64"], 0)}, {D(fview(B["bl1"]), range(0, 32), R)}, H, W);
            conv(sg, p + "Mixer.conv_blend2", {fsrc(B["bl1"], 0)}, {D(fview(B["xb"]), range(0, 64), R)}, H, W);
            const Tensor* h = &hin;
            for (int s = 0; s < 2; ++s) {
                const Tensor& hnext = s == 0 ? B["h1"] : hout;
                const std::string sfx = std::to_string(s + 1);
                if (gru6) {
                    // round 6: r*h, then z + q + blend in one launch (fuse_gru); the three plain layers of the reference module
                    conv(sg, p + "GB.convr" + sfx, {fsrc(*h, 0), fsrc(B["xb"], 64)},
                         {D(fview(B["rh"]), range(0, 64), DEMFI_ACT_NONE, DEMFI_MODE_MUL, fview(*h))}, H, W);
                    conv(sg, p + "GB.convz" + sfx, {fsrc(*h, 0), fsrc(B["xb"], 64)}, {D(fview(B["zb"]), range(0, 64), DEMFI_ACT_SIGMOID)}, H, W);
                } else
                conv(sg, p + "GB.convzr" + sfx, {fsrc(*h, 0), fsrc(B["xb"], 64)},
                     {D(fview(B["zb"]), range(0, 64), DEMFI_ACT_SIGMOID),
                      D(fview(B["rh"]), range(64, 128), DEMFI_ACT_NONE, DEMFI_MODE_MUL, fview(*h))}, H, W, ConvOpt().weights(zr[s]));
                conv(sg, p + "GB.convq" + sfx, {fsrc(B["rh"], 0), fsrc(B["xb"], 64)},
                     {D(fview(hnext), range(0, 64), DEMFI_ACT_NONE, DEMFI_MODE_GRU, fview(*h), fview(B["zb"]))}, H, W);
                if (gru6) fuse_gru(sg, p + "GB.step" + sfx);
                h = &hnext;
            }
            conv(sg, p + "flow_occ.conv1", {fsrc(hout, 0)}, {D(fview(B["fo1"]), range(0, 32), R)}, H, W);
            ConvOpt fo2;
            if (c->dtype == DEMFI_F16) fo2.packed(fview(B["delta16"]), 0);     // step it+1's record for the next recursion's conv_delta1
            conv(sg, p + "flow_occ.conv2", {fsrc(B["fo1"], 0)},
                 {D(delta_v(it + 1, 0), range(0, 5), DEMFI_ACT_NONE, DEMFI_MODE_STORE, delta_v(it, 0))}, H, W, fo2);
            // PWB of the recursion; the kernel also writes Agg3's per-recursion planes [St_new | rflow_t0, rflow_t1 | occ]
            // (DeMFInet.py:151-155) as the NHWC record Dec_first_2 reads (agg3d): no plane-packing launch
            warp(sg, "warp_thin", 3, tview(B["sharp1"], 0), tview(B["sharp1"], 3), tview(B["stnew"]), delta_p(it + 1, 0), delta_p(it + 1, 2),
                 delta_p(it + 1, 4), plane(B["occ"], it + 1), tp, ptr(B["agg3d"]));
            if (c->dtype == DEMFI_F16) {
                conv(sg, "Dec_first_2#dyn", {fsrc_map(B["ref16"], dyn_m16), fsrc_map(B["agg3d"], range(11, 19))},
                     {D(fview(B["g_p2"]), range(0, 64), DEMFI_ACT_NONE, DEMFI_MODE_STORE, fview(TB["g_pw"]))}, H, W, ConvOpt().weights(w_dyn));
                conv(sg, "Dec_first_2#rec", {fsrc(hout, 0)}, {D(fview(B["g_a"]), range(0, 64), R, DEMFI_MODE_STORE, fview(B["g_p2"]))}, H, W, ConvOpt().weights(w_rec));
            } else
            conv(sg, "Dec_first_2", {fsrc(hout, 9), fsrc_map(B["agg3s"], agg3s_cin), fsrc_map(B["agg3d"], a3d_sel)},
                 {D(fview(B["g_a"]), range(0, 64), R)}, H, W);
            const Tensor* g = resblocks(sg, "Decoder_res_2", c->hp.num_resb_dec, B["g_a"], B["g_t"], B["g_b"], H, W, 1);
            conv(sg, "Dec_last1_2", {fsrc(*g, 0)}, {D(fview(B["g_t"]), range(0, 64), R)}, H, W);
            conv(sg, "Dec_last2_2", {fsrc(B["g_t"], 0)},
                 {D(tview(B["finals"], 9 * it + 0), range(0, 3), DEMFI_ACT_NONE, DEMFI_MODE_STORE, tview(B["sharp1"], 0)),
                  D(tview(B["finals"], 9 * it + 3), range(3, 6), DEMFI_ACT_NONE, DEMFI_MODE_STORE, tview(B["sharp1"], 3)),
                  D(tview(B["finals"], 9 * it + 6), range(6, 9), DEMFI_ACT_NONE, DEMFI_MODE_STORE, tview(B["stnew"]))}, H, W,
                 ConvOpt().to_sink(ptr(B["sink"]), it));
        }
    }
};

}  // namespace

int run_builder(demfi_ctx* c, bool dry)
{
    c->blob_fill = 0;
    c->descs.clear();
    c->pack_cache.clear();
    c->tr_ops.assign(c->n_trunk, OpList());
    c->head_ops.assign(c->n_trunk, std::vector<OpList>(c->n_ctx));
    c->iter_ops.assign(c->n_trunk, std::vector<std::vector<OpList>>(c->n_ctx, std::vector<OpList>(c->N)));
    c->tb_head_ops.assign(c->n_trunk, OpList());
    c->tb_iter_ops.assign(c->n_trunk, std::vector<OpList>(c->N));
    c->fused_now.clear();
    Builder b{c, esz_of(c), c->dtype == DEMFI_F32, dry};
    // the sizing pass records which launches it fused; the bind pass must fuse the same ones (their untouched scratch has no memory)
    auto done = [&]() {
        if (b.status < 0) return b.status;
        if (dry) c->fused_dry = c->fused_now;
        else if (c->fused_now != c->fused_dry)
            return demfi_set_error(DEMFI_ERR_ARG, "demfi_ctx_bind: the bound plan fuses %d launches, the sizing pass fused %d (or others): the "
                                   "arena gave their scratch buffers no memory -- set DEMFI_ARENA=0 and report", (int)c->fused_now.size(), (int)c->fused_dry.size());
        return b.status;
    };
    if (c->op_kind) {
        b.build_operator();
        return done();
    }
    for (int k = 0; k < c->n_trunk && b.status >= 0; ++k) {
        b.build_trunk(k);
        for (int q = 0; q < c->n_ctx && b.status >= 0; ++q) b.build_t(k, q);
        if (c->n_ctx > 1 && b.status >= 0) {                    // the batched plan over all contexts of this trunk set
            b.tb = c->n_ctx; b.tb_k = k;
            b.build_t(k, 0);
            b.tb = 1;
        }
    }
    return done();
}

}  // namespace plan
