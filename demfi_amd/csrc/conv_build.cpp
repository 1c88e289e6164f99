// Convolution descriptor builder (shared by demfi_conv_build and the plan): shapes a call site for the kernel that owns it, then packs
// its weights in that shape.  Host logic only.
#include "plan.h"
#include <algorithm>
#include <string.h>

namespace plan {

constexpr int64_t LDS_BUDGET = 78 * 1024;      // general kernel: haloed tile + 2-tap weight ring, 2 workgroups per CU

int conv_shape(int dtype, int H, int W, int stride, int batch, const Layer& l, const demfi_conv_src* srcs, int n_srcs,
               const demfi_conv_dst* dsts, int n_dsts, ConvShape& out, const char* name, int pad_y, int pad_x, int grid_div)
{
    if (dtype != DEMFI_F16 && dtype != DEMFI_F32) return demfi_set_error(DEMFI_ERR_ARG, "%s: dtype", name);
    if (!srcs || !dsts || n_srcs <= 0 || n_dsts <= 0 || n_dsts > DEMFI_MAX_SEGS || (stride != 1 && stride != 2))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: sources / destinations / stride", name);
    const int cout = l.cout, cin = l.cin, kh = l.kh, kw = l.kw;
    const int esz = dtype == DEMFI_F32 ? 4 : 2;
    const int64_t LH = 7 * stride + kh, LW = 31 * stride + kw;
    int n_oct = 0;
    for (int i = 0; i < n_dsts; ++i) n_oct += (dsts[i].n + 7) / 8;
    const int sub = (n_oct + 3) / 4;
    int nco = sub <= 5 ? sub : 4;
    int rec = 128;
    // round 6: the stride-2 4x4 layers (UNet encoders, DeMFInet.py:575-577) whose inputs are NHWC pieces of 32-channel multiples (+ at
    // most one 16-channel tail) and whose outputs are 64-channel blocks of one NHWC tensor belong to the phase-decomposed streamed-weight
    // kernel (wsconv.hip): units of 32 channels (64-byte records, a 16-channel tail padded to a whole unit), two 32-cout subtiles per
    // work item
    // ... and so do the 3x3 stride-1 layers of that output shape with >= 96 input channels (the UNet decoders dec0 / dec1 / dec2 with their
    // upsampled pieces, FGAC's w_gen): the 64 -> 64 and the narrow layers keep their own kernels
    int src_nch = 0;
    for (int i = 0; i < n_srcs; ++i) src_nch += srcs[i].nch;
    const bool ws2_s2 = stride == 2 && kh == 4 && kw == 4, ws2_s1 = stride == 1 && kh == 3 && kw == 3 && src_nch > 64;
    bool ws2_shape = esz == 2 && (ws2_s2 || ws2_s1) && pad_y < 0 && pad_x < 0 && n_dsts == 1 && dsts[0].n % 64 == 0 &&
                     dsts[0].mode == DEMFI_MODE_STORE && (dsts[0].act == DEMFI_ACT_NONE || dsts[0].act == DEMFI_ACT_RELU) && dsts[0].scale <= 1 &&
                     dsts[0].dst.sc == 1 && !dsts[0].dst.is_f32 && (!dsts[0].res.ptr || (dsts[0].res.sc == 1 && !dsts[0].res.is_f32));
    for (int i = 0; ws2_shape && i < n_srcs; ++i)
        // a tail unit at the end: a 16-channel piece, optionally followed by an 8-channel one (Dec_first_2: ref16 | agg3d)
        ws2_shape = srcs[i].fat && !srcs[i].v.is_f32 &&
                    (srcs[i].nch % 32 == 0 || (srcs[i].nch == 16 && !srcs[i].up_shift && (i == n_srcs - 1 || (i == n_srcs - 2 && srcs[n_srcs - 1].nch == 8))) ||
                     (srcs[i].nch == 8 && !srcs[i].up_shift && i == n_srcs - 1 && i > 0 && srcs[i - 1].nch == 16)) &&
                    (srcs[i].up_shift == 0 || (srcs[i].up_shift == 1 && ws2_s1 && H % 2 == 0 && W % 2 == 0));
    if (ws2_shape) nco = 2;
    // the SepConvGRU layers (1x5 / 5x1 over two 64-channel NHWC pieces) run on their own persistent kernel, which wants
    // the two pieces as two 64-channel chunks whatever the general kernel's LDS budget says
    bool sep = esz == 2 && stride == 1 && ((kh == 1 && kw == 5) || (kh == 5 && kw == 1)) && n_srcs == 2 && (cout == 64 || cout == 128);
    for (int i = 0; sep && i < n_srcs; ++i) sep = srcs[i].fat && srcs[i].nch == 64 && !srcs[i].up_shift;
    while (!sep && rec > 32 && LH * LW * (rec + 16) + 2 * (rec / 32) * nco * 1024 > LDS_BUDGET) rec /= 2;
    // Small grids (the half- and lower-resolution layers: 920 tiles at 720p): with 128-byte records only two workgroups fit a
    // CU (LDS), so ~1000 workgroups run in two rounds; 64-byte records (five per CU) finish in one.  Not for the single
    // 64-channel 3x3 shape, which belongs to the persistent kernel (it needs 128-byte records).
    {
        // grid_div: the batched per-t plan runs the layer over batch = images x contexts; the choice is made on the grid of ONE
        // context so that both plans use the same record size, i.e. the same summation order: bit-identical results
        const int64_t n_wg = (int64_t)((W + 31) / 32) * ((H + 7) / 8) * (batch / grid_div) * ((sub + nco - 1) / nco);
        const bool persist_shape = n_srcs == 1 && srcs[0].fat && srcs[0].nch == 64 && kh == 3 && kw == 3 && stride == 1;
        // measured at 720p (same box): the 48 RDB growth convs 0.045-0.072 -> 0.035-0.058 ms, dec2 0.082 -> 0.070; the 96-cout
        // layers (nco = 3: LFF, GFF.1) get slower with it, hence nco <= 2
        if (!sep && !persist_shape && rec == 128 && nco <= 2 && n_wg <= 5 * 256) rec = 64;
        // round 5: the RDB growth shape (3x3, <= 32 couts, >= 3 units of 32 channels from NHWC pieces) belongs to the 3x3 instantiation
        // of the streamed-weight kernel at any grid size: it walks 32-channel units (64-byte records)
        bool rdb_shape = !sep && esz == 2 && kh == 3 && kw == 3 && stride == 1 && sub == 1 && n_dsts == 1 && dsts[0].n == 32 && cin >= 96 && pad_y < 0 && pad_x < 0;
        for (int i = 0; rdb_shape && i < n_srcs; ++i) rdb_shape = srcs[i].fat && !srcs[i].up_shift && srcs[i].nch % 32 == 0;
        if (rdb_shape || ws2_shape) rec = 64;
    }

    // ---- every original input channel must be fed exactly once ------------------------------------------------
    {
        std::vector<int> seen(cin, 0);
        for (int i = 0; i < n_srcs; ++i)
            for (int j = 0; j < srcs[i].nch; ++j) {
                const int c = srcs[i].cin[j];
                if (c >= cin) return demfi_set_error(DEMFI_ERR_ARG, "%s: input map names channel %d >= cin %d", name, c, cin);
                if (c >= 0) seen[c]++;
            }
        for (int c = 0; c < cin; ++c)
            if (seen[c] != 1) return demfi_set_error(DEMFI_ERR_ARG, "%s: input channel %d fed %d times", name, c, seen[c]);
    }
    // ---- pack the input pieces into chunks of <= rec bytes (fat pieces first: 16-byte aligned) -------------------
    struct P { demfi_view v; int nch, lds_ch, up, fat; };
    struct Ck { int first, n, nks; };
    std::vector<P> pieces;
    std::vector<Ck> chunks;
    std::vector<int32_t>&cin_map = out.cin_map, &cout_map = out.cout_map, &nks = out.nks;
    cin_map.clear(); cout_map.clear(); nks.clear();
    int first = 0, fill = 0;
    const demfi_view null_view = {nullptr, 0, 0, 0, 0, 0, 0};
    auto close_chunk = [&]() {
        if (fill == 0) return;
        const int unit = ws2_shape ? 64 : 32;                     // wsconv.hip walks whole 32-channel units
        const int padb = (unit - fill % unit) % unit;
        if (padb) {
            pieces.push_back({null_view, padb / esz, fill / esz, 0, 0});
            cin_map.insert(cin_map.end(), padb / esz, -1);
            fill += padb;
        }
        chunks.push_back({first, (int)pieces.size() - first, fill / 32});
        first = (int)pieces.size();
        fill = 0;
    };
    std::vector<int> order;
    for (int i = 0; i < n_srcs; ++i) if (srcs[i].fat) order.push_back(i);
    for (int i = 0; i < n_srcs; ++i) if (!srcs[i].fat) order.push_back(i);
    for (int si : order) {
        const demfi_conv_src& s = srcs[si];
        const int selt = s.v.is_f32 ? 4 : 2;
        int done = 0;
        while (done < s.nch) {
            if (fill >= rec) close_chunk();
            const int room = (rec - fill) / esz;
            int take;
            if (s.fat) {
                if (fill % 16) {
                    const int padc = (16 - fill % 16) / esz;
                    pieces.push_back({null_view, padc, fill / esz, 0, 0});
                    cin_map.insert(cin_map.end(), padc, -1);
                    fill += padc * esz;
                    continue;
                }
                take = std::min(s.nch - done, room);
                int vec = take * esz / 16;
                if (vec == 0) { close_chunk(); continue; }
                int p2 = 1;
                while (p2 * 2 <= vec) p2 *= 2;                       // 1, 2, 4, 8 vectors per pixel
                take = p2 * 16 / esz;
            } else {
                take = std::min(s.nch - done, room);
            }
            demfi_view v = s.v;
            v.ptr = s.v.ptr ? (char*)s.v.ptr + (int64_t)done * s.v.sc * selt : nullptr;
            pieces.push_back({v, take, fill / esz, s.up_shift, s.fat ? 1 : 0});
            cin_map.insert(cin_map.end(), s.cin + done, s.cin + done + take);
            fill += take * esz;
            done += take;
        }
    }
    close_chunk();
    if ((int)chunks.size() > DEMFI_MAX_CHUNKS || (int)pieces.size() > DEMFI_MAX_PIECES)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d chunks / %d pieces", name, (int)chunks.size(), (int)pieces.size());
    // ---- output routing ----------------------------------------------------------------------------------------
    struct Oct { int seg, n, ch; };
    std::vector<Oct> octs;
    for (int si = 0; si < n_dsts; ++si) {
        const demfi_conv_dst& ds = dsts[si];
        for (int o = 0; o < ds.n; o += 8) {
            const int k = std::min(8, ds.n - o);
            octs.push_back({si, k, o});
            for (int j = 0; j < 8; ++j) cout_map.push_back(j < k ? ds.couts[o + j] : -1);
        }
    }
    {
        std::vector<int> seen(cout, 0);
        for (int c : cout_map) {
            if (c >= cout) return demfi_set_error(DEMFI_ERR_ARG, "%s: output map names channel %d >= cout %d", name, c, cout);
            if (c >= 0) seen[c]++;
        }
        for (int c = 0; c < cout; ++c)
            if (seen[c] != 1) return demfi_set_error(DEMFI_ERR_ARG, "%s: output channel %d routed %d times", name, c, seen[c]);
    }
    const int cout_pad = (sub + nco - 1) / nco * nco * 32;
    if (cout_pad > 256) return demfi_set_error(DEMFI_ERR_ARG, "%s: %d packed output channels > 256", name, cout_pad);
    while ((int)octs.size() < cout_pad / 8) {
        octs.push_back({0, 0, 0});
        cout_map.insert(cout_map.end(), 8, -1);
    }
    for (auto& c : chunks) nks.push_back(c.nks);
    // ---- descriptor ----------------------------------------------------------------------------------------------
    demfi_conv& d = out.d;
    memset(&d, 0, sizeof(d));
    d.dtype = dtype; d.H = H; d.W = W;
    d.inH = stride == 2 ? H * stride : H;
    d.inW = stride == 2 ? W * stride : W;
    d.kh = kh; d.kw = kw; d.stride = stride;
    d.pad_y = pad_y >= 0 ? pad_y : (stride == 2 ? 1 : kh / 2);      // explicit: the 2x2 phase filters of an upsampled 3x3 layer
    d.pad_x = pad_x >= 0 ? pad_x : (stride == 2 ? 1 : kw / 2);
    d.batch = batch; d.cout_pad = cout_pad; d.nco = nco; d.rec_bytes = rec;
    d.n_chunks = (int)chunks.size(); d.n_pieces = (int)pieces.size(); d.n_segs = n_dsts;
    const int taps = kh * kw;
    int64_t tot_ks = 0;
    for (int k : nks) tot_ks += k;
    d.w_blk_stride = tot_ks * taps * nco * 64;
    int64_t woff = 0;
    for (size_t i = 0; i < chunks.size(); ++i) {
        d.chunks[i].first_piece = chunks[i].first;
        d.chunks[i].n_pieces = chunks[i].n;
        d.chunks[i].nks = chunks[i].nks;
        d.chunks[i].w_off = woff;
        woff += (int64_t)chunks[i].nks * taps * nco * 64;
    }
    for (size_t i = 0; i < pieces.size(); ++i) {
        d.pieces[i].v = pieces[i].v;
        d.pieces[i].nch = pieces[i].nch;
        d.pieces[i].lds_ch = pieces[i].lds_ch;
        d.pieces[i].up_shift = pieces[i].up;
        d.pieces[i].fat = pieces[i].fat;
    }
    for (int i = 0; i < n_dsts; ++i) {
        demfi_seg& sg = d.segs[i];
        sg.dst = dsts[i].dst; sg.res = dsts[i].res; sg.aux = dsts[i].aux;
        sg.act = dsts[i].act; sg.mode = dsts[i].mode;
        sg.scale = dsts[i].scale ? dsts[i].scale : 1;
        sg.dy = dsts[i].dy; sg.dx = dsts[i].dx;
    }
    for (size_t i = 0; i < octs.size(); ++i) { d.oct_seg[i] = octs[i].seg; d.oct_n[i] = octs[i].n; d.oct_ch[i] = octs[i].ch; }
    for (int sb = 0; sb < DEMFI_MAX_OCTS / 4; ++sb) d.sub_seg[sb] = -1;
    const bool f32 = dtype == DEMFI_F32;
    auto fat_ok = [&](const demfi_view& v) { return v.ptr && v.sc == 1 && (v.is_f32 != 0) == f32; };
    for (int sb = 0; sb < cout_pad / 32; ++sb) {
        const Oct* o4 = &octs[sb * 4];
        const int si = o4[0].seg;
        const demfi_conv_dst& ds = dsts[si];
        bool ok = o4[0].ch % 8 == 0;
        for (int j = 0; j < 4; ++j) ok = ok && o4[j].seg == si && o4[j].n == 8 && o4[j].ch == o4[0].ch + 8 * j;
        ok = ok && fat_ok(ds.dst) && (!ds.res.ptr || fat_ok(ds.res));
        if (ds.mode == DEMFI_MODE_GRU) ok = ok && fat_ok(ds.aux);
        if (ds.mode != DEMFI_MODE_STORE) ok = ok && ds.res.ptr;
        if (ok) d.sub_seg[sb] = si;
    }
    d.lw_magic = (uint32_t)((0x100000000ull + LW - 1) / LW);
    out.macs = (int64_t)cout * cin * taps * H * W * batch;
    // ---- cout order --------------------------------------------------------------------------------------------
    // Layers of the persistent kernels (conv.hip: 64-channel 3x3, narrow with an NHWC destination, SepConvGRU) are packed in their cout order: MFMA
    // row r of a 32-cout subtile holds channel (r>>4)*16 + ((r>>2)&1)*8 + ((r>>3)&1)*4 + (r&3), which makes the two accumulator
    // quads of a lane 8 consecutive channels (a 16-byte store without any cross-lane exchange).  The octet tables keep
    // describing the un-permuted routing (that kernel only reads oct_ch[0]).
    {
        demfi_conv probe = d;
        probe.zero_page = &probe;                                   // the context / caller sets the real one later
        if (!probe.pieces[0].v.ptr) probe.pieces[0].v.ptr = &probe; // sizing pass
        if (demfi_persist_eligible(&probe)) {
            d.cout_perm = 1;
            std::vector<int32_t> pm(cout_map.size());
            for (size_t i = 0; i < cout_map.size(); ++i) {
                const int sb = (int)i / 32, r = (int)i % 32;
                pm[i] = cout_map[sb * 32 + (r >> 4) * 16 + ((r >> 2) & 1) * 8 + ((r >> 3) & 1) * 4 + (r & 3)];
            }
            cout_map.swap(pm);
        }
    }
    out.wbytes = d.w_blk_stride * 16 * (cout_pad / (32 * nco));    // what demfi_pack_conv_weights writes
    return DEMFI_OK;
}

int conv_pack(const ConvShape& s, const Layer& l, const float* w, const float* bias, std::vector<uint8_t>& wpack, std::vector<float>& bias_packed)
{
    int64_t nbytes = 0;
    wpack.resize(s.wbytes);
    const int st = demfi_pack_conv_weights(w, l.cout, l.cin, l.kh, l.kw, s.cin_map.data(), (int)s.cin_map.size(), s.nks.data(), (int)s.nks.size(),
                                           s.cout_map.data(), s.d.cout_pad, s.d.nco, s.d.dtype, wpack.data(), &nbytes);
    if (st < 0) return st;
    if (nbytes != s.wbytes) return demfi_set_error(DEMFI_ERR_ARG, "conv_pack: %lld B packed, %lld B planned", (long long)nbytes, (long long)s.wbytes);
    bias_packed.assign(s.d.cout_pad, 0.0f);
    for (int i = 0; i < s.d.cout_pad; ++i)
        if (s.cout_map[i] >= 0 && bias) bias_packed[i] = bias[s.cout_map[i]];
    return DEMFI_OK;
}

}  // namespace plan

extern "C" int demfi_conv_build(int dtype, int H, int W, int stride, int batch, const float* w, const float* bias, int cout, int cin,
                                int kh, int kw, const demfi_conv_src* srcs, int n_srcs, const demfi_conv_dst* dsts, int n_dsts,
                                demfi_conv* desc, void* wpack, int64_t* wpack_bytes, float* bias_packed, int32_t* cout_pad)
{
    if (!w || !desc || !wpack_bytes || !cout_pad || H <= 0 || W <= 0 || batch <= 0 || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_conv_build: bad arguments");
    const plan::Layer l = {cout, cin, kh, kw};
    plan::ConvShape s;
    int st = plan::conv_shape(dtype, H, W, stride, batch, l, srcs, n_srcs, dsts, n_dsts, s, "demfi_conv_build");
    if (st < 0) return st;
    *cout_pad = s.d.cout_pad;
    *wpack_bytes = s.wbytes;
    *desc = s.d;
    if (!wpack) return DEMFI_OK;                                 // sizing call
    std::vector<uint8_t> wp;
    std::vector<float> bp;
    st = plan::conv_pack(s, l, w, bias, wp, bp);
    if (st < 0) return st;
    memcpy(wpack, wp.data(), wp.size());
    if (bias_packed) memcpy(bias_packed, bp.data(), bp.size() * 4);
    return DEMFI_OK;
}
