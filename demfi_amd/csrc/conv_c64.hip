// The 3x3 kernels for ONE 64-channel NHWC input piece: the 32-cout persistent kernel and the staged-store 64 -> 64 kernel (a unit of its own since
// round 6; the kernels are unchanged).
#include "conv_common.h"

namespace {

// ======================================================================================================
// Persistent specialisation for the workhorse shape of the network: fp16, stride 1, KHxKW filter, ONE NHWC
// input of 64 channels (128-byte pixel records), <= 64 output channels (all 3x3 64->64 layers of the FAC-FB
// encoder, D1 and D2: ~52 % of the MACs of a forward).
//   * one workgroup per CU walks many 8x32 output tiles (XCD-aware bands);
//   * ALL filter taps stay resident in LDS for the whole launch (72 KiB for 3x3x64x64) -> no per-tap weight
//     traffic and no per-tap barriers;
//   * the haloed input tile is fetched by LDS-DMA (global_load_lds, no VGPR round trip, zero padding through a
//     zero page) into a double buffer: tile k+1 streams in while tile k is on the matrix cores;
//   * the epilogue needs no LDS and no cross-lane traffic: the layers of this kernel are packed in a permuted cout order
//     (demfi_conv.cout_perm) in which the two accumulator quads a lane owns are 8 consecutive output channels of its
//     pixel (16-byte stores / residual loads straight from registers), so there is ONE barrier per tile;
//   * pixel records are unpadded (128 B); bank conflicts are removed by an XOR swizzle of the 16-byte slot,
//     applied on the DMA's per-lane SOURCE address and on the ds_read address (the LDS image stays lane-linear).
// ======================================================================================================
constexpr int P_LW = TW + 2, P_LH = TH + 2;                    // 3x3 halo
constexpr int P_NP = P_LW * P_LH;                               // 340 pixels
constexpr int P_NI = (P_NP + 7) / 8;                            // 43 DMA instructions (8 pixels x 8 slots each)
constexpr int P_TILE_BYTES = P_NI * 1024;                       // 44,032 B per buffer

constexpr int P_NT = NT + 64;                                   // 4 MFMA waves + 1 DMA wave

// Both kernels add ONE 32-bit per-lane byte offset to a uniform 64-bit tile base.  Source: the DMA lanes' off[] spans the haloed window,
// up to P_LH rows and P_LW records (+ the 128-byte record) from the tile origin, a signed int in the 32-cout kernel.  Destination of the
// staged-store kernel: the helpers' doff[] spans the TH x TW output tile.  (The MFMA waves' own stores and every residual load multiply
// int64 strides.)  A view beyond these bounds is not this family's: demfi_conv_owner passes it on.
constexpr int64_t P_OFF_LIMIT = (int64_t)1 << 31;

// One k-step pair of fragments: 2 k-steps x (NCO A fragments + 2 B fragments)

#ifndef DEMFI_P_NDMA
#define DEMFI_P_NDMA 2
#endif
constexpr int P_NDMA = DEMFI_P_NDMA;                            // waves issuing the tile DMA (instruction i -> wave i % P_NDMA)
template <int NCO, bool RES = true>   // RES: the segment has a residual input (compile time: keeps the loads free of phis)
__global__ __launch_bounds__(NT + 64 * P_NDMA, 1) void conv3x3_c64_persist_kernel(const demfi_conv* __restrict__ d)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NTAPS = 9, NKS = 4;
    constexpr int WBYTES = NTAPS * NKS * NCO * 1024;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = d->H, W = d->W;
    const int tiles_x = (W + TW - 1) / TW;
    const int tiles_y = (H + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y;
    const int total = tiles_img * d->batch;
    char* const wlds = smem;                                    // resident weights
    char* const tbuf = smem + WBYTES;                           // 2 x tile buffer

    // tile sequence of this workgroup: XCD x = b & 7 owns the contiguous band [lo, hi) of tile indices
    int t_first, t_end, t_step;
    XCD_TILE_STRIDE(total, t_first, t_end, t_step);
    if (t_first >= t_end) return;                               // uniform per workgroup

    auto tile_coords = [&](int t, int& bimg, int& oy0, int& ox0) {
        bimg = t / tiles_img;
        const int rem = t - bimg * tiles_img;
        const int ty = rem / tiles_x;
        oy0 = ty * TH;
        ox0 = (rem - ty * tiles_x) * TW;
    };

    if (wave >= 4) {
        // ================= DMA waves: own every global->LDS transfer, so only THEIR vmcnt tracks them ============
        const int dw = wave - 4;
        const demfi_piece& pc = d->pieces[0];
        const char* const src = (const char*)pc.v.ptr;
        const int64_t sx = pc.v.sx * 2, sy = pc.v.sy * 2, sb = pc.v.sb * 2;
        const char* const zeros = (const char*)d->zero_page;
        // instruction i covers pixels 8i..8i+7; lane -> (pixel 8i + lane/8, physical 16-byte slot lane%8).
        // The per-lane byte offsets relative to the tile origin and the (row, column) pairs never change: compute
        // them once (86 VGPRs) so that issuing a tile is ~4 VALU per DMA instruction instead of ~50.
        int off[P_NI], lyx[P_NI];
#pragma unroll
        for (int i = 0; i < P_NI; ++i) {
            const int px = i * 8 + (lane >> 3);
            const int ly = px / P_LW;
            const int lxx = px - ly * P_LW;
            const int v = (lane & 7) ^ ((lxx >> 1) & 7);                // logical slot at this physical slot: swizzle by tile COLUMN
            off[i] = (int)(ly * sy + lxx * sx) + v * 16;
            lyx[i] = px < P_NP ? (ly | (lxx << 8)) : 0xffff;
        }
        auto issue_tile = [&](int t, int buf) {
            int bimg, oy0, ox0;
            tile_coords(t, bimg, oy0, ox0);
            const char* base = src + (int64_t)bimg * sb + (int64_t)(oy0 - 1) * sy + (int64_t)(ox0 - 1) * sx;
            char* dst = tbuf + buf * P_TILE_BYTES;
            const bool interior = oy0 >= 1 && oy0 + TH + 1 <= H && ox0 >= 1 && ox0 + TW + 1 <= W;
            if (interior) {
#pragma unroll
                for (int i = 0; i < P_NI; ++i) {
                    if ((i % P_NDMA) != dw) continue;            // wave-uniform
                    const char* g = (i == P_NI - 1 && lyx[i] == 0xffff) ? zeros : base + off[i];
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                     (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
                }
            } else {
#pragma unroll
                for (int i = 0; i < P_NI; ++i) {
                    if ((i % P_NDMA) != dw) continue;
                    const int iy = oy0 - 1 + (lyx[i] & 255), ix = ox0 - 1 + (lyx[i] >> 8);
                    const char* g = (lyx[i] != 0xffff && iy >= 0 && iy < H && ix >= 0 && ix < W) ? base + off[i] : zeros;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                     (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
                }
            }
        };
        const uint4* wsrc = (const uint4*)d->wpack;
        for (int i = dw; i < NTAPS * NKS * NCO; i += P_NDMA)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + i * 64 + lane),
                                             (__attribute__((address_space(3))) void*)(wlds + i * 1024), 16, 0, 0);
        issue_tile(t_first, 0);
        int buf = 0;
        [[maybe_unused]] int trk = 0;
        for (int t = t_first; t < t_end; t += t_step, buf ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t (and the weights) have landed in LDS
            TRACE_STAMP(wave, trk, 0);
            __syncthreads();                                    // A: hand tile t to the MFMA waves
            TRACE_STAMP(wave, trk, 1);
            if (t + t_step < t_end) issue_tile(t + t_step, buf ^ 1);   // streams in under the MFMAs
            TRACE_STAMP(wave, trk, 2);
            ++trk;
        }
        return;
    }

    // ================= MFMA waves ============================================================================
    const int hi = lane >> 5;
    const int lx = lane & 31;
    // ---- everything the epilogue needs from the descriptor, hoisted out of the tile loop (barriers are memory
    // fences: descriptor fields read inside the loop would be re-fetched through dependent scalar loads per tile)
    const demfi_seg& sg0 = d->segs[d->sub_seg[0]];
    half_t* const dstp = (half_t*)sg0.dst.ptr;
    const half_t* const resp = (const half_t*)sg0.res.ptr;
    const int64_t d_sx = sg0.dst.sx, d_sy = sg0.dst.sy, d_sb = sg0.dst.sb;
    const int64_t r_sx = sg0.res.sx, r_sy = sg0.res.sy, r_sb = sg0.res.sb;
    const float act_floor = sg0.act == DEMFI_ACT_RELU ? 0.0f : -__builtin_huge_valf();
    h8_t act_floor8;
#pragma unroll
    for (int j = 0; j < 8; ++j) act_floor8[j] = (half_t)act_floor;
    const int ch0 = d->oct_ch[0];
    // Epilogue layout (cout_perm): quads 2m and 2m+1 of lane (lx, hi) are the 8 consecutive output channels
    // s*32 + 16m + 8hi .. of pixel lx: 16-byte stores / residual loads straight from registers, no LDS transpose, no
    // lane exchange.  The bias (NCO*32 floats, MFMA-row order) sits in the 2 KiB of LDS behind the tile buffers.
    float* const bias_lds = (float*)(tbuf + 2 * P_TILE_BYTES);
    if (tid < NCO * 32) bias_lds[tid] = d->bias[tid];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the write is in LDS before this wave's first (raw) barrier A
    int boff[12];                                               // [kx*4 + ks]: (column lx+kx) record + swizzled 16-byte slot
#pragma unroll
    for (int g = 0; g < 12; ++g) {
        const int col = lx + (g >> 2);
        boff[g] = col * 128 + ((((g & 3) * 2 + hi) ^ ((col >> 1) & 7)) << 4);
    }
    const char* const wl = wlds + lane * 16;
    int buf = 0;
    [[maybe_unused]] int trk = -1;
    for (int t = t_first; t < t_end; t += t_step, buf ^= 1) {
        int bimg, oy0, ox0;
        tile_coords(t, bimg, oy0, ox0);
        ++trk;
        // Residual of this tile: issued before the MFMA phase, consumed in the epilogue.  The loads are unconditional
        // (clamped address, no per-lane branch) and barrier A is a RAW s_barrier: a lane-divergent load leaves register
        // copies behind and __syncthreads() carries a fence -- either one makes the compiler put s_waitcnt vmcnt(0)
        // in front of the MFMA phase, i.e. a full HBM round trip per tile (measured: +0.064 ms on the 0.28 ms launch).
        u4_t rreg[NCO][2][2];
        if constexpr (RES) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int oy = min(oy0 + wave * 2 + p, H - 1), oxx = min(ox0 + lx, W - 1);
                const half_t* rp = resp + bimg * r_sb + oy * r_sy + oxx * r_sx + ch0 + hi * 8;
#pragma unroll
                for (int s = 0; s < NCO; ++s) {
#pragma unroll
                    for (int m2 = 0; m2 < 2; ++m2) rreg[s][p][m2] = *gcp<u4_t>(rp + s * 32 + m2 * 16);
                }
            }
        }
        // A: tile t is in LDS (the DMA wave waited for it).  These waves wrote no LDS and consumed every ds_read of the
        // previous tile, so no counter has to drain here; "memory" keeps the compiler from moving LDS reads above it.
        TRACE_STAMP(wave, trk, 0);
        asm volatile("s_barrier" ::: "memory");
        TRACE_STAMP(wave, trk, 1);
        f16x_t acc[NCO][2];
#pragma unroll
        for (int s = 0; s < NCO; ++s) {
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[s][0][i] = 0.0f; acc[s][1][i] = 0.0f; }
        }
        const char* tb = tbuf + buf * P_TILE_BYTES + (wave * 2) * (P_LW * 128);
        // software pipeline over the taps: the fragments of group g+1 are in flight while the MFMAs of group g run (one wave per SIMD:
        // nothing else hides the LDS latency).
        // Input-row reuse across ky: for one (kx, k-step) the taps ky = 0..2 of output rows p = 0, 1 read input rows
        // p + ky = 0..3 at the same column offset -- 4 distinct B fragments feed 6 (ky, p) combinations.  One group =
        // 4 row fragments + 3*NCO weight fragments -> 6*NCO MFMAs: 10 ds_reads per 12 MFMAs instead of 12 (NCO = 2).
        struct RowFrag { uint4 a[3][NCO]; uint4 b[4]; };
        auto load_g = [&](RowFrag& f, int g) {          // g = kx*4 + ks
            const int kx = g >> 2, ks = g & 3;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int s = 0; s < NCO; ++s) f.a[ky][s] = *(const uint4*)(wl + (((ky * 3 + kx) * NKS + ks) * NCO + s) * 1024);
            }
            const char* p0 = tb + boff[kx * 4 + ks];    // row index is an immediate of the ds_read
#pragma unroll
            for (int r = 0; r < 4; ++r) f.b[r] = *(const uint4*)(p0 + r * (P_LW * 128));
        };
        auto mma_g = [&](const RowFrag& f) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int s = 0; s < NCO; ++s) {
                    Mma<half_t>::run(acc[s][0], f.a[ky][s], f.b[ky]);
                    Mma<half_t>::run(acc[s][1], f.a[ky][s], f.b[ky + 1]);
                }
            }
        };
        auto groups = [&](bool loads) {
#pragma unroll
            for (int q = 0; q < 6 * NCO; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                      // 1 MFMA
                if (loads && q < 3 * NCO + 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // 1 DS read of the next group
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        RowFrag f0, f1;
        load_g(f0, 0);
        static_for<0, 6>([&](auto I) {
            constexpr int i = decltype(I)::value;
            load_g(f1, 2 * i + 1);
            mma_g(f0);
            groups(true);
            if constexpr (i < 5) load_g(f0, 2 * i + 2);
            mma_g(f1);
            groups(i < 5);
        });
        // no second barrier: the epilogue works from registers, and tile t's buffer is only overwritten by the DMA of
        // tile t+2, issued after barrier A of tile t+1, which every MFMA wave reaches after this MFMA phase
        // ---- epilogue straight from the accumulators (the tile buffer is not reused: barrier B only orders the DMA) ----
#if defined(DEMFI_TRACE) && defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
        for (int s = 0; s < NCO; ++s) { asm volatile("" ::"v"(acc[s][0])); asm volatile("" ::"v"(acc[s][1])); }
        TRACE_STAMP(wave, trk, 2);
#endif
        if constexpr (RES) {
            // Retire the residual loads HERE (they landed during the MFMA phase): otherwise the compiler's in-order
            // vmcnt bookkeeping makes the later units wait for this epilogue's own stores to be acknowledged.
#pragma unroll
            for (int s = 0; s < NCO; ++s) {
#pragma unroll
                for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(rreg[s][q >> 1][q & 1]));
            }
        }
#pragma unroll
        for (int s = 0; s < NCO; ++s) {
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2) {
                // cout_perm: MFMA row (quad g, half hi, j) holds channel (g>>1)*16 + hi*8 + (g&1)*4 + j, so quads 2*m2 and 2*m2+1
                // of this lane are the 8 consecutive channels 16*m2 + 8*hi .. +7 of its pixel -- no cross-lane exchange (round 1
                // used a v_permlane32_swap per accumulator pair here); bias_lds is in MFMA-row order
                const f4_t b0 = *(const f4_t*)(bias_lds + s * 32 + (2 * m2) * 8 + hi * 4);
                const f4_t b1 = *(const f4_t*)(bias_lds + s * 32 + (2 * m2 + 1) * 8 + hi * 4);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] = acc[s][p][(2 * m2) * 4 + j] + b0[j];
                        v[4 + j] = acc[s][p][(2 * m2 + 1) * 4 + j] + b1[j];
                    }
                    if constexpr (RES) {
                        const h8_t r = __builtin_bit_cast(h8_t, rreg[s][p][m2]);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] += (float)r[j];
                    }
                    h8_t o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = (half_t)v[j];
                    o = __builtin_elementwise_max(o, act_floor8);   // ReLU or identity (floor -inf), branch-free; rounding is monotonic: max after the conversion gives the same value
                    const int oy = oy0 + wave * 2 + p, oxx = ox0 + lx;
                    if (oy < H && oxx < W)
                        *gp<u4_t>(dstp + bimg * d_sb + oy * d_sy + oxx * d_sx + ch0 + s * 32 + m2 * 16 + hi * 8) = __builtin_bit_cast(u4_t, o);
                }
            }
        }
        TRACE_STAMP(wave, trk, 3);
    }
}

template <int NCO>
int launch_persist(const demfi_conv* h, const demfi_conv* dev, hipStream_t st)
{
    const size_t lds = 9 * 4 * NCO * 1024 + 2 * P_TILE_BYTES + 1024;      // weights + 2 tiles + bias
    DEMFI_LDS_ATTR((conv3x3_c64_persist_kernel<NCO, true>));
    DEMFI_LDS_ATTR((conv3x3_c64_persist_kernel<NCO, false>));
    const int total = ((h->W + TW - 1) / TW) * ((h->H + TH - 1) / TH) * h->batch;
    const int grid = total >= 256 ? 256 : total;
    if (h->segs[h->sub_seg[0]].res.ptr != nullptr)
        hipLaunchKernelGGL((conv3x3_c64_persist_kernel<NCO, true>), dim3(grid), dim3(NT + 64 * P_NDMA), lds, st, dev);
    else
        hipLaunchKernelGGL((conv3x3_c64_persist_kernel<NCO, false>), dim3(grid), dim3(NT + 64 * P_NDMA), lds, st, dev);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}


// ======================================================================================================
// STAGED-STORE variant of the 64 -> 64 kernel (NCO == 2).
// What the in-kernel phase trace says about the 4-wave kernel above (profiles/r03_phase_trace.md; cycles at the ~1.7 GHz the part
// sustains under this load): a tile period of 7 700 cycles = MFMA phase 5 200 (144 MFMAs = 4 608 pipe cycles) + epilogue 2 200 +
// barrier ~300, and the epilogue is the CU's store path: 32 KiB per tile at ~16 B/clk/CU (tools/microbench/store_path_per_cu.hip)
// = 2 048 cycles during which the matrix pipe of all four SIMDs idles.  tools/microbench/overlap_matrix.hip says which waves may
// share a SIMD: an OLDER k-loop-like MFMA wave is not slowed by a YOUNGER wave that issues global stores (687 vs 683 cycles per
// 16 MFMAs, stores at full rate), while an older storing wave starves a younger MFMA wave completely -- so the roles are fixed by
// age: MFMA waves 0-3 never touch global memory for their outputs; after the MFMA phase they apply bias / residual / ReLU in
// registers, ds_write the packed fp16 tile into the tile buffer they have just finished reading (barrier B) and go on to the next
// tile.  The four helper waves (4-7, one per SIMD, younger) read the staged tile back 8 lanes per pixel, issue the global stores
// as whole 128-byte lines while the next tile is on the matrix cores, and then issue the LDS-DMA of tile k+2 into the same buffer
// (helper w drains exactly the 1-KiB chunks its own DMA instructions overwrite, so nothing else has to be synchronised).
// Round 2 built this once on the 2-DMA-wave kernel and measured nothing (profiles/r02_notes.md); the trace shows why: there the
// helper path (stores, then 3 300 cycles of DMA issue starved by the MFMA waves, then the landing) was as long as the period.
// ======================================================================================================
// Streaming (nt) hint of the staged-store kernel on the helper waves' output stores -- whole 128-byte lines of tensors of hundreds of MB
// that the next launch re-reads from HBM anyway; without the hint the written lines compete with the input tiles for the L2s and the
// Infinity Cache: residual launches -1.5..-2 %, the window -0.6 ms (profiles/r04_notes.md section 11).  Measured negative there: nt
// residual loads (+15 % on the residual launches), nt tile DMA.  The same hint on the 16-byte-per-lane stores of the MFMA waves of the
// GRU / narrow / streamed-weight kernels is 1.8x / 1.1x / 1.02x SLOWER (partial lines).
constexpr int SG_NH = 4;                                         // helper waves
constexpr int SG_NT = NT + 64 * SG_NH;
template <bool RES, bool TANH = false>   // TANH: tanh after the residual add (Refine_Module.dec3's feature halves, DeMFInet.py:86-87) instead of ReLU / identity
__global__ __launch_bounds__(SG_NT, 1) void conv3x3_c64_stg_kernel(const demfi_conv* __restrict__ d)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NTAPS = 9, NKS = 4, NCO = 2;
    constexpr int WBYTES = NTAPS * NKS * NCO * 1024;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = d->H, W = d->W;
    const int tiles_x = (W + TW - 1) / TW;
    const int tiles_y = (H + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y;
    const int total = tiles_img * d->batch;
    char* const wlds = smem;
    char* const tbuf = smem + WBYTES;
    int t_first, t_end, t_step;
    XCD_TILE_STRIDE(total, t_first, t_end, t_step);
    if (t_first >= t_end) return;
    auto tile_coords = [&](int t, int& bimg, int& oy0, int& ox0) {
        bimg = t / tiles_img;
        const int rem = t - bimg * tiles_img;
        const int ty = rem / tiles_x;
        oy0 = ty * TH;
        ox0 = (rem - ty * tiles_x) * TW;
    };
    const demfi_seg& sg0 = d->segs[d->sub_seg[0]];
    const int64_t d_sx = sg0.dst.sx, d_sy = sg0.dst.sy, d_sb = sg0.dst.sb;
    [[maybe_unused]] int trk = 0;

    if (wave >= 4) {
        // ================= helper waves: tile DMA + the global stores of the staged outputs ==========================
        const int dw = wave - 4;
        constexpr int NIW = (P_NI + SG_NH - 1) / SG_NH;          // DMA instructions per helper (11; the last one may not exist)
        const demfi_piece& pc = d->pieces[0];
        const char* const src = (const char*)pc.v.ptr;
        const int64_t sx = pc.v.sx * 2, sy = pc.v.sy * 2, sb = pc.v.sb * 2;
        const char* const zeros = (const char*)d->zero_page;
        unsigned off[NIW];                                       // unsigned: uniform base + zero-extended 32-bit lane offset = the saddr form (no VALU per instruction)
        int lyx[NIW];
#pragma unroll
        for (int k = 0; k < NIW; ++k) {
            const int i = dw + SG_NH * k;
            const int px = i * 8 + (lane >> 3);
            const int pxc = min(px, P_NP - 1);                   // lanes past the tile (last instruction only) re-read its last pixel: never consumed
            const int ly = pxc / P_LW;
            const int lxx = pxc - ly * P_LW;
            const int v = (lane & 7) ^ ((lxx >> 1) & 7);
            off[k] = (unsigned)((ly + 1) * sy + (lxx + 1) * sx) + v * 16;      // relative to pixel (-2,-2) of the tile: never negative
            lyx[k] = (i < P_NI && px < P_NP) ? (ly | (lxx << 8)) : 0xffff;
        }
        auto issue_tile = [&](int t, int buf) {
            int bimg, oy0, ox0;
            tile_coords(t, bimg, oy0, ox0);
            const char* base = src + (int64_t)bimg * sb + (int64_t)(oy0 - 2) * sy + (int64_t)(ox0 - 2) * sx;
            char* dst = tbuf + buf * P_TILE_BYTES;
            const bool interior = oy0 >= 1 && oy0 + TH + 1 <= H && ox0 >= 1 && ox0 + TW + 1 <= W;
            if (interior) {                                      // uniform base + precomputed 32-bit lane offset: ~2 VALU per instruction
#pragma unroll
                for (int k = 0; k < NIW; ++k) {
                    const int i = dw + SG_NH * k;
                    if (i >= P_NI) continue;                     // wave-uniform
                    const char* g = base + off[k];
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                     (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
                }
            } else {
#pragma unroll
                for (int k = 0; k < NIW; ++k) {
                    const int i = dw + SG_NH * k;
                    if (i >= P_NI) continue;
                    const int iy = oy0 - 1 + (lyx[k] & 255), ix = ox0 - 1 + (lyx[k] >> 8);
                    const char* g = (lyx[k] != 0xffff && iy >= 0 && iy < H && ix >= 0 && ix < W) ? base + off[k] : zeros;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                     (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
                }
            }
        };
        half_t* const dstp = (half_t*)sg0.dst.ptr + d->oct_ch[0];
        constexpr int NCH = 32 / SG_NH;                          // 1-KiB chunks (8 pixels x 128 B) of the 32-KiB staging per helper
        u4_t stage[NCH];
        auto stage_read = [&](int b) {
            const char* sbp = tbuf + b * P_TILE_BYTES + lane * 16;
#pragma unroll
            for (int k = 0; k < NCH; ++k) stage[k] = *(const u4_t*)(sbp + (dw + SG_NH * k) * 1024);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // in registers before this wave's DMA may overwrite the chunks
        };
        // byte offset of this lane's 16-byte piece of chunk k relative to the tile's first output pixel (loop-invariant)
        unsigned doff[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int j = dw + SG_NH * k;                        // chunk j: pixels 8j .. 8j+7 of the 8x32 tile; lane -> (pixel, physical slot)
            const int oxl = (j & 3) * 8 + (lane >> 3);
            const int q = (lane & 7) ^ ((oxl >> 1) & 7);         // logical 16-byte slot = channels 8q .. 8q+7
            doff[k] = (unsigned)(((j >> 2) * d_sy + oxl * d_sx + q * 8) * 2);
        }
        auto stage_store = [&](int bimg, int oy0, int ox0) {
            char* const obase = (char*)(dstp + bimg * d_sb + oy0 * d_sy + ox0 * d_sx);      // wave-uniform
            if (oy0 + TH <= H && ox0 + TW <= W) {
#pragma unroll
                for (int k = 0; k < NCH; ++k) __builtin_nontemporal_store(stage[k], gp<u4_t>(obase + doff[k]));
            } else {
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const int j = dw + SG_NH * k;
                    if (oy0 + (j >> 2) < H && ox0 + (j & 3) * 8 + (lane >> 3) < W) *gp<u4_t>(obase + doff[k]) = stage[k];
                }
            }
        };
        const uint4* wsrc = (const uint4*)d->wpack;
        for (int i = dw; i < NTAPS * NKS * NCO; i += SG_NH)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + i * 64 + lane),
                                             (__attribute__((address_space(3))) void*)(wlds + i * 1024), 16, 0, 0);
        issue_tile(t_first, 0);
        int buf = 0;
        int pb = 0, py = 0, px = 0;
        bool have_prev = false;
        for (int t = t_first; t < t_end; t += t_step, buf ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // tile t has landed (and this wave's stores of tile t-2 are out)
            TRACE_STAMP(wave, trk, 0);
            asm volatile("s_barrier" ::: "memory");             // A: tile t to the MFMA waves; their outputs of tile t-1 are staged in buffer buf^1
            TRACE_STAMP(wave, trk, 1);
            // stores first: the vmcnt(0) in front of the next barrier A then waits for the tile loads issued LAST, not for the
            // acknowledgements of stores issued late in the phase
            if (have_prev) { stage_read(buf ^ 1); stage_store(pb, py, px); }
            if (t + t_step < t_end) issue_tile(t + t_step, buf ^ 1);
            TRACE_STAMP(wave, trk, 2);
            tile_coords(t, pb, py, px);
            have_prev = true;
            asm volatile("s_barrier" ::: "memory");             // B: the MFMA waves have finished reading buffer buf and may stage into it
            ++trk;
        }
        asm volatile("s_barrier" ::: "memory");                 // F: the last tile is staged (in buffer buf^1: buf was toggled on exit)
        stage_read(buf ^ 1);
        stage_store(pb, py, px);
        return;
    }

    // ================= MFMA waves ============================================================================
    const int hi = lane >> 5;
    const int lx = lane & 31;
    const half_t* const resp = (const half_t*)sg0.res.ptr;
    const int64_t r_sx = sg0.res.sx, r_sy = sg0.res.sy, r_sb = sg0.res.sb;
    const float act_floor = sg0.act == DEMFI_ACT_RELU ? 0.0f : -__builtin_huge_valf();
    h8_t act_floor8;
#pragma unroll
    for (int j = 0; j < 8; ++j) act_floor8[j] = (half_t)act_floor;
    const int ch0 = d->oct_ch[0];
    // bias of this lane's 32 accumulator rows (MFMA-row order: element 4g + j = quad g, half hi, j), in registers for the whole
    // launch and fed to the FIRST MFMA of every accumulator as its C operand: the accumulation starts at the bias, so the
    // epilogue has no bias adds at all (the 4-wave kernel re-reads the bias from LDS per epilogue unit: 8 dependent LDS round
    // trips, ~700 cycles per tile in the phase trace).  fp32 summation order differs from "sum, then + bias" by one rounding.
    f16x_t bias16[NCO];
#pragma unroll
    for (int s = 0; s < NCO; ++s) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f4_t bq = *gcp<f4_t>(d->bias + s * 32 + g * 8 + hi * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) bias16[s][g * 4 + j] = bq[j];
        }
    }
    int boff[12];
#pragma unroll
    for (int g = 0; g < 12; ++g) {
        const int col = lx + (g >> 2);
        boff[g] = col * 128 + ((((g & 3) * 2 + hi) ^ ((col >> 1) & 7)) << 4);
    }
    const char* const wl = wlds + lane * 16;
    // staging slot of this lane's (s, m2) piece: pixel record (row, lx) of a 32-pixel-per-row image, 16-byte slot
    // q = 4s + 2m2 + hi XOR-swizzled by the column like the input tiles (conflict-free ds_write_b128 groups)
    int soff[NCO][2];
#pragma unroll
    for (int s = 0; s < NCO; ++s) {
#pragma unroll
        for (int m2 = 0; m2 < 2; ++m2) soff[s][m2] = lx * 128 + (((s * 4 + m2 * 2 + hi) ^ ((lx >> 1) & 7)) << 4);
    }
    // Residual: the tile's own, issued at the head of the tile (before barrier A).  Issued in the middle of the MFMA phase, or a tile
    // ahead into a second register set, it measured no better (profiles/r04_notes.md).  The tile loop is unrolled by two so that the
    // tile buffer index is static.
    using ResRegs = u4_t[NCO][2][2];
    auto tile_body = [&](const int t, const int buf, ResRegs& rreg) {
        int bimg, oy0, ox0;
        tile_coords(t, bimg, oy0, ox0);
        if constexpr (RES) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int oy = min(oy0 + wave * 2 + p, H - 1), oxx = min(ox0 + lx, W - 1);
                const half_t* rp = resp + bimg * r_sb + oy * r_sy + oxx * r_sx + ch0 + hi * 8;
#pragma unroll
                for (int s = 0; s < NCO; ++s) {
#pragma unroll
                    for (int m2 = 0; m2 < 2; ++m2) rreg[s][p][m2] = *gcp<u4_t>(rp + s * 32 + m2 * 16);
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the staged outputs of the previous tile are in LDS
        TRACE_STAMP(wave, trk, 0);
        asm volatile("s_barrier" ::: "memory");                 // A
        TRACE_STAMP(wave, trk, 1);
        f16x_t acc[NCO][2];
        char* const tbase = tbuf + buf * P_TILE_BYTES;
        const char* tb = tbase + (wave * 2) * (P_LW * 128);
        {
            struct RowFrag { uint4 a[3][NCO]; uint4 b[4]; };
            auto load_g = [&](RowFrag& f, int g) {              // g = kx*4 + ks
                const int kx = g >> 2, ks = g & 3;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                    for (int s = 0; s < NCO; ++s) f.a[ky][s] = *(const uint4*)(wl + (((ky * 3 + kx) * NKS + ks) * NCO + s) * 1024);
                }
                const char* p0 = tb + boff[kx * 4 + ks];
#pragma unroll
                for (int r = 0; r < 4; ++r) f.b[r] = *(const uint4*)(p0 + r * (P_LW * 128));
            };
            auto mma_g = [&](const RowFrag& f, auto FIRST) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                    for (int s = 0; s < NCO; ++s) {
                        if (decltype(FIRST)::value && ky == 0) {
                            Mma<half_t>::initc(acc[s][0], f.a[ky][s], f.b[ky], bias16[s]);
                            Mma<half_t>::initc(acc[s][1], f.a[ky][s], f.b[ky + 1], bias16[s]);
                        } else {
                            Mma<half_t>::run(acc[s][0], f.a[ky][s], f.b[ky]);
                            Mma<half_t>::run(acc[s][1], f.a[ky][s], f.b[ky + 1]);
                        }
                    }
                }
            };
            auto groups = [&](bool loads) {
#pragma unroll
                for (int q = 0; q < 6 * NCO; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (loads && q < 3 * NCO + 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            RowFrag f0, f1;
            load_g(f0, 0);
            static_for<0, 6>([&](auto I) {
                constexpr int i = decltype(I)::value;
                load_g(f1, 2 * i + 1);
                mma_g(f0, std::integral_constant<bool, i == 0>{});
                groups(true);
                if constexpr (i < 5) load_g(f0, 2 * i + 2);
                mma_g(f1, std::false_type{});
                groups(i < 5);
            });
        }
#if defined(DEMFI_TRACE) && defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
        for (int s = 0; s < NCO; ++s) { asm volatile("" ::"v"(acc[s][0])); asm volatile("" ::"v"(acc[s][1])); }
        TRACE_STAMP(wave, trk, 2);
#endif
        // B: every MFMA wave has consumed its reads of this tile buffer -> its first 32 KiB become the staging image of the outputs
        asm volatile("s_barrier" ::: "memory");
        TRACE_STAMP(wave, trk, 4);
        if constexpr (RES) {
#pragma unroll
            for (int s = 0; s < NCO; ++s) {
#pragma unroll
                for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(rreg[s][q >> 1][q & 1]));
            }
        }
#pragma unroll
        for (int s = 0; s < NCO; ++s) {
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2) {
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] = acc[s][p][(2 * m2) * 4 + j];
                        v[4 + j] = acc[s][p][(2 * m2 + 1) * 4 + j];
                    }
                    if constexpr (RES) {
                        // + residual: v_fma_mix_f32 (fp16 operand * 1.0 + fp32) = the conversion and the add in one instruction, same rounding
                        const u4_t r = rreg[s][p][m2];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            v[2 * q] = res_mix_lo(r[q], v[2 * q]);
                            v[2 * q + 1] = res_mix_hi(r[q], v[2 * q + 1]);
                        }
                    }
                    if constexpr (TANH) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = fast_tanh(v[j]);
                    }
                    h8_t o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = (half_t)v[j];
                    if constexpr (!TANH) o = __builtin_elementwise_max(o, act_floor8);
                    *(u4_t*)(tbase + (wave * 2 + p) * 4096 + soff[s][m2]) = __builtin_bit_cast(u4_t, o);
                }
            }
        }
        TRACE_STAMP(wave, trk, 3);
        ++trk;
    };
    ResRegs r_even, r_odd;
    for (int t = t_first; t < t_end;) {
        tile_body(t, 0, r_even);
        t += t_step;
        if (t >= t_end) break;
        tile_body(t, 1, r_odd);
        t += t_step;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the last tile is staged
    asm volatile("s_barrier" ::: "memory");                     // F
}

static int launch_stg(const demfi_conv* h, const demfi_conv* dev, hipStream_t st)
{
    const size_t lds = 9 * 4 * 2 * 1024 + 2 * P_TILE_BYTES + 1024;
    DEMFI_LDS_ATTR((conv3x3_c64_stg_kernel<true, false>));
    DEMFI_LDS_ATTR((conv3x3_c64_stg_kernel<false, false>));
    DEMFI_LDS_ATTR((conv3x3_c64_stg_kernel<true, true>));
    DEMFI_LDS_ATTR((conv3x3_c64_stg_kernel<false, true>));
    const int total = ((h->W + TW - 1) / TW) * ((h->H + TH - 1) / TH) * h->batch;
    const int grid = total >= 256 ? 256 : total;
    const demfi_seg& sg = h->segs[h->sub_seg[0]];
    const bool res = sg.res.ptr != nullptr, th = sg.act == DEMFI_ACT_TANH;
    if (res && th)  hipLaunchKernelGGL((conv3x3_c64_stg_kernel<true, true>), dim3(grid), dim3(SG_NT), lds, st, dev);
    else if (res)   hipLaunchKernelGGL((conv3x3_c64_stg_kernel<true, false>), dim3(grid), dim3(SG_NT), lds, st, dev);
    else if (th)    hipLaunchKernelGGL((conv3x3_c64_stg_kernel<false, true>), dim3(grid), dim3(SG_NT), lds, st, dev);
    else            hipLaunchKernelGGL((conv3x3_c64_stg_kernel<false, false>), dim3(grid), dim3(SG_NT), lds, st, dev);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}


}  // namespace

int demfi_c64_trace_collect(unsigned long long* acc) { return TRACE_DRAIN(acc, true); }

bool demfi_c64_strides_ok(const demfi_conv* h)
{
    const demfi_view& s = h->pieces[0].v;
    if (s.sy < 0 || s.sx < 0 || s.sy >= P_OFF_LIMIT || s.sx >= P_OFF_LIMIT) return false;
    if ((s.sy * P_LH + s.sx * P_LW) * 2 + 128 >= P_OFF_LIMIT) return false;
    if (h->nco == 2) {
        const demfi_view& d = h->segs[h->sub_seg[0]].dst;
        if (d.sy < 0 || d.sx < 0 || d.sy >= P_OFF_LIMIT || d.sx >= P_OFF_LIMIT) return false;
        if ((d.sy * TH + d.sx * TW) * 2 + 128 >= P_OFF_LIMIT) return false;
    }
    return true;
}

int demfi_c64_launch(const demfi_conv* h, const demfi_conv* dev, hipStream_t st)
{
    return h->nco == 2 ? launch_stg(h, dev, st) : launch_persist<1>(h, dev, st);
}
