/*
 * demfi_hip.h -- C ABI of libdemfi_hip.so: the MI355X (gfx950) kernels of the DeMFI-Net_rb forward path.
 *
 * The upstream reference (JihyongOh/DeMFI) has NO native / FFI boundary: its hot path is the Python
 * nn.Module DeMFInet.forward (DeMFInet.py:46-179) calling stock ATen ops.  This header therefore defines
 * the boundary a host binds instead of those ATen call sites.  Each entry
 * point names the reference lines it replaces.  Rules of the ABI:
 *   - extern "C", plain pointers + sizes, no torch / C++ types;
 *   - every function returns 0 on success, a negative demfi_status otherwise, never throws;
 *     demfi_last_error() returns a thread-local message for the last failure;
 *   - the caller owns every buffer (device pointers unless stated otherwise); nothing is allocated
 *     behind the caller's back except the hipGraph objects of demfi_graph_*;
 *   - all launches go to the hipStream_t the caller passes (as void*), nothing synchronises.
 *
 * Data layouts
 *   "fat"  tensors : NHWC, element type = the path dtype (DEMFI_F16 or DEMFI_F32), described by strides;
 *   "thin" tensors : planar fp32 (the NCHW tensors the PyTorch host hands over / gets back:
 *                    flows, occlusion logits, 3-channel frames).
 * Both are described by demfi_view (element strides, so channel slices of wider buffers are views).
 */
#ifndef DEMFI_HIP_H
#define DEMFI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEMFI_ABI_VERSION 8

enum demfi_dtype { DEMFI_F16 = 0, DEMFI_F32 = 1 };

enum demfi_status {
    DEMFI_OK = 0,
    DEMFI_ERR_ARG = -1,      /* malformed descriptor / unsupported shape */
    DEMFI_ERR_HIP = -2,      /* a HIP runtime call failed (message holds hipGetErrorString) */
    DEMFI_ERR_NODEV = -3     /* no gfx950 device visible */
};

/* Colour conversion of the Y4M stream edge (demfi_yuv420_to_bgr / demfi_bgr_to_yuv420 below). */
enum demfi_yuv_matrix { DEMFI_BT601 = 0, DEMFI_BT709 = 1 };
enum demfi_chroma_siting { DEMFI_420JPEG = 0, DEMFI_420MPEG2 = 1 };   /* chroma centred / co-sited horizontally, centred vertically */
/* Chroma layouts of demfi_yuvl_to_bgr and its kin below (4:2:0 = 0 is served by the demfi_yuv420 functions). */
enum demfi_yuv_layout { DEMFI_YUV_420 = 0, DEMFI_YUV_422 = 1, DEMFI_YUV_444 = 2, DEMFI_YUV_MONO = 3 };

enum demfi_act { DEMFI_ACT_NONE = 0, DEMFI_ACT_RELU = 1, DEMFI_ACT_TANH = 2, DEMFI_ACT_SIGMOID = 3 };

/* Output modes of a convolution segment (v = conv + bias):
 *   STORE : dst = act(v + res)                                  (res optional)
 *   MUL   : dst = sigmoid(v) * res                              (GRU reset gate: r*h, DeMFInet.py:846-847)
 *   GRU   : dst = (1 - aux) * res + aux * tanh(v)               (GRU update, aux = z, res = h; 847-848)      */
enum demfi_mode { DEMFI_MODE_STORE = 0, DEMFI_MODE_MUL = 1, DEMFI_MODE_GRU = 2 };

/* A strided 4-D view.  Strides are in ELEMENTS of the view's own type.  ptr already points at the
 * first channel of the slice.  A NULL ptr means "absent" (or "zeros" for an input piece). */
typedef struct demfi_view {
    void*   ptr;
    int64_t sx;        /* x -> x+1        */
    int64_t sy;        /* y -> y+1        */
    int64_t sc;        /* channel -> +1   (1 for NHWC fat views) */
    int64_t sb;        /* batch image -> +1 */
    int32_t is_f32;    /* element type of ptr: 1 = fp32, 0 = fp16 */
    int32_t _pad;
} demfi_view;

/* One piece of a convolution's logical input-channel concatenation (replaces torch.cat). */
typedef struct demfi_piece {
    demfi_view v;
    int32_t nch;       /* channels taken from v (v.ptr == NULL: nch zero channels)               */
    int32_t lds_ch;    /* first channel of this piece inside its chunk                           */
    int32_t up_shift;  /* 1: the piece is read through a nearest-neighbour x2 upsample
                          (UNet decoder, DeMFInet.py:592,597,601), 0: direct                      */
    int32_t fat;       /* 1: NHWC view of the path dtype, nch*elt % 16 == 0, 16-byte vector loads;
                          0: generic element-wise loads (any strides, fp16 or fp32)               */
} demfi_piece;

#define DEMFI_MAX_PIECES 48
#define DEMFI_MAX_CHUNKS 40
#define DEMFI_MAX_SEGS    8
#define DEMFI_MAX_OCTS   32     /* cout_pad / 8, cout_pad <= 256 */

/* Input channels are consumed in chunks staged through LDS; a chunk is <= rec_bytes of channel data
 * per pixel (a multiple of one MFMA k-step = 32 bytes = 16 fp16 or 8 fp32 channels). */
typedef struct demfi_chunk {
    int32_t first_piece;
    int32_t n_pieces;
    int32_t nks;        /* k-steps in this chunk (32 bytes of channel data each)                  */
    int32_t _pad;
    int64_t w_off;      /* offset of this chunk's packed weights, in 16-byte units, cout block 0  */
} demfi_chunk;

typedef struct demfi_seg {
    demfi_view dst;
    demfi_view res;     /* optional */
    demfi_view aux;     /* optional */
    int32_t act;        /* demfi_act, STORE mode only */
    int32_t mode;       /* demfi_mode */
    int32_t scale;      /* 1, or 2 = PixelShuffle(2) store (DeMFInet.py:229): dst pixel (2y+dy, 2x+dx) */
    int32_t dy, dx;
    int32_t _pad;
} demfi_seg;

/* Implicit-GEMM convolution on the matrix cores (replaces every nn.Conv2d / nn.Conv3d(1,k,k) call site
 * of DeMFInet.py, SURVEY.md section 2.2 C1/C6-C12, together with the torch.cat / PixelShuffle /
 * UpsamplingNearest2d / activation / residual ops around them). */
typedef struct demfi_conv {
    int32_t dtype;              /* path dtype (type of fat views and packed weights)               */
    int32_t H, W;               /* OUTPUT height / width                                           */
    int32_t inH, inW;           /* input height / width as the convolution sees it (after up_shift) */
    int32_t kh, kw;
    int32_t stride;             /* 1 or 2                                                          */
    int32_t pad_y, pad_x;
    int32_t batch;              /* images sharing weights (Conv3d depth of D1 / the two FAC-FB frames) */
    int32_t cout_pad;           /* packed output channels, multiple of 32                          */
    int32_t nco;                /* 32-cout subtiles per workgroup (1..5), cout_pad % (32*nco) == 0 */
    int32_t rec_bytes;          /* LDS bytes of channel data per pixel per chunk (32/64/128)        */
    int32_t n_chunks;
    int32_t n_pieces;
    int32_t n_segs;
    int32_t cout_perm;          /* 1: the packed weights / bias are in the cout order of the persistent kernels (64-channel
                                   3x3, narrow with an NHWC destination, SepConvGRU; set by demfi_conv_build / the context for the
                                   layers those kernels own: within a
                                   32-cout subtile MFMA row r holds channel (r>>4)*16 + ((r>>2)&1)*8 + ((r>>3)&1)*4 + (r&3), so a
                                   lane's two accumulator quads are 8 consecutive channels); demfi_conv2d refuses such a
                                   descriptor when that kernel cannot take it, and an eligible one without the flag */
    int64_t w_blk_stride;       /* packed-weight stride between cout blocks, 16-byte units         */
    const void*  wpack;         /* packed weights, see demfi_pack_conv_weights                     */
    const float* bias;          /* [cout_pad] fp32 in packed cout order                            */
    const void*  zero_page;     /* >= 16 bytes of zeros in device memory (source of padding pixels for the
                                   LDS-DMA tile loads of the persistent 3x3 path); NULL disables that path */
    demfi_chunk chunks[DEMFI_MAX_CHUNKS];
    demfi_piece pieces[DEMFI_MAX_PIECES];
    demfi_seg   segs[DEMFI_MAX_SEGS];
    /* packed cout octet o = couts [8o, 8o+8): which segment, first channel inside the segment's views,
     * number of valid channels (0 = padding octet, nothing stored). */
    int32_t oct_seg[DEMFI_MAX_OCTS];
    int32_t oct_n[DEMFI_MAX_OCTS];
    int32_t oct_ch[DEMFI_MAX_OCTS];
    /* packed 32-cout subtile s: segment index when its 4 octets are one aligned run of 32 channels of an
     * NHWC view of the path dtype (dst, and res/aux when present) -> coalesced LDS-staged epilogue;
     * -1 -> per-octet direct epilogue (thin / planar / ragged outputs). */
    int32_t sub_seg[DEMFI_MAX_OCTS / 4];
    /* magic = ceil(2^32 / LW), LW = (32-1)*stride + kw: exact px / LW for px < 2^16 (filled by host) */
    uint32_t lw_magic;
    int32_t  u8_iter;           /* recursion index this descriptor belongs to (compared with demfi_u8_sink.iter) */
    /* optional uint8 sink (planar fp32 3-channel segments on the thin epilogue only, i.e. the frame-producing last layer
     * Dec_last2_2): device pointer to a demfi_u8_sink record read AT RUN TIME, so a captured hipGraph serves every
     * destination.  NULL = none. */
    const struct demfi_u8_sink* u8_sink;
    /* optional PACKED COPY of thin outputs (ABI v6; thin epilogue of the narrow persistent kernel only): besides its planar fp32
     * destination, octet o (o < 4) with pack_oct_ch[o] >= 0 also writes its channels, converted to the path dtype, as channels
     * pack_oct_ch[o] .. of the NHWC record `pack` (a lane's group of up to 4 channels is one 8-byte store; the unused channels of
     * the group are written as zeros) -- the record the next convolution stages with vector loads, i.e. what a
     * demfi_pack_planes launch over these planes would have produced (replaces the per-recursion pack of the flow / occlusion
     * deltas, DeMFInet.py:130-137 -> 800-812).  pack.ptr == NULL: none.  pack_oct_ch[o] must be a multiple of 4. */
    demfi_view pack;
    int32_t pack_oct_ch[4];
} demfi_conv;

/* uint8 egress fused into the last store: when `iter` equals the descriptor's u8_iter, segment
 * s of the convolution additionally writes crop + denorm255_np + uint8 truncation (utils.py:718-721, main.py:1165-1178:
 * float64 arithmetic) of its 3 channels to frame[s] as [h, w, 3] bytes (NULL = that frame is not wanted) and skips the
 * fp32 store of that segment. */
#define DEMFI_U8_SINK_STRIDE 256   /* bytes between the sink records of consecutive batch images (the per-t contexts' "sink" buffers) */
typedef struct demfi_u8_sink {
    uint8_t* frame[DEMFI_MAX_SEGS];
    int32_t  h, w;              /* crop (top-left h x w of the padded H x W) */
    int32_t  iter;              /* recursion index whose output is the final one (num_update - 1); -1 disables */
    int32_t  _pad;
} demfi_u8_sink;

/* ---- library / device ------------------------------------------------------------------------- */
int         demfi_abi_version(void);
const char* demfi_last_error(void);
/* Fills name[len] with the device's gcnArchName; returns DEMFI_ERR_NODEV without a GPU. */
int         demfi_device_info(char* name, int len, int* n_cu, int64_t* hbm_bytes);

/* ---- weight repack (host memory in, host memory out) -------------------------------------------
 * w_oihw : fp32 [cout, cin, kh, kw] (the state_dict tensor; Conv3d weights are passed squeezed).
 * cin_map[n_k]   : original input channel feeding packed k index (chunk-concatenated order, every
 *                  chunk padded to its k-step multiple), -1 = zero.
 * chunk_nks[n_chunks] : k-steps per chunk (sum * chans_per_kstep == n_k).
 * cout_map[cout_pad] : original output channel of packed cout, -1 = zero.
 * Packed order: [cout_blk][chunk][tap = ky*kw+kx][kstep][subtile < nco][lane < 64][16 bytes]; lane l of
 * a k-step holds, for cout = blk*32*nco + subtile*32 + (l & 31), the 8 fp16 (4 fp32) weights of packed
 * channels kstep*16 + 8*(l>>5) + j (kstep*8 + 4*(l>>5) + j) -- the A fragment of
 * v_mfma_f32_32x32x16_f16 (4 x v_mfma_f32_32x32x2_f32).
 * Returns the packed size in bytes through out_bytes (call with out == NULL to size the buffer). */
int demfi_pack_conv_weights(const float* w_oihw, int cout, int cin, int kh, int kw,
                            const int32_t* cin_map, int n_k, const int32_t* chunk_nks, int n_chunks,
                            const int32_t* cout_map, int cout_pad, int nco, int dtype,
                            void* out, int64_t* out_bytes);

/* LDS bytes one workgroup of demfi_conv2d needs for this descriptor (host-side helper). */
int64_t demfi_conv_lds_bytes(const demfi_conv* host_desc);

/* ---- kernels ----------------------------------------------------------------------------------- */
/* host_desc: descriptor in host memory (grid sizing / validation); dev_desc: the same bytes in device
 * memory (the kernel reads it through the scalar cache). */
int demfi_conv2d(const demfi_conv* host_desc, const demfi_conv* dev_desc, void* stream);

/* Fused residual block (ABI v7): y = x + conv2(relu(conv1(x))) in ONE launch -- ResBlock2D_3D / ResBlock2D (DeMFInet.py:524-563)
 * as the FAC-FB encoder (341-344), D1 (95-101: Conv3d(1,3,3) == batch 3) and D2 (158-160) use them.  h1 / h2: HOST descriptors of
 * the two 3x3 64 -> 64 fp16 convolutions exactly as demfi_conv_build makes them for demfi_conv2d (conv1: ReLU, no residual, writing
 * the intermediate; conv2: no activation, residual == conv1's input, reading the intermediate); the kernel takes the input view,
 * both packed weight sets / biases and conv2's destination from them (its arguments travel by value: no device descriptors) and
 * never touches the intermediate buffer: the intermediate lives in LDS (rounded to fp16 like the stored one, so conv1's half is
 * bit-identical to the two-launch form; conv2 accumulates onto bias + identity instead of adding the identity last: one fp32
 * rounding apart).  demfi_resblock_eligible: 1 when the pair is such a block (then demfi_resblock3x3_c64 == the two demfi_conv2d
 * launches), else 0. */
int demfi_resblock_eligible(const demfi_conv* h1, const demfi_conv* h2);
int demfi_resblock3x3_c64(const demfi_conv* h1, const demfi_conv* h2, void* stream);

/* SepConvGRU half-step with the update gate kept on chip (ABI v8; DeMFInet.py:838-857, horizontal 844-849, vertical 851-856):
 *     launch R  (demfi_gru_r)  : r * h = sigmoid(convr([h, x])) * h
 *     launch ZQ (demfi_gru_zq) : h' = (1 - z) h + z tanh(convq([r * h, x])),  z = sigmoid(convz([h, x]))
 * instead of the z | r and q launches of demfi_conv2d: z never goes to memory (handed from the z waves to the q waves through LDS,
 * rounded to fp16 as the stored z was), 896 instead of 1 152 bytes per pixel and half-step.  The arguments are HOST descriptors of
 * the plain 64-cout layers exactly as demfi_conv_build makes them for demfi_conv2d (1x5 or 5x1, fp16, two 64-channel NHWC pieces):
 *   hr: [h, x] -> MUL epilogue with res == h;   hz: [h, x] -> sigmoid, STORE into the z buffer (never touched by the fused launch);
 *   hq: [r*h, x] -> GRU epilogue with res == h, aux == hz's destination.
 * The kernel arguments travel by value (no device descriptors).  *_eligible: 1 when the descriptors are such layers (then the fused
 * launch equals the demfi_conv2d launches up to the summation order of the fp32 accumulators), else 0. */
int demfi_gru_r_eligible(const demfi_conv* hr);
int demfi_gru_r(const demfi_conv* hr, void* stream);
int demfi_gru_zq_eligible(const demfi_conv* hz, const demfi_conv* hq);
int demfi_gru_zq(const demfi_conv* hz, const demfi_conv* hq, void* stream);

/* pixel_reshuffle(cat(B0,B1,B-1,B2), 2) (DeMFInet.py:234-235, 290-316): x fp32 [3,4,H,W] (C,T order of the
 * module input, batch 1) -> fat NHWC [H/2, W/2, 48], channel = (frame*3 + c)*4 + ry*2 + rx. */
int demfi_space_to_depth(const float* x, void* out, int dtype, int H, int W, void* stream);

/* Reflect padding of the harness (utils.py:1360-1365): x [planes,h,w] -> out [planes,H,W], bottom/right. */
int demfi_reflect_pad(const float* x, float* out, int planes, int h, int w, int H, int W, void* stream);

/* torch.mean(x[:, :, 0:2], dim=2) (DeMFInet.py:178): x [3,4,H,W] -> out [3,H,W]. */
int demfi_overlay_mean(const float* x, float* out, int H, int W, void* stream);

/* CFR_flow_t_align (DeMFInet.py:606-622) = two forward splats (fwarp 625-671, sample_one 683-729) +
 * the linear combination / normalisation.  flow01, flow10: planar fp32 [2,H,W]; t: device pointer to
 * one fp32; acc: caller workspace of demfi_cfr_workspace_bytes(H, W) bytes (six int64 [H,W] planes + per-tile flags)
 * that MUST be all-zero on entry (allocate it zeroed once) and is left all-zero on exit; out: planar fp32 [4,H,W] =
 * (flow_t0, flow_t1).  The splat accumulates in 64-bit fixed point (2^-32 resolution) so the result
 * does not depend on the order of the adds (LDS atomics per target tile; global atomics only for sources displaced
 * by more than 32 px).  dbg_idx (optional, may be NULL): int32
 * [2 flows][4 corners][H*W] flat target index of every source pixel, -1 where masked off
 * (sample_one's ids / mask, DeMFInet.py:712-719) for the index-parity tests. */
int64_t demfi_cfr_workspace_bytes(int H, int W);
int demfi_cfr_reset(int64_t* acc, int H, int W, void* stream);      /* re-zero the workspace after an aborted launch */
int demfi_cfr_flow_align(const float* flow01, const float* flow10, const float* t, int H, int W,
                         int64_t* acc, float* out, int32_t* dbg_idx, void* stream);

/* Eq.(2): two backward warps (bwarp, DeMFInet.py:732-766) blended with the occlusion map
 * (DeMFInet.py:66-71, 90-93, 146-149):
 *   o0 = sigmoid(logit); out = ((1-t) o0 bwarp(A,fa) + t (1-o0) bwarp(B,fb)) / ((1-t) o0 + t (1-o0)).
 * A, B, out: views with C channels (fat NHWC of the path dtype, or thin planar fp32); a fat view whose pixel is
 * not a power-of-two number of 16-byte lanes, or more than 64 of them (1 KiB), is refused; fa, fb: planar
 * fp32 [2,H,W]; logit: planar fp32 [H,W]; t: device fp32.  occ_out (optional): sigmoid(logit) [H,W].
 * dbg_maps (optional): int32 [2 warps][3][H*W] = floor x index, floor y index, bit0-3 in-bounds of
 * (nw,ne,sw,se) | bit4 validity mask -- the integer maps of grid_sample for the index-parity tests. */
int demfi_warp_blend(const demfi_view* A, const float* fa, const demfi_view* B, const float* fb,
                     const float* logit, const float* t, const demfi_view* out, int C, int H, int W,
                     float* occ_out, int32_t* dbg_maps, void* stream);

/* The same for 3-channel planar frames (the PWB of the recursion, DeMFInet.py:140-149) with the packed copy the next layer
 * reads: pack8 = NHWC [H,W,8] of pack_dtype holding [out 0..2 | fa | fb | sigmoid(logit)] (Agg3's per-recursion planes,
 * DeMFInet.py:151-155) -- replaces a demfi_pack_planes launch. */
int demfi_warp_blend_pack(const demfi_view* A, const float* fa, const demfi_view* B, const float* fb,
                          const float* logit, const float* t, const demfi_view* out, int H, int W, float* occ_out,
                          void* pack8, int pack_dtype, void* stream);

/* ---- batched point-wise launches (ABI v5): the same op for the nb per-t contexts of one trunk set in ONE launch ----------------
 * The per-t buffers of a context set are laid out tensor-major (copy c of a buffer sits c * stride bytes behind copy 0), so a
 * batched launch takes the pointers of context 0 plus one BYTE stride per pointer (0 = a window-level buffer every context shares:
 * trunk features, flow_01 / flow_10).  Counterpart of the reference running its whole forward once per t (main.py:1121-1178):
 * the t loop moves inside the kernel.  For the fat warp (Ft = blend of the two warped trunk feature maps, DeMFInet.py:66-71) the
 * contexts are the INNERMOST loop of a tile, so F0 / F1 are fetched from HBM once per window instead of once per t. */
typedef struct demfi_batch {
    int32_t nb;            /* contexts in the launch; 0 or 1 = a plain launch                                              */
    int32_t _pad;          /* fat warp only: 0 = the contexts are the innermost loop of a tile, 1 = one grid slice per context (the
                              same work as nb launches without their gaps and tails; round 5)                                  */
    int64_t a, b, o;       /* byte strides of the op's A / B / out views                                                   */
    int64_t t;             /* ... of the device time instant                                                               */
    int64_t p[32];         /* ... of the op's pointer arguments, in demfi_op.p order                                       */
} demfi_batch;
/* p order: fa, fb, logit, occ_out, pack8 (demfi_op of kind WARP) */
int demfi_warp_blend_batched(const demfi_view* A, const float* fa, const demfi_view* B, const float* fb, const float* logit,
                             const float* t, const demfi_view* out, int C, int H, int W, float* occ_out, void* pack8,
                             int pack_dtype, const demfi_batch* bt, void* stream);
/* p order: flow01, flow10, acc, out (kind CFR) */
int demfi_cfr_flow_align_batched(const float* flow01, const float* flow10, const float* t, int H, int W, int64_t* acc, float* out,
                                 const demfi_batch* bt, void* stream);
/* The same with the packed copy the next layer reads (ABI v8; p order of a batched launch: flow01, flow10, acc, out, logit, pack16): the finish
 * also writes pack16 = NHWC [H,W,16] of pack_dtype holding [flow_t0, flow_t1 | flow_01, flow_10, logit | 7 zeros] -- the thin members of Agg1
 * (DeMFInet.py:77) as Refine_Module.enc1 stages them -- replacing a demfi_pack_planes launch per window.  logit: planar fp32 [H,W]; bt may be NULL. */
int demfi_cfr_flow_align_pack(const float* flow01, const float* flow10, const float* logit, const float* t, int H, int W, int64_t* acc,
                              float* out, void* pack16, int pack_dtype, const demfi_batch* bt, void* stream);

/* bilinear_sampler at ABSOLUTE flow coordinates (FGAC, DeMFInet.py:413-419, 499-514; rr = sr = 0):
 * src, out fat views with C channels; flow planar fp32 [2,H,W]. */
int demfi_fgac_gather(const demfi_view* src, const float* flow, const demfi_view* out, int C, int H,
                      int W, int32_t* dbg_maps, void* stream);

/* Generalised FGAC (radii rr > 0, DeMFInet.py:401-445): correlation of the (2rr+1)^2 bilinear samples of ref_k with
 * source_k over the C = 64 channels, softmax over the window, attention-weighted sum (Eq. 3).  fp16 NHWC views.
 * mode 0: the index map the reference code computes when its hard-coded radii are overridden (pinned by fixtures from a
 * patched in-memory copy of the reference); mode 1: window centred on flow[y,x] (the paper's description), (2rr+2)^2
 * texel window staged per pixel in LDS; both: wavefront-shuffle channel reduction + softmax.  attn_out (optional):
 * fp32 [(2rr+1)^2, H, W] softmax weights.  sr > 0 (DeMFInet.py:417, 434): apply demfi_avg_pool_fat to ref_k / source_k
 * first.  rr in {1, 2}. */
int demfi_fgac_window(const demfi_view* ref_k, const demfi_view* source_k, const float* flow, const demfi_view* out,
                      int C, int H, int W, int rr, int mode, float* attn_out, void* stream);
/* F.avg_pool2d(x, 2sr+1, stride 1, padding sr) (count_include_pad), fp16 NHWC. */
int demfi_avg_pool_fat(const demfi_view* src, const demfi_view* out, int C, int H, int W, int sr, void* stream);

/* Visualisation extras of FGAC.forward (DeMFInet.py:454-496; returned by DeMFInet.forward when args.visualization_flag or is_training,
 * 167-176).  demfi_absmean_map: out[H,W] = mean over the C channels of |a| (b == NULL) or |a - b| (torch.mean(torch.abs(.), 1));
 * demfi_minmax_normalize: plane = (plane - min(plane)) / max(plane - min(plane)) in place, the reference's two in-place steps
 * (459-461), deterministic; scratch: demfi_minmax_scratch_floats() floats; demfi_one_minus: out = 1 - in (the (1 - w_sr) map, 495). */
int     demfi_absmean_map(const demfi_view* a, const demfi_view* b, float* out, int C, int H, int W, void* stream);
int64_t demfi_minmax_scratch_floats(void);
int     demfi_minmax_normalize(float* plane, int64_t n, float* scratch, void* stream);
int     demfi_one_minus(const float* in, float* out, int64_t n, void* stream);

/* Eq.(4) gate blend (DeMFInet.py:452): out = w*source + (1-w)*e; w planar fp32 [H,W]. */
int demfi_gate_blend(const float* w, const demfi_view* source, const demfi_view* e, const demfi_view* out,
                     int C, int H, int W, void* stream);

/* Pack planar fp32 channels into an NHWC slice of the path dtype (replaces the thin members of torch.cat at
 * DeMFInet.py:77, 117-120, 123, 151-155 for the consuming convolutions).  planes: HOST array of nch device
 * pointers to [H,W] fp32 planes (NULL = zero channel); nch multiple of 8, <= 32; dst: first channel of the slice,
 * dst_pix_stride in elements. */
int demfi_pack_planes(const float* const* planes, int nch, void* dst, int dtype, int64_t dst_pix_stride,
                      int H, int W, void* stream);
/* batched over contexts: bt->p[i] = byte stride of plane i, bt->o = byte stride of dst */
int demfi_pack_planes_batched(const float* const* planes, int nch, void* dst, int dtype, int64_t dst_pix_stride, int H, int W,
                              const demfi_batch* bt, void* stream);

/* uint8 frame I/O of the boundary caller.
 * demfi_u8_to_window: frames = HOST array of 4 device pointers to BGR uint8 [h,w,3] images in the module's frame order
 * (B0,B1,B-1,B2); writes x [3,4,H,W] fp32 = RGBframes_np2Tensor normalisation (utils.py:224-238) + reflect padding to
 * H x W (utils.py:1363).
 * demfi_frame_to_u8: frame planar fp32 [3,H,W] -> out uint8 [h,w,3]: crop + denorm255_np (utils.py:718-721) + uint8
 * truncation (main.py:1165-1178), bit-identical to the reference's float64 arithmetic. */
int demfi_u8_to_window(const uint8_t* const* frames, int h, int w, float* x, int H, int W, void* stream);
/* The same fused with the first layers' loads: one pass over the 4 uint8 frames writes x (fp32 [3,4,H,W], still needed by
 * the Mixer / D2 inputs), the space-to-depth tensor of FF_RDB (NHWC [H/2,W/2,48], path dtype; pixel_reshuffle,
 * DeMFInet.py:234-235) and the overlay (mean of B0, B1; DeMFInet.py:178). */
int demfi_u8_ingest(const uint8_t* const* frames, int h, int w, float* x, void* s2d, float* overlay, int dtype, int H, int W,
                    void* stream);
/* one BGR uint8 [h,w,3] frame -> planar fp32 [3,h,w] with the same arithmetic (ground-truth frames of the evaluation) */
int demfi_u8_to_planar(const uint8_t* frame, int h, int w, float* out, void* stream);
int demfi_frame_to_u8(const float* frame, uint8_t* out, int h, int w, int H, int W, void* stream);
/* YUV 4:2:0 <-> BGR uint8 (the Y4M stream edge, demfi_amd/video.py), integer arithmetic that matches demfi_amd/y4m.py
 * (yuv420_to_bgr_np / bgr_to_yuv420_np) bit for bit.  A 4:2:0 frame is the Y4M payload: Y [h,w], then Cb and Cr
 * [ceil(h/2), ceil(w/2)]; any h, w in 2..16384.  matrix: DEMFI_BT601 / DEMFI_BT709; full_range: 0 = limited (Y 16-235,
 * C 16-240), 1 = full.  Device buffers; one launch converts n frames.
 * yuv420_to_bgr: frame i read at src + i*src_stride, written at dst + i*dst_stride; siting = the input's chroma siting.
 * bgr_to_yuv420: output chroma is 420jpeg (centred).  Frame i is read at src + (i / group)*group_stride + (i % group)*src_stride
 * (group <= 0: one group of n frames) and written at dst + i*dst_stride, so that frames kept per window in the sink's buffers
 * land in stream order in one launch.
 * bgr_to_yuv420_gather: as bgr_to_yuv420, but frame i is read at base + src_offsets[i] (src_offsets: n int64 byte offsets in
 * DEVICE memory, any order, repeats allowed) and written at dst + i*dst_stride: the egress of a retimed stream, whose windows
 * give a varying number of frames.
 * yuv420_sad: sad[i] = sum over the payload bytes of |a - b| for a at base + a_offsets[i], b at base + b_offsets[i] (n int64 byte
 * offsets each, in DEVICE memory; any alignment, any order, repeats allowed), exact in uint64; payload = the frame's byte
 * count (any length > 0).  sad is zeroed on the stream first.  Scores the scene cuts of demfi_amd/scene.py (sad_np). */
int demfi_yuv420_to_bgr(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int n, int h, int w, int matrix,
                        int full_range, int siting, void* stream);
int demfi_bgr_to_yuv420(const uint8_t* src, int64_t src_stride, int group, int64_t group_stride, uint8_t* dst, int64_t dst_stride,
                        int n, int h, int w, int matrix, int full_range, void* stream);
int demfi_bgr_to_yuv420_gather(const uint8_t* base, const int64_t* src_offsets, uint8_t* dst, int64_t dst_stride, int n, int h, int w,
                               int matrix, int full_range, void* stream);
int demfi_yuv420_sad(const uint8_t* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int64_t payload, uint64_t* sad,
                     void* stream);

/* ---- the 16-bit frame path of the Y4M edge (csrc/yuv_family.hip, yuv.hip, frames16.hip; video.py --high-depth) ------------
 * The functions above at bit depth d = `depth`, 8 <= d <= 16 (the Y4M tags C420p10 .. C420p16; 8 is accepted so that this path can
 * be compared with the 8-bit one value for value): samples and B, G, R values are unsigned 16-bit holding 0 .. peak = 2^d - 1,
 * buffers are 2-byte aligned, and EVERY stride and offset counts 16-bit samples, not bytes.  Integer arithmetic that matches
 * demfi_amd/y4m.py (yuv420_to_bgr16_np / bgr16_to_yuv420_np) bit for bit: the 8-bit definition with s = 2^(d-8) -- limited range
 * Y 16s-235s, C 16s-240s, chroma centre 2^(d-1), Q(8+d) coefficients, 64-bit accumulators, one rounding, clamp to [0, peak].
 * Any h, w in 2..16384; device buffers; one launch for n frames.
 * yuv420p16_to_bgr16: frame i read at src + i*src_stride ([payload] samples), written at dst + i*dst_stride ([h,w,3]).
 * bgr16_to_yuv420p16_gather: frame i read at base + src_offsets[i] (n int64 sample offsets in DEVICE memory, any order, repeats
 * allowed), written at dst + i*dst_stride; output chroma is 420jpeg.
 * yuv420p16_sad: sad[i] = sum over `samples` samples of |a - b|, a at base + a_offsets[i], b at base + b_offsets[i] (sample
 * offsets in DEVICE memory), exact in uint64; sad is zeroed on the stream first (demfi_amd/scene.py: sad_np on uint16 arrays).
 * u16_ingest: demfi_u8_ingest for 4 BGR uint16 [h,w,3] frames: v = p / peak, v -= 0.5, v *= 2 in fp32, the same reflect padding
 * and the same three outputs.  frame_to_u16: demfi_frame_to_u8 with peak in place of 255: float64 clip((x + 1) / 2, 0, 1) * peak,
 * truncated.
 * u16_ingest_rect: u16_ingest for the h x w rectangle at (y0, x0) of four [fh,fw,3] frames: tile pixel (sy, sx) is frame pixel
 * (y0 + sy, x0 + sx), the reflect padding is in tile coordinates, so the outputs are those of u16_ingest on the contiguous crop.
 * frame_to_u16_rect: `frame` [3,H,W] is the output of a tile whose pixel (0, 0) is pixel (y0, x0) of the [fh,fw,3] frame `out`; the
 * pixels of the kept rectangle rows ky0 .. ky1-1, columns kx0 .. kx1-1 (frame coordinates, inside the tile and the frame) are written
 * to out[(y*fw + x)*3 + c] by the rule of frame_to_u16, and nothing else is.  Both refuse a rectangle that leaves the frame. */
int demfi_yuv420p16_to_bgr16(const uint16_t* src, int64_t src_stride, uint16_t* dst, int64_t dst_stride, int n, int h, int w, int depth,
                             int matrix, int full_range, int siting, void* stream);
int demfi_bgr16_to_yuv420p16_gather(const uint16_t* base, const int64_t* src_offsets, uint16_t* dst, int64_t dst_stride, int n, int h,
                                    int w, int depth, int matrix, int full_range, void* stream);
int demfi_yuv420p16_sad(const uint16_t* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int64_t samples, uint64_t* sad,
                        void* stream);
int demfi_u16_ingest(const uint16_t* const* frames, int h, int w, int depth, float* x, void* s2d, float* overlay, int dtype, int H,
                     int W, void* stream);
int demfi_frame_to_u16(const float* frame, uint16_t* out, int h, int w, int H, int W, int depth, void* stream);
int demfi_u16_ingest_rect(const uint16_t* const* frames, int fh, int fw, int y0, int x0, int h, int w, int depth, float* x, void* s2d,
                          float* overlay, int dtype, int H, int W, void* stream);
int demfi_frame_to_u16_rect(const float* frame, uint16_t* out, int fh, int fw, int y0, int x0, int ky0, int kx0, int ky1, int kx1, int H,
                            int W, int depth, void* stream);

/* ---- the other chroma layouts of the Y4M edge (csrc/yuv_family.hip; demfi_amd/video.py --any-layout) ------------------------
 * demfi_yuv420_to_bgr / demfi_bgr_to_yuv420_gather and their 16-bit forms for layout = DEMFI_YUV_422 (Y [h,w]; Cb, Cr
 * [h, ceil(w/2)], co-sited horizontally), DEMFI_YUV_444 (three [h,w] planes) and DEMFI_YUV_MONO (Y only; B = G = R), with the
 * same argument conventions: byte strides and offsets for the uint8 pair, sample strides and offsets (and 2-byte aligned
 * buffers, depth 8..16) for the uint16 pair; any h, w in 2..16384; device buffers; one launch for n frames; the output keeps the
 * layout.  Integer arithmetic that matches demfi_amd/y4m.py (yuv_to_bgr_np / bgr_to_yuv_np, yuv_to_bgr16_np / bgr16_to_yuv_np) bit
 * for bit: the matrix step of the 4:2:0 functions; 4:2:2 upsamples by the horizontal rule of 420mpeg2 and downsamples by the
 * co-sited [1,2,1]/4 with clamped edges, 4:4:4 does neither.  DEMFI_YUV_420 is an argument error here. */
int demfi_yuvl_to_bgr(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int n, int h, int w, int layout,
                      int matrix, int full_range, void* stream);
int demfi_bgr_to_yuvl_gather(const uint8_t* base, const int64_t* src_offsets, uint8_t* dst, int64_t dst_stride, int n, int h, int w,
                             int layout, int matrix, int full_range, void* stream);
int demfi_yuvl16_to_bgr16(const uint16_t* src, int64_t src_stride, uint16_t* dst, int64_t dst_stride, int n, int h, int w, int depth,
                          int layout, int matrix, int full_range, void* stream);
int demfi_bgr16_to_yuvl16_gather(const uint16_t* base, const int64_t* src_offsets, uint16_t* dst, int64_t dst_stride, int n, int h,
                                 int w, int depth, int layout, int matrix, int full_range, void* stream);

/* ---- repeated frames of the Y4M edge (csrc/dedup.hip; demfi_amd/video.py --dedup) ---------------------------------------------
 * luma_block_counts: for pair i, frame a at base + a_offsets[i] against frame b at base + b_offsets[i] (n int64 BYTE offsets in
 * DEVICE memory; even ones for 16-bit samples), over the luma plane = the first h*w samples of a payload, sample_bytes = 1
 * (bytes) or 2 (16-bit little-endian samples).  The plane is cut into 8x8 blocks from the top-left corner (edge blocks are
 * partial, area a < 64); with SAD = sum |a - b| over a block, the block is hot when 64*SAD > hi_s*a and warm when
 * 64*SAD > lo_s*a, hi_s / lo_s = the thresholds times 2^(depth-8), 0 .. 2^40.  counts[2i] = hot blocks, counts[2i+1] = warm
 * blocks of pair i (device memory, 2n uint32, zeroed on the stream first); exact integers, the numpy definition is
 * demfi_amd/cadence.py block_counts_np.  Any h, w in 2..16384; one launch for n pairs; each frame of a pair is read once. */
int demfi_luma_block_counts(const uint8_t* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int h, int w,
                            int sample_bytes, int64_t hi_s, int64_t lo_s, uint32_t* counts, void* stream);

/* ---- interlaced input of the Y4M edge (csrc/deint.hip; demfi_amd/video.py --deinterlace) ------------------------------------------
 * yuv_bob: the n (0..64) payloads at payloads + i*stride_bytes (Y [h,w], then Cb and Cr of `layout`; sample_bytes = 1, or 2 for
 * 16-bit little-endian samples: even address and stride) become progressive frames IN PLACE: in every plane of payload i the rows
 * of parity q_i = bit i of odd_mask (0: even rows, the top field; 1: odd rows) are kept and the other rows are rebuilt from
 * them by the five-direction edge-directed line average of demfi_amd/deint.py (bob_plane_np), which this matches sample for
 * sample; a missing row with one neighbour copies it, a one-row plane whose row is not kept stays.  Kept rows and everything
 * between the payloads are not written.  Any h, w in 2..16384; stride_bytes >= the payload's bytes; one launch for all planes of
 * all payloads; n = 0 does nothing. */
int demfi_yuv_bob(void* payloads, int64_t stride_bytes, int n, int h, int w, int layout, int sample_bytes, uint64_t odd_mask,
                  void* stream);
/* yuv_deint_adaptive: the motion-adaptive mode (--deinterlace-mode adaptive; demfi_amd/deint.py adaptive_plane_np, matched sample
 * for sample).  Field i (n = 0..64 per launch) has five int64 BYTE offsets from base, offsets[5i .. 5i+4]: the payloads that hold
 * fields f-2, f-1, f, f+1, f+2 of the stream, -1 for a field the stream does not have (even offsets for 16-bit samples).  The
 * payload of f, whose rows of parity q_i = bit i of odd_mask are kept, becomes a progressive frame IN PLACE: a missing row with
 * both neighbours is the bob's value clamped to [d - diff, d + diff] (yadif's temporal rule with the spatial check), every other row
 * as in yuv_bob.  Of the payloads of f-1 and f+1 only rows of parity 1 - q_i are read, of those of f-2 and f+2 only rows of parity
 * q_i, i.e. kept rows of the fields they belong to: such a payload may be raw, already rebuilt, or rebuilt by the same launch.  The
 * offsets are passed twice with the same content: offsets in HOST memory, checked here before anything is launched (every present
 * payload inside base .. base + size_bytes, the payload of f present, f-1 or f+1 present, no payload rebuilt twice), and
 * offsets_dev in DEVICE memory, read by the kernel, which leaves a field without its own payload alone and gives one without f-1
 * and f+1 the bob's value.  One launch for all planes of all n fields; n = 0 does nothing. */
int demfi_yuv_deint_adaptive(void* base, int64_t size_bytes, const int64_t* offsets, const int64_t* offsets_dev, int n, int h, int w,
                             int layout, int sample_bytes, uint64_t odd_mask, void* stream);

/* ---- temporal denoising of the Y4M edge (csrc/denoise.hip; demfi_amd/video.py --denoise) --------------------------------------------
 * payload_denoise: frame i (n = 0..64 per launch) has taps + 1 int64 BYTE offsets, offsets[i*(taps+1) .. i*(taps+1) + taps]: first the
 * taps = 2 R + 1 (3, 5 or 7) payloads of frames f - R step .. f + R step of the stream in that order, offsets from src, -1 for a frame
 * the stream does not have (the centre, entry R, must be present), then the offset from dst at which the denoised payload of f is
 * written.  A payload is one flat array of P stored samples (sample_bytes = 1, or 2 for 16-bit little-endian samples: even addresses and
 * offsets): layout, depth, matrix and range do not matter.  With c the centre's sample, each side walks outward from the centre on its
 * own, adds up d = |x - c| and stops for good at the first absent payload, the first d > thr_a or the first accumulated d > thr_b; the
 * output is (2 * sum + k) / (2 * k) over c and the k - 1 samples taken before the stops, round half up, exact integers; the numpy
 * definition is demfi_amd/denoise.py denoise_payload_np (thr_a, thr_b: its thresholds at the stream's depth, 0 <= thr_a <= thr_b <= 255
 * for bytes, <= 65535 for 16-bit samples).  src is only read and dst only written.  The offsets are passed twice with the same content:
 * offsets in HOST memory, checked here before anything is launched, and offsets_dev in DEVICE memory, read by the kernel.
 * DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n outside 0..64, taps not 3, 5 or 7, sample_bytes not 1 or 2, thresholds out of
 * range, P outside 1..2^40, 16-bit samples at an odd address or offset, an offset below -1, an absent centre, a payload that leaves
 * src .. src + src_bytes or dst .. dst + dst_bytes, two frames whose destinations overlap, src and dst buffers that overlap.  When src +
 * every present offset and dst + every destination offset are multiples of 16 every thread makes 16 output bytes from 16-byte loads and
 * one 16-byte store (the last P * sample_bytes mod 16 bytes of a payload sample by sample); otherwise the whole launch goes sample by
 * sample with the same arithmetic.  Every offset and index is 64-bit.  One launch for all n frames, no LDS, no atomics, plain stores;
 * n == 0 does nothing. */
int demfi_payload_denoise(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int64_t* offsets_dev, int n, int taps,
                          int64_t P, int sample_bytes, int thr_a, int thr_b, uint8_t* dst, int64_t dst_bytes, void* stream);

/* ---- deblocking of the Y4M edge (csrc/deblock.hip; demfi_amd/video.py --deblock) ------------------------------------------------------
 * payload_deblock: the n (>= 0, any number) payloads at payloads + i*stride_bytes are deblocked IN PLACE (sample_bytes = 1, or 2 for 16-bit
 * little-endian samples: even address and stride).  planes: the plane table in HOST memory, n_planes (1..6: 3 planes x 2 fields) entries of
 * six int64 each, what demfi_amd/deblock.py plane_table gives: the plane's first sample in the payload, its rows and cols (1..16384 each),
 * its row pitch in samples (>= cols; two rows for a field of an interlaced payload) and its x and y phase (0..7: the columns and rows that
 * a crop removed in front of it, mod 8).  The entries must not share a sample.  Every entry is filtered as a plane in its own right by
 * H.264's intra-edge (bS = 4) luma filter on the fixed grid of 8: a vertical edge at column x when (x + x phase) % 8 == 0 and 4 <= x <=
 * cols - 4, rows likewise; a line p3 p2 p1 p0 | q0 q1 q2 q3 across an edge changes only when |p0-q0| < thr_a, |p1-p0| < thr_b and
 * |q1-q0| < thr_b, a side takes the strong form when also |p0-q0| < thr_s and |p2-p0| < thr_b (q side: the mirror image), p3 and q3 never
 * change; all vertical edges first, then all horizontal edges on that result.  Exact integers; the numpy definition is
 * deblock_payload_np, matched byte for byte (thr_a, thr_b, thr_s: deblock.thresholds at the stream's depth, 0 <= thr_b <= thr_a <= 255
 * for bytes, <= 65535 for 16-bit samples, thr_s likewise).  A workgroup owns a tile of a plane whose borders lie half way between edges,
 * so it reads and writes nothing another workgroup touches: no second buffer, no atomics.  Samples no entry names and everything between
 * the payloads are neither read nor written.
 * DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, sample_bytes not 1 or 2, n_planes outside 1..6, thresholds out of range, a
 * plane that starts below sample 0, a side outside 1..16384, a pitch below cols, a phase outside 0..7, 16-bit samples at an odd address
 * or stride, stride_bytes below the bytes the table reaches.  One launch for all planes of all n payloads; n == 0 does nothing. */
int demfi_payload_deblock(void* payloads, int64_t stride_bytes, int n, const int64_t* planes, int n_planes, int sample_bytes, int thr_a,
                          int thr_b, int thr_s, void* stream);

/* ---- deringing of the Y4M edge (csrc/dering.hip; demfi_amd/video.py --dering) ----------------------------------------------------------
 * payload_dering: the n (>= 0, any number) payloads at src + i*src_stride_bytes are deringed into dst + i*dst_stride_bytes, OUT OF PLACE: the
 * two ranges must not overlap (sample_bytes = 1, or 2 for 16-bit little-endian samples: even addresses and strides).  planes: the plane
 * table in HOST memory as for demfi_payload_deblock, n_planes (1..6) entries of six int64 each: first sample, rows, cols (1..16384 each),
 * row pitch in samples (>= cols), x and y phase (0..7).  The entries must not share a sample.  Every entry is filtered as a plane in its own
 * right by AV1's constrained directional enhancement filter: blocks of 8x8 start at column x when (x + x phase) % 8 == 0, rows likewise
 * (the first and last block of an axis may be partial); a block's direction is the first of the greatest of 8 costs over x = min(v >>
 * (depth - 8), 255) - 128 at positions clamped into the plane, its variance (cost[dir] - cost[dir ^ 4]) >> 10 scales the primary strength;
 * a sample takes 4 primary taps along the direction (weights 4, 2) and 8 secondary taps along dir +- 2 (weights 2, 1), each through
 * constrain(diff, thr, damping), rounds the sum / 16 to nearest, ties away from zero, and is clamped to the extremes of itself and its
 * taps; taps outside the plane are skipped.  pri (0..15), sec (0..4) and damping (3..6) are at the 8-bit scale and depth (8, 10, 12, 14 or
 * 16; above 8 needs sample_bytes = 2) shifts them inside.  Exact integers; the numpy definition is dering.dering_payload_np, matched byte
 * for byte.  Every sample of every entry is written; where the entries do not name every sample up to the last one they reach, the
 * payloads are copied first, so dst holds whole payloads.  Nothing between the payloads is read or written.
 * DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, sample_bytes not 1 or 2, a depth outside the list or above 8 in bytes, pri,
 * sec or damping out of range, n_planes outside 1..6, a plane that starts below sample 0, a side outside 1..16384, a pitch below cols, a
 * phase outside 0..7, 16-bit samples at an odd address or stride, a stride below the bytes the table reaches or so large that n of them
 * leave int64, src and dst ranges that overlap.  One launch for all planes of all n payloads; n == 0 does nothing. */
int demfi_payload_dering(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes, int n, const int64_t* planes,
                         int n_planes, int sample_bytes, int depth, int pri, int sec, int damping, void* stream);

/* ---- debanding of the Y4M edge (csrc/deband.hip; demfi_amd/video.py --deband) -------------------------------------------------------------
 * payload_deband: the n (>= 0, any number) payloads at src + i*src_stride_bytes are debanded into dst + i*dst_stride_bytes, OUT OF PLACE: the
 * two ranges must not overlap (sample_bytes = 1, or 2 for 16-bit little-endian samples: even addresses and strides).  planes: the plane
 * table in HOST memory as for demfi_payload_dering, n_planes (1..6) entries of six int64 each: first sample, rows, cols (1..16384 each),
 * row pitch in samples (>= cols), x and y phase (0..7; checked, carried and ignored: banding has no grid).  The entries must not share a
 * sample.  Every entry is filtered as a plane in its own right by a range-limited box mean: for a sample c at (x, y), rx = min(radius, x,
 * cols - 1 - x), ry = min(radius, y, rows - 1 - y) (the window is clipped symmetrically about the sample and never leaves the plane), N =
 * the samples v of the source at (x + i, y + j), |i| <= rx, |j| <= ry, with |v - c| < thr8 << (depth - 8), n = |N| >= 1, out =
 * (2 sum(N) + n) / (2 n) floored: the mean of the near samples rounded to nearest, ties up.  thr8 (0..8) is at the 8-bit scale, radius
 * (1..16) in samples; depth is 8, 10, 12, 14 or 16 (above 8 needs sample_bytes = 2).  Exact integers; the numpy definition is
 * deband.deband_payload_np, matched byte for byte.  thr8 == 0 copies the payloads.  Every sample of every entry is written; where the
 * entries do not name every sample up to the last one they reach, the payloads are copied first, so dst holds whole payloads.  Nothing
 * between the payloads is read or written.
 * DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, sample_bytes not 1 or 2, a depth outside the list or above 8 in bytes, thr8
 * or radius out of range, n_planes outside 1..6, a plane that starts below sample 0, a side outside 1..16384, a pitch below cols, a phase
 * outside 0..7, 16-bit samples at an odd address or stride, a stride below the bytes the table reaches or so large that n of them leave
 * int64, src and dst ranges that overlap.  One launch for all planes of all n payloads; n == 0 does nothing. */
int demfi_payload_deband(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes, int n, const int64_t* planes,
                         int n_planes, int sample_bytes, int depth, int thr8, int radius, void* stream);

/* ---- spatial denoising of the Y4M edge (csrc/nlmeans.hip; demfi_amd/video.py --nlmeans) ---------------------------------------------------
 * payload_nlmeans: the n (>= 0, any number) payloads at src + i*src_stride_bytes are denoised into dst + i*dst_stride_bytes, OUT OF PLACE:
 * the two ranges must not overlap (sample_bytes = 1, or 2 for 16-bit little-endian samples: even addresses and strides).  planes: the plane
 * table in HOST memory as for demfi_payload_deband, n_planes (1..6) entries of six int64 each: first sample, rows, cols (1..16384 each),
 * row pitch in samples (>= cols), x and y phase (0..7; checked, carried and ignored).  The entries must not share a sample.  Every entry
 * is filtered as a plane in its own right by non-local means in exact integers.  With u(x, y) the sample of the source at column
 * clamp(x, 0, cols - 1), row clamp(y, 0, rows - 1), s = depth - 8, b = min(s, 4) and q(t) = min(|t| >> (s - b), 4095): for the sample at
 * (x, y) and every offset (i, j), |i|, |j| <= search, whose candidate (x + i, y + j) lies inside the plane, D = the sum over |a|, |e| <=
 * patch of q(u(x + a, y + e) - u(x + i + a, y + j + e))^2, w = table[min(D >> shift, 1023)], v = u(x + i, y + j); out =
 * (2 sum(w v) + W) / (2 W) floored, W = sum(w): the weighted mean rounded to nearest, ties up.  table: 1024 uint16 in HOST memory, read
 * before the call returns (nlmeans.weight_table gives it and shift): table[0] = 256, no entry above 256, none above the one before; a
 * table that is 0 behind table[0] is the identity.  patch is 1..3, search 1..7, shift 0..31; depth is 8, 10, 12, 14 or 16 (above 8 needs
 * sample_bytes = 2).  Exact integers at every depth (the sums are unsigned 32-bit: sum(w v) <= 225 * 256 * 65535); the numpy definition is
 * nlmeans.nlmeans_payload_np, matched byte for byte.  Every sample of every entry is written; where the entries do not name every sample
 * up to the last one they reach, the payloads are copied first, so dst holds whole payloads.  Nothing between the payloads is read or
 * written.
 * DEMFI_ERR_ARG, with nothing launched: a NULL buffer or table, n < 0, sample_bytes not 1 or 2, a depth outside the list or above 8 in
 * bytes, patch, search or shift out of range, a table that does not start at 256, exceeds it or increases, n_planes outside 1..6, a plane
 * that starts below sample 0, a side outside 1..16384, a pitch below cols, a phase outside 0..7, 16-bit samples at an odd address or
 * stride, a stride below the bytes the table reaches or so large that n of them leave int64, src and dst ranges that overlap.  One launch
 * for all planes of all n payloads; n == 0 does nothing. */
int demfi_payload_nlmeans(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes, int n, const int64_t* planes,
                          int n_planes, int sample_bytes, int depth, int patch, int search, const uint16_t* table, int shift, void* stream);

/* ---- inverse telecine of the Y4M edge (csrc/ivtc.hip; demfi_amd/video.py --ivtc) ------------------------------------------------
 * A woven frame W(top, bot) has the even rows of the luma plane (the first h*w samples of a payload; sample_bytes = 1, or 2 for
 * 16-bit little-endian samples) of payload `top` and the odd rows of that of payload `bot`; it is read in place, never built.
 * Offsets are int64 BYTE offsets from base in DEVICE memory (even ones for 16-bit samples).  Any h, w in 2..16384; one launch for
 * n entries; nothing but the output words is written, and those are zeroed on the stream first; n = 0 does nothing.
 * luma_comb_counts: entry i has the top payload at top_offsets[i] and three candidates for the bottom field at
 * bot_offsets[3i + k], k = 0, 1, 2 (c, p, n of demfi_amd/telecine.py), -1 for an absent one.  out[6i + 2k] = the most combed
 * samples in one 16x16 block (blocks from the top-left corner, partial at the right and bottom), out[6i + 2k + 1] = the combed
 * samples of the plane, of W(top, candidate k); both stay 0 for an absent candidate.  A sample of row y, 2 <= y <= h-3, is combed
 * when, with d1 = W[y] - W[y-1] and d2 = W[y] - W[y+1], (d1 > T and d2 > T) or (d1 < -T and d2 < -T), and
 * |W[y-2] + 4 W[y] + W[y+2] - 3 (W[y-1] + W[y+1])| > 6 T, T = thresh_s = the threshold times 2^(depth-8), 0 .. 2^20.  Exact
 * integers; the numpy definition is telecine.comb_counts_np.  The three candidates are scored in one pass over their shared even
 * rows: the top plane and each present candidate's plane are read about once.
 * luma_woven_sad: out[i] (uint64) = sum |W(a_top, a_bot) - W(b_top, b_bot)| over the luma plane, the four payloads at
 * offsets[4i .. 4i+3] in that order; the numpy definition is telecine.woven_sad_np. */
int demfi_luma_comb_counts(const uint8_t* base, const int64_t* top_offsets, const int64_t* bot_offsets, int n, int h, int w,
                           int sample_bytes, int thresh_s, uint32_t* out, void* stream);
int demfi_luma_woven_sad(const uint8_t* base, const int64_t* offsets, int n, int h, int w, int sample_bytes, uint64_t* out,
                         void* stream);

/* ---- letterbox and pillarbox bars of the Y4M edge (csrc/crop.hip; demfi_amd/video.py --crop auto) ----------------------------------
 * luma_line_counts: plane i is the luma plane (the first h*w samples; sample_bytes = 1, or 2 for 16-bit little-endian samples) of
 * the payload at base + offsets[i] (n int64 BYTE offsets in DEVICE memory, any order; even ones for 16-bit samples).
 * rows[i*h + y] = the samples of row y strictly greater than thresh, cols[i*w + x] = those of column x (device memory, n*h and
 * n*w uint32, zeroed on the stream first); thresh = the limit times 2^(depth-8), 0 .. 65535.  Exact integers; the numpy
 * definition is demfi_amd/letterbox.py line_counts_np.  Any h, w in 2..16384; one launch for n planes; every sample is loaded
 * once; nothing but rows and cols is written; n = 0 does nothing. */
int demfi_luma_line_counts(const uint8_t* base, const int64_t* offsets, int n, int h, int w, int sample_bytes, int64_t thresh,
                           uint32_t* rows, uint32_t* cols, void* stream);

/* ---- synthesized motion blur of the Y4M edge (csrc/shutter.hip; demfi_amd/video.py --shutter) -------------------------------------
 * payload_mix: written payload i (n per launch) is the rounded box average of the fine payloads it keeps: row i has smax (1..32)
 * int64 BYTE offsets from base, offsets[i*smax .. i*smax + smax - 1], the k_i kept ones first and -1 behind them (k_i >= 1).  Every
 * one of the P stored samples (sample_bytes = 1, or 2 for 16-bit little-endian samples: even addresses and stride) of the payload at
 * dst + i*dst_stride becomes (2 * sum + k_i) / (2 * k_i) of the samples at its position in the kept payloads: round half up, exact
 * integers, in the stored (gamma) values; the numpy definition is demfi_amd/shutter.py mix_np.  The payload is one flat array: layout,
 * depth, matrix and range do not matter.  The offsets are passed twice with the same content: offsets in HOST memory, checked here
 * before anything is launched (a row whose first offset is -1, a kept offset behind a -1 or an offset below -1 is DEMFI_ERR_ARG, and
 * so are smax outside 1..32, a bad sample_bytes and dst_stride < P * sample_bytes), and offsets_dev in DEVICE memory, read by the
 * kernel.  When base + every kept offset, dst and dst_stride are multiples of 16 every thread makes 16 output bytes from 16-byte loads
 * and one 16-byte store (the last P * sample_bytes mod 16 bytes of a row sample by sample); otherwise the whole launch goes sample by
 * sample with the same arithmetic.  The bytes between P * sample_bytes and dst_stride are not written.  One launch for all n rows, no
 * LDS, no atomics; the sources may overlap each other but not dst; n <= 0 does nothing. */
int demfi_payload_mix(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, int smax, int64_t P,
                      int sample_bytes, uint8_t* dst, int64_t dst_stride, void* stream);

/* payload_mix_w: payload_mix with a weighted window (--shutter-window; the numpy definition is mix_np(..., weights=...)).  weights is
 * HOST memory: smax int32 weights w_j >= 1 whose sum is at most 4096, one vector for all rows of the launch.  The kept offsets of a row
 * are its first k_i samples, so with W = w_0 + .. + w_(k_i - 1) every stored sample becomes (2 * sum_j w_j x_j + W) / (2 W): round half
 * up, exact integers (32-bit accumulators: 2 * 4096 * 65535 + 4096 < 2^30; the division is one multiply-high with the constants of
 * demfi_amd/shutter.py magic_w, computed here on the host for every k and passed to the kernel by value).  Everything else is
 * payload_mix: the same checks, paths, strides and launch shape.  DEMFI_ERR_ARG, launching nothing, also for weights == NULL, a weight
 * below 1 and a sum of weights above 4096.  All weights 1 give the bytes of payload_mix. */
int demfi_payload_mix_w(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, int smax, int64_t P,
                        int sample_bytes, uint8_t* dst, int64_t dst_stride, const int32_t* weights, void* stream);

/* ---- interlaced output of the Y4M edge (csrc/interlace.hip; demfi_amd/video.py --interlace) ------------------------------------------
 * payload_weave: written payload i (n per launch) weaves two progressive payloads: row i has two int64 BYTE offsets from base,
 * offsets[2 i] the frame of the first field in time and offsets[2 i + 1] that of the second (equal for an odd tail).  A payload is
 * n_planes (1..3) planes one behind the other, plane p of planes[2 p] rows and planes[2 p + 1] columns of samples (1..32768 each;
 * planes is HOST memory); sample_bytes = 1, or 2 for 16-bit little-endian samples (even addresses and stride).  Output row y of a
 * plane comes from the first source when y mod 2 == q0 (0 or 1), else from the second, low-passed vertically within that one source,
 * rows clamped to the plane: lowpass 0 = off (c), 1 = linear ((a + 2 c + b + 2) >> 2), 2 = complex (v = clip((4 + 6 c + 2 (a + b) - a2
 * - b2) >> 3, 0, peak); a + b > 2 c ? max(v, c) : min(v, c)) with c, a / b, a2 / b2 the source's rows y, y -/+ 1, y -/+ 2; the numpy
 * definition is demfi_amd/interlace.py weave_payload_np.  The payload is written at dst + i*dst_stride; the bytes between its end and
 * dst_stride are not written.  The offsets are passed twice with the same content: offsets in HOST memory, checked here before
 * anything is launched, and offsets_dev in DEVICE memory, read by the kernel.  DEMFI_ERR_ARG, with nothing launched: a NULL buffer,
 * sample_bytes not 1 or 2, 16-bit samples at an odd address, offset or stride, peak outside 1..65535 (1..255 for bytes), q0 or
 * lowpass out of range, no plane or more than three, a plane size out of range, dst_stride below the payload, a negative offset.
 * When base + every offset, every plane's first byte and row length in bytes, dst and dst_stride are multiples of 16 every thread
 * walks a 16-byte column down a strip of rows with 16-byte loads and streaming stores; otherwise the whole launch goes sample by
 * sample with the same arithmetic (decided per launch).  One launch for all n rows, no LDS, no atomics; the sources may overlap each
 * other but not dst; n <= 0 does nothing. */
int demfi_payload_weave(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes,
                        int n_planes, int sample_bytes, int peak, int q0, int lowpass, uint8_t* dst, int64_t dst_stride, void* stream);

/* ---- resized output of the Y4M edge (csrc/scale.hip; demfi_amd/video.py --scale) -------------------------------------------------------
 * payload_scale: written payload i (n per launch) is the source payload at base + offsets[i] (int64 BYTE offsets) with every plane
 * resampled by a separable polyphase filter.  A payload is n_planes (1..3) planes one behind the other; plane p has planes_in[2 p] rows
 * and planes_in[2 p + 1] columns of samples in the source and planes_out[2 p] x planes_out[2 p + 1] in dst (1..32768 each; both lists
 * are HOST memory; a payload stays below 2^31 bytes); sample_bytes = 1, or 2 for 16-bit little-endian samples (even addresses, offsets
 * and stride).  The function computes no weights: tables_dev is one DEVICE blob (4-byte aligned) that holds, per plane and axis, first
 * (int32 [n_out]: the source index of tap 0 of output sample o; indices clamp to the axis where they are used) and coef (int16
 * [n_out][T], Q14, a row sums to 1 << 14), as demfi_amd/scale.py axis_table gives them (table_blob lays them out); table_desc is HOST
 * memory, int32 [6 n_planes + 1]: per plane the byte offsets in the blob of the horizontal first and coef, the horizontal taps Tx, the
 * byte offsets of the vertical first and coef, the vertical taps Ty; the last word is the blob's size in bytes.  In exact integers,
 * >> an arithmetic shift:  t = (sum_j cx[xo][j] src[y][clamp(fx[xo] + j)] + 128) >> 8 (signed, unclamped), then
 * v = clip((sum_j cy[yo][j] t[clamp(fy[yo] + j)][xo] + 2^19) >> 20, 0, peak); the numpy definition is scale_payload_np.  The payload
 * is written at dst + i*dst_stride; the bytes between its end and dst_stride are not written.  The offsets are passed twice with the
 * same content: offsets in HOST memory, checked here before anything is launched, and offsets_dev in DEVICE memory, read by the kernel.
 * DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, no plane or more than three, a plane size out of range, sample_bytes not
 * 1 or 2, 16-bit samples at an odd address, offset or stride, peak outside 1..65535 (1..255 for bytes), taps outside 1..32, a table
 * offset that is negative, misaligned (first: 4 bytes, coef: 2) or ends behind the blob, a payload of 2^31 bytes or more, dst_stride
 * below the output payload, a negative offset.  One launch for all n payloads: a 256-thread workgroup owns 64 columns x 16 rows of one
 * output plane (fewer rows beyond a 4:1 shrink), keeps the horizontal pass of the source rows they need in 24 KiB of LDS as int32 and
 * reads them back with 128-bit reads for the vertical pass; both sums in int32 for bytes, the vertical one in 64 bits for 16-bit
 * samples; 4- or 8-byte stores where the destination address allows.  No atomics; the sources may overlap each other but not dst;
 * n == 0 does nothing. */
int demfi_payload_scale(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes_in,
                        const int32_t* planes_out, int n_planes, int sample_bytes, int peak, const uint8_t* tables_dev,
                        const int32_t* table_desc, uint8_t* dst, int64_t dst_stride, void* stream);

/* ---- bit depth of the Y4M edge (csrc/bitdepth.hip; demfi_amd/video.py --work-depth / --out-depth) ------------------------------------
 * payload_promote / payload_requant: written payload i (n per launch) is the source payload at base + offsets[i] (int64 BYTE offsets)
 * with every sample taken from depth_in to depth_out bits (8, 10, 12, 14 or 16 each; promote: depth_out > depth_in, requant: depth_out <
 * depth_in).  A payload is n_planes (1..3) planes one behind the other, plane p of planes[2 p] rows and planes[2 p + 1] columns of samples
 * (1..2^20 each, 2^30 samples a plane at most; planes is HOST memory), the first luma, the others chroma; in_bytes / out_bytes are the bytes of a source / written
 * sample: 1 at 8 bits, 2 (little-endian; even addresses, offsets and stride) above.  In exact integers, floor the mathematical floor:
 *   out = clip(off_out + floor(((v - off_in) * num + T) / den), 0, 2^depth_out - 1)
 * full_range = 0: off = 0 and (num, den) = (2^(depth_out - depth_in), 1) going up, (1, 2^(depth_in - depth_out)) going down; full_range = 1:
 * (num, den) = (2^depth_out - 1, 2^depth_in - 1), off = 0 for luma and 2^(depth - 1) for chroma on each side.  T = den / 2 for promote and
 * for dither = 0; dither = 1 (requant): T = ((2 B + 1) * den) >> 7, B the 8x8 ordered-dither index of the sample's column x and row y
 * within its plane, B = sum_{i=0..2} (((x ^ y) >> i) & 1) << (5 - 2 i) | ((y >> i) & 1) << (4 - 2 i), with y = row >> 1 when field_rows = 1
 * (the payload holds two fields).  v is the stored sample, whatever it holds.  The numpy definition is demfi_amd/bitdepth.py
 * convert_payload_np.  The payload is written at dst + i*dst_stride; the bytes between its end and dst_stride are not written.  The
 * offsets are passed twice with the same content: offsets in HOST memory, checked here before anything is launched, and offsets_dev in
 * DEVICE memory, read by the kernel.  DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, no plane or more than three, a plane
 * size out of range, a depth that is none of the five or goes the wrong way, sample bytes that do not fit the depths, a flag that is
 * neither 0 nor 1, 16-bit samples at an odd address, offset or stride, dst_stride below the written payload, a negative offset.  When base
 * + every offset, every plane's first sample and row length are multiples of 8 source samples and dst and dst_stride multiples of 8
 * written samples, every thread makes 8 samples from one 16-byte (8-byte for bytes) load with one streaming store of 16 (8) bytes;
 * otherwise the whole launch goes sample by sample with the same arithmetic (decided per launch).  One launch for all n payloads, no LDS,
 * no atomics, no table; the sources may overlap each other but not dst; n == 0 does nothing. */
int demfi_payload_promote(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes,
                          int n_planes, int in_bytes, int out_bytes, int depth_in, int depth_out, int full_range, uint8_t* dst,
                          int64_t dst_stride, void* stream);
int demfi_payload_requant(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes,
                          int n_planes, int in_bytes, int out_bytes, int depth_in, int depth_out, int full_range, int dither,
                          int field_rows, uint8_t* dst, int64_t dst_stride, void* stream);

/* ---- film grain at the egress of the Y4M edge (csrc/grain.hip; demfi_amd/video.py --grain) ---------------------------------------------
 * payload_grain: written payload i (n per launch) is the source payload at base + offsets[i] (int64 BYTE offsets) with synthetic grain
 * added.  A payload is n_planes (1 or 3) planes one behind the other, plane p of planes[2 p] rows and planes[2 p + 1] columns of samples
 * (1..65531 each; HOST memory; a payload stays below 2^31 bytes), the first luma, the others chroma of one shape: the luma's or half of
 * it, rounded up, on either axis (sx, sy = 1 or 2).  sample_bytes = 1 at depth 8, 2 (little-endian; even addresses, offsets and stride) at
 * 10, 12, 14 and 16.  keys: uint32 [3 n], the key of plane p of payload i at keys[3 i + p] (demfi_amd/grain.py plane_key; three words per
 * payload whatever n_planes); gains: int32 [2][256], the gain tables of luma and chroma (grain.gain_tables).  In exact integers, >> an
 * arithmetic shift, mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32:
 *   white(X, Y) = b0 + b1 + b2 + b3 - 510 over the bytes of mix32(key ^ mix32((Y << 16) | X))
 *   F(x, y)     = sum over i, j in -size..size of c[i] c[j] white(x + 2 + i, y + 2 + j), c = [1], [1,2,1], [1,4,6,4,1] for size 0, 1, 2
 *   out         = clip(v + ((F * G[min(L >> (depth - 8), 255)] + 2^15) >> 16), min(lo, v), max(hi, v))
 * L is the source payload's own luma: v in the luma plane, for the chroma sample (x, y) the luma sample at (min(x sx, w - 1), min(y sy,
 * h - 1)); lo / hi: full_range = 0: 16 << (depth - 8) and 235 << (depth - 8) (chroma: 240 << (depth - 8)), full_range = 1: 0 and 2^depth
 * - 1.  v is the stored sample, whatever it holds.  The numpy definition is grain.grain_payload_np.  The payload is written at dst +
 * i*dst_stride; the bytes between its end and dst_stride are not written.  offsets, keys and gains are passed twice with the same
 * content: in HOST memory, checked here before anything is launched, and (offsets_dev, keys_dev, gains_dev) in DEVICE memory, read by
 * the kernel.  DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, a plane count other than 1 or 3, a plane size out of range,
 * chroma planes that do not fit the luma plane, a depth that is none of the five, sample_bytes that do not fit it, full_range not 0 or 1,
 * size outside 0..2, a gain that is negative or so large that F * G + 2^15 could leave int32 at this size, a payload of 2^31 bytes or
 * more, 16-bit samples at an odd address, offset or stride, keys_dev or gains_dev off a 4-byte boundary, dst_stride below the payload, a
 * negative offset.  One launch for all n payloads: a 256-thread workgroup owns 64 columns x 16 rows of one plane, hashes the white
 * cells of the tile and its halo once into LDS (int16), runs the separable taps through LDS (size 0: no LDS for the noise), keeps the
 * plane's gain table in LDS and moves the samples with 16-byte loads and stores where the addresses allow, sample by sample otherwise.
 * No atomics; the sources may overlap each other but not dst; n == 0 does nothing. */
int demfi_payload_grain(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, const uint32_t* keys,
                        const uint32_t* keys_dev, int n, const int32_t* planes, int n_planes, int sample_bytes, int depth, int full_range,
                        int size, const int32_t* gains, const int32_t* gains_dev, uint8_t* dst, int64_t dst_stride, void* stream);

/* ---- linear light at the Y4M edge (csrc/colour.hip; demfi_amd/video.py --linear-light) -------------------------------------------------
 * A LINEAR payload of an h x w frame is uint16 [3, h, w]: planes B, G, R at full resolution, linear light 0 .. 65535, whatever the working
 * depth (8, 10 or 12) and the chroma layout.  The functions compute no transfer function: fwd_table (DEVICE, uint16 [2^depth]: code ->
 * linear value) and inv_table (DEVICE, uint16 [65536]: linear value -> the code nearest in light) are those of demfi_amd/colour.py
 * (forward_table / inverse_table), and the numpy definitions are linearize_np / encode_payload_np there, matched bit for bit.
 * bgr_to_linear_gather: written payload i (n per launch) is the interleaved BGR frame of codes at base + src_offsets[i] (DEVICE int64
 * offsets in SAMPLES of sample_bytes = 1, uint8 at depth 8, or 2, uint16), every code replaced by fwd_table[code] (a stored value above
 * the peak reads the peak's entry); it is written at dst + i*dst_stride (uint16 samples, at least 3 h w).
 * linear_to_yuv: written payload i is the linear payload at src + offsets[i] (int64 BYTE offsets, even) taken to codes through inv_table
 * and then to Y'CbCr by the arithmetic of demfi_bgr_to_yuv420_gather / demfi_bgr_to_yuvl_gather and their 16-bit forms (matrix, range,
 * rounding, 2x2 box, 4:2:2 [1,2,1]); any layout of demfi_yuv_layout; samples are bytes at depth 8, 16-bit little-endian above; it is
 * written at dst + i*dst_stride BYTES.  The offsets are passed twice with the same content: offsets in HOST memory, checked here before
 * anything is launched, and offsets_dev in DEVICE memory, read by the kernel.
 * DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, a frame size outside 2..16384, a depth other than 8, 10 or 12, sample_bytes
 * that do not fit the depth, an unknown layout, matrix or range flag, 16-bit samples at an odd address, offset or stride, a dst_stride
 * below the written payload, a negative offset.  One launch for all n payloads: a lane owns 8 pixels of a row (4:2:0 encode: of two rows);
 * fwd_table is copied into LDS once per workgroup, inv_table is read through L2.  No atomics; n == 0 does nothing. */
int demfi_bgr_to_linear_gather(const void* base, const int64_t* src_offsets, uint16_t* dst, int64_t dst_stride, int n, int h, int w,
                               int sample_bytes, int depth, const uint16_t* fwd_table, void* stream);
int demfi_linear_to_yuv(const uint8_t* src, const int64_t* offsets, const int64_t* offsets_dev, int n, int h, int w, int depth, int layout,
                        int matrix, int full_range, const uint16_t* inv_table, uint8_t* dst, int64_t dst_stride, void* stream);

/* ---- a 3D colour LUT at the egress of the Y4M edge (csrc/lut3d.hip; demfi_amd/video.py --lut) ---------------------------------------------
 * rgb_lut3d: written payload i (n per launch) is the RGB payload (uint16 [3, h, w], planes B, G, R: the LINEAR payload's format above) at
 * src + offsets[i] (int64 BYTE offsets, even) taken through a cube of cube_n^3 lattice points (2..65) by tetrahedral interpolation in
 * exact integers; the numpy definition is lut3d.lut_payload_np, matched byte for byte.  Per pixel and channel: code = inv_in[v] (DEVICE,
 * uint16 [65536]: colour.inverse_table of the table the payloads were made with; a value above the peak reads the peak's entry), word =
 * axis_table[code] (DEVICE, uint32 [2^depth]: lut3d.axis_table, idx << 16 | frac with idx the lattice cell, clamped here to cube_n - 2,
 * and frac in 0..65535).  With the fractions sorted f1 >= f2 >= f3, v0 the cell's low corner, v1 = v0 plus a step along the axis of f1,
 * v2 = v1 plus a step along the axis of f2, v3 the high corner, per output channel
 *   out = (Q[v0] (65535 - f1) + Q[v1] (f1 - f2) + Q[v2] (f2 - f3) + Q[v3] f3 + 32767) / 65535, rounded down, in uint32,
 * Q = cube (DEVICE, uint16 [cube_n^3][4]: R, G, B, 0 of the lattice point r + cube_n g + cube_n^2 b; lut3d.cube_words; 8-byte aligned).
 * The written payload, 16-bit encoded values in the same format, lies at dst + i*dst_stride BYTES; the bytes between its end and
 * dst_stride are not written.  cube_in_lds = 1 (cube_n <= 17 only) keeps the cube in LDS instead of reading it through L2: the same
 * bytes, another schedule.  The offsets are passed twice with the same content: offsets in HOST memory, checked here before anything is
 * launched, and offsets_dev in DEVICE memory, read by the kernel.  DEMFI_ERR_ARG, with nothing launched: a NULL buffer, n < 0, a frame
 * size outside 2..16384, a depth other than 8, 10 or 12, a cube size outside 2..65, cube_in_lds not 0 or 1 or with a cube above 17,
 * axis_table off a 4-byte or cube off an 8-byte boundary, a dst_stride below the 6 h w bytes of a payload, a negative offset, an odd
 * address, offset or stride, a dst that overlaps the span of the source payloads (the stage does not work in place).  One launch: a lane
 * owns 8 pixels of a row, one 16-byte access per plane in and out where the addresses allow; axis_table is copied into LDS once per
 * workgroup.  No atomics; n == 0 does nothing. */
int demfi_rgb_lut3d(const uint8_t* src, const int64_t* offsets, const int64_t* offsets_dev, int n, int h, int w, int depth,
                    const uint16_t* inv_in, int cube_n, const uint16_t* cube, const uint32_t* axis_table, int cube_in_lds, uint8_t* dst,
                    int64_t dst_stride, void* stream);

/* ---- tiles of large frames (csrc/tile.hip) --------------------------------------------------------------------------
 * Byte movers of the tiled clip pipeline; the numpy definition is demfi_amd/tiling.py (crop_np / stitch_np).  A plan has n_tiles
 * tiles of ONE size th x tw inside the h x w frame (uint8 [h,w,3]; any h, w in 2..16384).  rects: 6 int32 per tile, frame
 * coordinates: the tile's source origin y0, x0, then its kept rectangle y0, x0, y1, x1 (exclusive ends), which lies inside the
 * tile.  The plan is passed twice with the same content: rects in HOST memory, checked here before anything is launched (a
 * tile that leaves the frame or keeps pixels outside itself is DEMFI_ERR_ARG), and rects_dev in DEVICE memory, read by the
 * kernels, which skip a tile that fails the same check.  One launch each, n frames per launch.
 * u8_tile_crop: frame i read at src + i*src_stride -> all its tiles, dst [n, n_tiles, th, tw, 3].
 * u8_tile_stitch: tile j of frame i is read at base + src_offsets[i*n_tiles + j] ([th,tw,3]) and its kept rectangle written into
 * the frame at dst + dst_offsets[i] (int64 byte offsets in DEVICE memory, any order; source repeats allowed).  The kept
 * rectangles of a plan partition the frame, so every byte of a frame is written once and nothing outside the frames is. */
int demfi_u8_tile_crop(const uint8_t* src, int64_t src_stride, uint8_t* dst, int n, int h, int w, int th, int tw, int n_tiles,
                       const int32_t* rects, const int32_t* rects_dev, void* stream);
int demfi_u8_tile_stitch(const uint8_t* base, const int64_t* src_offsets, uint8_t* dst, const int64_t* dst_offsets, int n, int h, int w,
                         int th, int tw, int n_tiles, const int32_t* rects, const int32_t* rects_dev, void* stream);

/* ---- on-GPU evaluation ------------------------------------------------------------
 * psnr (utils.py:652-660) and MATLAB-style 11x11 Gaussian ssim (utils.py:663-705) of one predicted frame against its
 * target as test() computes them (main.py:762-770): pred is rounded after denorm255_np, the target is not (round_gt = 0)
 * or is (round_gt = 1); fp64 arithmetic.  pred / gt: planar fp32 [3, ., .] in [-1,1] with explicit row / channel strides
 * (elements), so a crop of a padded buffer is a view.  workspace: demfi_eval_workspace_bytes(h, w) bytes;
 * out3 (device): {psnr dB (inf when identical), ssim, mse}.  Deterministic (fixed-order reductions). */
int64_t demfi_eval_workspace_bytes(int h, int w);
int demfi_eval_frame(const float* pred, int64_t pred_row_stride, int64_t pred_ch_stride, const float* gt,
                     int64_t gt_row_stride, int64_t gt_ch_stride, int h, int w, int round_gt, double* workspace,
                     double* out3, void* stream);

/* ---- PNG codec of the clip I/O edge (host only, thread-safe) -------------------------
 * Counterpart of cv2.imread (utils.py:583-593) / cv2.imwrite (main.py:1165-1178) on zlib: uint8 [h,w,3] images in cv2's
 * B,G,R order, `stride` bytes per row.  decode: 8/16-bit gray / RGB / palette / +alpha, non-interlaced -> BGR8 (what
 * cv2.imread(path) returns); encode: 8-bit RGB, zlib `level` 0..9, filter -1 = adaptive (libpng's heuristic) or 0..4 (1 = Sub, OpenCV's default),
 * strategy -1 = Z_RLE at level <= 3 (OpenCV's default) or a zlib strategy constant. */
int64_t demfi_png_encode_bound(int h, int w);
int demfi_png_encode(const uint8_t* bgr, int h, int w, int64_t stride, int level, int filter, int strategy, uint8_t* out,
                     int64_t out_cap, int64_t* out_bytes);
int demfi_png_info(const uint8_t* data, int64_t n, int* h, int* w);
int demfi_png_decode(const uint8_t* data, int64_t n, uint8_t* bgr, int64_t stride, int h_expect, int w_expect);

/* ---- convolution descriptor builder (host only) ---------------------------------------------------
 * The ONE implementation of the layout logic behind demfi_conv: packs the logical input-channel concatenation
 * (replaces torch.cat) into LDS chunks, routes output channels to destination slices, repacks the weights.
 * Two-call pattern: with wpack == NULL only *wpack_bytes and *cout_pad are written. */
typedef struct demfi_conv_src {
    demfi_view v;           /* first channel of the piece                                               */
    int32_t fat;            /* 1: NHWC view of the path dtype (vector loads), 0: generic (planar fp32 ...) */
    int32_t up_shift;       /* 1: read through a nearest-neighbour x2 upsample                          */
    int32_t nch;            /* channels of the piece                                                    */
    int32_t _pad;
    const int32_t* cin;     /* [nch] original input channel of each channel, -1 = unused (zero weights)  */
} demfi_conv_src;

typedef struct demfi_conv_dst {
    demfi_view dst, res, aux;   /* res / aux: ptr == NULL when absent                                   */
    int32_t act, mode, scale, dy, dx;
    int32_t n;              /* output channels routed to this destination                               */
    const int32_t* couts;   /* [n] original output channel of channel j of the destination slice        */
} demfi_conv_dst;

/* desc: filled except wpack / bias / zero_page (the caller places the blobs and sets the pointers).
 * wpack: *wpack_bytes bytes; bias_packed: *cout_pad floats. H, W: OUTPUT size. */
int demfi_conv_build(int dtype, int H, int W, int stride, int batch, const float* w_oihw, const float* bias,
                     int cout, int cin, int kh, int kw, const demfi_conv_src* srcs, int n_srcs,
                     const demfi_conv_dst* dsts, int n_dsts, demfi_conv* desc, void* wpack, int64_t* wpack_bytes,
                     float* bias_packed, int32_t* cout_pad);

/* ---- forward context: the launch plan of DeMFInet.forward (DeMFInet.py:46-179) behind the C ABI -------
 * A context owns NO device memory: the caller allocates demfi_workspace_bytes() bytes (zero-filled) and binds them.
 * Inside the workspace: [packed weights + biases (one flat blob: the buffer a multi-GPU launch may broadcast) |
 * descriptors | n_trunk trunk buffer sets | n_trunk * n_ctx per-t buffer sets].  Since ABI v7 the big activation buffers of a set
 * are planned by liveness and share an arena (buffers that are never alive together occupy the same bytes; the workspace of the
 * 720p x8 configuration with 3 x 7 sets: 87.5 -> 36.1 GB): the named inputs / outputs of demfi_ctx_buffer ("x", "t", "sink",
 * "finals", "delta", "occ", "sharp1", "overlay", "ffo", "aF", "F01", "ft", "gate", "viz") own their memory, other buffers hold their value only
 * while the plan needs it.  Everything a per-t context touches lies in memory no other context touches (slots with a common context
 * stride), so the independence promised below is kept.  The liveness plan holds for executions in PLAN ORDER (trunk, head, recursions
 * 0..N-1, or prefixes of it): demfi_run_op on a single op out of order reads memory later tenants have recycled.  The scratch of a fused
 * launch (DEMFI_OP_RESBLOCK's intermediate, DEMFI_OP_GRU_ZQ's z buffer) has NO memory under the arena: such an op must not be run as its
 * constituent convolutions on the bound workspace, and demfi_ctx_bind fails if it would fuse other launches than the sizing pass did.
 * Environment DEMFI_ARENA=0: one region per buffer (debugging, isolated per-op profiling).  n_trunk / n_ctx > 1 build
 * independent buffer sets so that a scheduler can overlap the trunk of window w+1 with the time instants of window w,
 * and several time instants of one window on different streams (results do not depend on it).
 * Re-entrant per context; one context per (GPU, frame size, dtype). */
typedef struct demfi_ctx demfi_ctx;

typedef struct demfi_hparams {           /* DeMFInet.py:17-21, 32, 42, 326, 328; main.py:88-101 defaults */
    int32_t nf;                          /* 64 (only value the kernels are built for)                    */
    int32_t scale_factor;                /* 2                                                            */
    int32_t num_resb_facfb;              /* 5                                                            */
    int32_t num_resb_dec;                /* 5                                                            */
    int32_t shared_fgac;                 /* 1                                                            */
    int32_t fgac_rr, fgac_sr;            /* 0, 0: the radii hard-coded at DeMFInet.py:401-402 (generalised FGAC when > 0) */
    int32_t flags;                       /* bit 0: generalised FGAC index map (0 = as the reference code computes it, 1 = pixel-centred);
                                            bit 1 (DEMFI_HP_EXTRAS, ABI v8): also compute the maps of the reference's visualisation /
                                            training return tuples (DeMFInet.py:167-176, 454-496) into the trunk buffer "viz"        */
} demfi_hparams;
#define DEMFI_HP_FGAC_CENTRED 1
#define DEMFI_HP_EXTRAS       2

enum demfi_op_kind {
    DEMFI_OP_CONV = 0, DEMFI_OP_PACK = 1, DEMFI_OP_S2D = 2, DEMFI_OP_OVERLAY = 3, DEMFI_OP_FGAC = 4, DEMFI_OP_GATE = 5,
    DEMFI_OP_CFR = 6, DEMFI_OP_WARP = 7, DEMFI_OP_FGAC_WINDOW = 8, DEMFI_OP_AVG_POOL = 9,
    DEMFI_OP_RESBLOCK = 10,     /* fused residual block: conv = descriptor of conv1, nch = descriptor of conv2 (demfi_resblock3x3_c64) */
    DEMFI_OP_GRU_R = 11,        /* reset gate of a SepConvGRU half-step: conv = descriptor of convr (demfi_gru_r)                        */
    DEMFI_OP_GRU_ZQ = 12,       /* update gate + candidate + blend: conv = descriptor of convz, nch = descriptor of convq (demfi_gru_zq) */
    DEMFI_OP_VIZ = 13           /* visualisation extras (DEMFI_HP_EXTRAS): conv = 0 channel mean of |a - b| (b optional) -> plane p[0];
                                   1 min-max normalisation of plane p[0] in place (scratch p[1]); 2 plane p[0] = 1 - plane p[1]           */
};
enum demfi_segment { DEMFI_SEG_TRUNK = 0, DEMFI_SEG_T_HEAD = 1, DEMFI_SEG_ITER = 2,     /* TRUNK: ops 0, 1 = s2d, overlay (the prologue demfi_ingest_u8 replaces) */
                     DEMFI_SEG_TB_HEAD = 3, DEMFI_SEG_TB_ITER = 4 };                     /* the batched per-t plan of demfi_forward_tb (context index ignored) */

/* One launch of the plan (introspection for tests / per-launch profiling; pointers are already bound). */
typedef struct demfi_op {
    int32_t kind;           /* demfi_op_kind                                                             */
    int32_t conv;           /* CONV: descriptor index (demfi_ctx_conv_desc); FGAC_WINDOW: rr; AVG_POOL: sr; RESBLOCK: conv1's descriptor */
    int32_t nch;            /* PACK: channels (multiple of 8); WARP / FGAC / GATE: C; RESBLOCK: conv2's descriptor */
    int32_t _pad;           /* FGAC_WINDOW: index map (0 reference code, 1 pixel-centred)                */
    int64_t macs;           /* CONV: algorithmic multiply-accumulates of the launch                      */
    demfi_view a, b, o;     /* WARP: A, B, out; FGAC: src, -, out; GATE: source, e, out; PACK: o = dst     */
    const void* p[32];      /* PACK: plane pointers; WARP: fa, fb, logit, occ_out, pack8 (or NULL); FGAC: flow; GATE: w;
                               CFR: flow01, flow10, acc, out; S2D / OVERLAY: x, out; all: t where needed  */
    const void* t;          /* device fp32 time instant (CFR, WARP)                                      */
    char name[64];
    demfi_batch bt;         /* batched plan: nb > 1 = ONE launch for the nb per-t contexts (CFR, WARP, PACK)   */
} demfi_op;

int     demfi_ctx_create(int H, int W, int max_updates, int dtype, const demfi_hparams* hp /* NULL = defaults */,
                         int n_trunk, int n_ctx, demfi_ctx** out);
int     demfi_ctx_destroy(demfi_ctx* ctx);
/* name: state_dict key ("FF_RDB_Module.SFENet1.weight" ...), host fp32, shape as in the state_dict (Conv3d weights
 * [cout,cin,1,3,3] accepted).  All 260 (270 non-shared) tensors must be loaded before demfi_ctx_bind. */
int     demfi_load_weight(demfi_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
int64_t demfi_ctx_workspace_bytes(const demfi_ctx* ctx);
/* Size without a context: same number as a context created with these arguments reports. */
int64_t demfi_workspace_bytes(int H, int W, int max_updates, int dtype, int n_trunk, int n_ctx);
/* Builds the plan into `workspace` (device memory, zero-filled by the caller; on_host != 0: host memory, nothing is
 * launched -- the CPU plan tests) and uploads weights + descriptors on `stream` (synchronises it before returning). */
int     demfi_ctx_bind(demfi_ctx* ctx, void* workspace, int64_t bytes, int on_host, void* stream);
/* Region of the workspace holding the packed weights (offset, bytes): identical on every rank after a broadcast. */
int     demfi_ctx_weight_region(const demfi_ctx* ctx, int64_t* offset, int64_t* bytes);
/* Named buffer of trunk context `trunk` / per-t context `c` (c = -1: trunk buffers): byte offset inside the workspace,
 * element kind (0 path dtype NHWC [B,h,w,C], 1 fp32 planar [C,h,w], 2 int64 raw) and dims[4].  Names: "x" (input
 * [3,4,H,W] fp32), "overlay", "ffo"; per-t: "t", "sharp1" (S0',S1',St' = D1 frames, 9 planes), "finals" ([N][3 frames][3]),
 * "delta" ([N+1][5]: flow_t0, flow_t1, occ logit), "occ" ([N+1]) ... every buffer of the plan is addressable. */
int     demfi_ctx_buffer(const demfi_ctx* ctx, int trunk, int c, const char* name, int64_t* offset, int32_t* kind,
                         int32_t dims[4]);
/* uint8 boundary of a context.  demfi_ingest_u8: 4 BGR uint8 [h,w,3] device frames (B0,B1,
 * B-1,B2; HOST array of 4 device pointers) -> the context's x / s2d / overlay buffers (normalise + reflect pad + pixel
 * reshuffle in one kernel); follow it with demfi_forward_trunk_body.  The per-t context's buffer "sink" is a
 * demfi_u8_sink record: fill it (device memory) before demfi_forward_t and the last layer writes uint8 frames directly. */
int     demfi_ingest_u8(demfi_ctx* ctx, int trunk, const uint8_t* const* frames, int h, int w, void* stream);
/* the same for 4 BGR uint16 [h,w,3] frames at bit depth `depth` (demfi_u16_ingest) */
int     demfi_ingest_u16(demfi_ctx* ctx, int trunk, const uint16_t* const* frames, int h, int w, int depth, void* stream);
/* the same for the h x w rectangle at (y0, x0) of 4 BGR uint16 [fh,fw,3] frames (demfi_u16_ingest_rect): a tile read in place */
int     demfi_ingest_u16_rect(demfi_ctx* ctx, int trunk, const uint16_t* const* frames, int fh, int fw, int y0, int x0, int h, int w,
                              int depth, void* stream);
int     demfi_forward_trunk_body(demfi_ctx* ctx, int trunk, void* stream);
/* t-independent segment (FF_RDB + FAC-FB, DeMFInet.py:59, 74) of trunk context `trunk`; x: device fp32 [3,4,H,W]
 * copied into the context's input buffer first, or NULL when the caller already filled buffer "x". */
int     demfi_forward_trunk(demfi_ctx* ctx, int trunk, const float* x, void* stream);
/* per-t segment (DeMFInet.py:63-165) of per-t context c reading trunk context `trunk`; t is read from buffer "t". */
int     demfi_forward_t(demfi_ctx* ctx, int trunk, int c, int n_updates, void* stream);
/* The same per-t segment for ALL n_ctx per-t contexts of trunk set `trunk` as one launch sequence: every convolution runs
 * once over batch x n_ctx images (the copies of a per-t buffer are contiguous in the workspace: copy c of buffer b sits
 * c * stride(b) bytes behind copy 0, see demfi_ctx_buffer), the point-wise kernels once per context.  Context c reads its
 * own "t" and "sink" buffers; results are bit-identical to n_ctx calls of demfi_forward_t.  The time instants of a window
 * are independent given the trunk (DeMFInet.py:63-165 runs once per t in the reference's loop, main.py:1121-1178): at
 * x8 the 7 instants of a window are one batch, which takes the launch tails / pipeline fill of the small per-t grids
 * out of the picture.  n_ctx >= 2. */
int     demfi_forward_tb(demfi_ctx* ctx, int trunk, int n_updates, void* stream);
/* demfi_forward_tb for a consumer of the LAST recursion's frames only -- which is what the reference's inference pipelines
 * are (utils.py:1430-1434 "considering list of final", main.py:798, 1153: Sharps_final[-1]).  The pixel-flow warp + D2 tail of
 * a recursion (DeMFInet.py:146-165) feeds nothing but that recursion's Sharps_final entry (the recursion state is F_rec and the
 * flow / occlusion logits, 130-137), so it is run for recursion n_updates - 1 only: "finals" / "occ" of the earlier recursions
 * are NOT written, everything else (flows, logits, the final frames, the uint8 sink) is bit-identical to demfi_forward_tb. */
int     demfi_forward_tb_final(demfi_ctx* ctx, int trunk, int n_updates, void* stream);
/* introspection / per-launch execution */
int     demfi_ctx_num_ops(const demfi_ctx* ctx, int segment, int trunk, int c, int iter);
int     demfi_ctx_get_op(const demfi_ctx* ctx, int segment, int trunk, int c, int iter, int index, demfi_op* out);
int     demfi_ctx_num_convs(const demfi_ctx* ctx);
const demfi_conv* demfi_ctx_conv_desc(const demfi_ctx* ctx, int index);          /* host copy */
/* The kernel demfi_conv2d runs a descriptor on (decided from the descriptor alone).  Every owner but NARROW_THIN and GENERAL wants its
 * weights packed with cout_perm. */
enum demfi_owner { DEMFI_OWNER_SEP = 0, DEMFI_OWNER_WSTREAM7 = 1, DEMFI_OWNER_WS2 = 2, DEMFI_OWNER_WSTREAM3 = 3, DEMFI_OWNER_C64 = 4,
                   DEMFI_OWNER_NARROW_NHWC = 5, DEMFI_OWNER_NARROW_THIN = 6, DEMFI_OWNER_GENERAL = 7 };
int     demfi_conv_owner(const demfi_conv* desc);
int     demfi_run_op(demfi_ctx* ctx, const demfi_op* op, void* stream);

/* ---- single-call operators behind the C ABI (ABI v7; SURVEY.md section 8b: demfi_gru_sep / demfi_fgac) -----------------------------
 * SepConvGRU (DeMFInet.py:827-857: h' = GRU_5x1(GRU_1x5(h, x), x)) and FGAC at its hard-coded radii rr = sr = 0 (DeMFInet.py:361-452:
 * conv_ref_k -> bilinear sample at the absolute flow coordinates -> fusion -> gate -> w source + (1 - w) E_s) as contexts of their own,
 * for a host that swaps ONE module of the reference network.  An operator context is a demfi_ctx whose only segment is the operator:
 * the whole context API applies -- demfi_load_weight with the reference module's own keys ("convz1.weight" ... "convq2.bias";
 * "conv_ref_k.*", "conv_source_k.*" (accepted, dead at rr = 0), "fusion.*", "w_gen.*", "w_gen_2.*"), demfi_ctx_workspace_bytes,
 * demfi_ctx_bind (caller-owned zero-filled workspace), demfi_ctx_buffer(ctx, 0, -1, name, ...) for the NHWC [batch,H,W,64] buffers of the
 * path dtype ("h", "x", "out" / "ref", "source", "out") and the planar fp32 ones ("flow" [batch,2,H,W], "w" [batch,1,H,W] = the gate),
 * demfi_ctx_num_ops / demfi_ctx_get_op on DEMFI_SEG_TRUNK, demfi_ctx_destroy -- and demfi_operator_run launches it (4 convolutions
 * for the GRU: z | r fused and q per direction; 4 convolutions + one gather and one blend per image for FGAC). */
int demfi_gru_sep_create(int batch, int H, int W, int dtype, demfi_ctx** out);
int demfi_fgac_create(int batch, int H, int W, int dtype, demfi_ctx** out);
int demfi_operator_run(demfi_ctx* ctx, void* stream);

/* ---- hipGraph capture of a launch sequence ------------------------------------------------------ */
int demfi_graph_begin(void* stream);
int demfi_graph_end(void* stream, void** graph_exec_out);
int demfi_graph_launch(void* graph_exec, void* stream);
int demfi_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* DEMFI_HIP_H */
