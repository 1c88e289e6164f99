// YUV 4:2:0 <-> BGR uint8 colour conversion of the Y4M stream edge (demfi_amd/video.py), the default path, and the SAD of its
// scene-cut detection over either sample type.
//
// The definition is the numpy pair yuv420_to_bgr_np / bgr_to_yuv420_np in demfi_amd/y4m.py; these kernels match it bit for
// bit.  Integer arithmetic only: the d = 8 coefficients of yuv_common.h (Q16), int32 accumulators, ONE round-half-up, clamp to
// [0, 255].
//   upsampling (YUV -> BGR): chroma kept in 1/16 units -- 420jpeg: 9/3/3/1 over the 2x2 nearest chroma samples; 420mpeg2:
//     co-sited horizontally (even x: the sample, odd x: 1/2 + 1/2), centred vertically (3/4 + 1/4); neighbours clamp to the edge;
//   downsampling (BGR -> YUV, always 420jpeg): a 2x2 box over the full-resolution Q16 Cb / Cr, rounded once; at an odd edge the
//     clamped neighbour repeats the pixel that exists, which is the mean of the 2 or 1 pixels there.
//
// Memory-bound on bytes: a lane owns a strip of 8 luma pixels x 2 rows (one chroma row): Y as one 8-byte access per row, the
// 24 bytes of BGR per row as three 8-byte accesses, 4 bytes per chroma plane.  Strips that are cut by the right edge or whose
// rows are not 8-byte aligned (widths that are not a multiple of 8) take the byte path; the data are the same.
//
// These kernels were shaped by hand around packed 64-bit words of bytes (see sat_shr and the strip macro below), so they keep byte
// helpers of their own -- load8 / store8 / load_c6 and the uint64_t overloads of load_bgr8 / store_bgr8 -- beside the int-array
// accessors of yuv_common.h that every other kernel of the edge uses (yuv_family.hip).
#include "yuv_common.h"

namespace {

// What the 8-bit 4:2:0 kernels take: the d = 8 coefficients (Q16; chroma arrives in 1/16 units -> one shift by 20) without the
// fields that are constants at 8 bits, so that the kernels' argument lists are what they were shaped around.
struct ToBgr8 {
    int cy, r_cr, g_cb, g_cr, b_cb, yoff;
};
struct ToYuv8 {                       // Q16 over 8-bit B, G, R
    int y_r, y_g, y_b, cb_r, cb_g, cb_b, cr_r, cr_g, cr_b, yoff;
};

ToBgr8 to_bgr_coefs8(int matrix, int full)
{
    const ToBgr c = to_bgr_coefs(matrix, full, 8);
    return ToBgr8{c.cy, c.r_cr, c.g_cb, c.g_cr, c.b_cb, c.yoff};
}

ToYuv8 to_yuv_coefs8(int matrix, int full)
{
    const ToYuv c = to_yuv_coefs(matrix, full, 8);
    return ToYuv8{c.y_r, c.y_g, c.y_b, c.cb_r, c.cb_g, c.cb_b, c.cr_r, c.cr_g, c.cr_b, c.yoff};
}

// clamp255(acc >> S), written as a clamp of the accumulator and then the shift: the shift-then-saturate form is matched to
// v_ashr_pk_u8_i32 on gfx950, which packs two results into the low half of a register and -- as the code came out -- left the
// upper half's old bits in place, to be OR-ed into the neighbouring bytes of the packed word.  Same value for every acc.
// (sat_shr<S>(acc), S a constant shift, is this one; sat_shr<A>(acc, sh, lim), A an accumulator type, is yuv_common.h's.)
template <int S> __device__ __forceinline__ int sat_shr(int acc) { return min(max(acc, 0), (256 << S) - 1) >> S; }

// 8 bytes row[x0 .. x0+7]; indices past the right edge repeat row[w-1]
__device__ __forceinline__ uint64_t load8(const uint8_t* row, int x0, int w)
{
    const uint8_t* p = row + x0;
    if (x0 + 8 <= w && ((uintptr_t)p & 7) == 0) return *gcp<uint64_t>(p);
    uint64_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v |= (uint64_t)gcp<uint8_t>(row)[min(x0 + i, w - 1)] << (8 * i);
    return v;
}

// store the first n (<= 8) bytes of v at p
__device__ __forceinline__ void store8(uint8_t* p, uint64_t v, int n)
{
    if (n >= 8 && ((uintptr_t)p & 7) == 0) { *gp<uint64_t>(p) = v; return; }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < n) gp<uint8_t>(p)[i] = (uint8_t)(v >> (8 * i));
}

// 6 chroma samples c0-1 .. c0+4 of one row, clamped to [0, cw-1]
__device__ __forceinline__ void load_c6(const uint8_t* row, int c0, int cw, int* c)
{
    c[0] = gcp<uint8_t>(row)[max(c0 - 1, 0)];
    const uint8_t* p = row + c0;
    if (c0 + 4 <= cw && ((uintptr_t)p & 3) == 0) {
        const uint32_t v = *gcp<uint32_t>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[1 + i] = (v >> (8 * i)) & 0xff;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) c[1 + i] = gcp<uint8_t>(row)[min(c0 + i, cw - 1)];
    }
    c[5] = gcp<uint8_t>(row)[min(c0 + 4, cw - 1)];
}

// 24 bytes of 8 BGR pixels (3 words); n = pixels inside the frame
__device__ __forceinline__ void store_bgr8(uint8_t* p, const uint64_t* q, int n)
{
    if (n >= 8 && ((uintptr_t)p & 7) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) gp<uint64_t>(p)[i] = q[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < 24; ++i)                   // edge / unaligned strip: constant byte positions, guarded
        if (i < 3 * n) gp<uint8_t>(p)[i] = (uint8_t)(q[i >> 3] >> (8 * (i & 7)));
}

__device__ __forceinline__ void load_bgr8(const uint8_t* row, int x0, int w, uint64_t* q)
{
    const uint8_t* p = row + 3 * x0;
    if (x0 + 8 <= w && ((uintptr_t)p & 7) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) q[i] = gcp<uint64_t>(p)[i];
        return;
    }
    q[0] = q[1] = q[2] = 0;
#pragma unroll
    for (int px = 0; px < 8; ++px) {               // past the right edge: the last pixel again
        const int x = min(x0 + px, w - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int b = 3 * px + ch;
            q[b >> 3] |= (uint64_t)gcp<uint8_t>(row)[3 * x + ch] << (8 * (b & 7));
        }
    }
}

__device__ __forceinline__ int byte_of(const uint64_t* q, int b) { return (int)((q[b >> 3] >> (8 * (b & 7))) & 0xff); }

// one lane: chroma row cy (luma rows 2cy, 2cy+1) x luma columns x0 .. x0+7 of one frame
__global__ __launch_bounds__(NT) void yuv420_to_bgr_kernel(const uint8_t* __restrict__ src, int64_t src_stride, uint8_t* __restrict__ dst,
                                                          int64_t dst_stride, int n, int h, int w, int mpeg2, ToBgr8 k)
{
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1, ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ch * ns) return;
    const int cy = id / ns, x0 = (id - cy * ns) * SX, c0 = x0 >> 1;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* Y = src + (int64_t)f * src_stride;
        const uint8_t* planes[2] = {Y + (int64_t)h * w, Y + (int64_t)h * w + (int64_t)ch * cw};
        // vertical 3/4 + 1/4 (both sitings are centred vertically): V[r][plane][i], weight 4
        int V[2][2][6];
        for (int pl = 0; pl < 2; ++pl) {
            int cm[6], c_[6], cp[6];
            load_c6(planes[pl] + (int64_t)max(cy - 1, 0) * cw, c0, cw, cm);
            load_c6(planes[pl] + (int64_t)cy * cw, c0, cw, c_);
            load_c6(planes[pl] + (int64_t)min(cy + 1, ch - 1) * cw, c0, cw, cp);
            for (int i = 0; i < 6; ++i) {
                V[0][pl][i] = 3 * c_[i] + cm[i];
                V[1][pl][i] = 3 * c_[i] + cp[i];
            }
        }
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * cy + r;
            if (y >= h) break;
            const uint64_t yv8 = load8(Y + (int64_t)y * w, x0, w);
            uint64_t q[3] = {0, 0, 0};
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                const int li = (px >> 1) + 1;      // V index of the pixel's own chroma sample
                int u[2];
                for (int pl = 0; pl < 2; ++pl) {
                    const int* v = V[r][pl];
                    if (mpeg2) u[pl] = (px & 1) ? 2 * (v[li] + v[li + 1]) : 4 * v[li];
                    else u[pl] = 3 * v[li] + ((px & 1) ? v[li + 1] : v[li - 1]);
                }
                const int yy = (((int)(yv8 >> (8 * px)) & 0xff) - k.yoff) * 16;
                const int cb = u[0] - 128 * 16, cr = u[1] - 128 * 16;
                const int R = sat_shr<20>(k.cy * yy + k.r_cr * cr + (1 << 19));
                const int G = sat_shr<20>(k.cy * yy + k.g_cb * cb + k.g_cr * cr + (1 << 19));
                const int B = sat_shr<20>(k.cy * yy + k.b_cb * cb + (1 << 19));
                const int b = 3 * px;
                q[b >> 3] |= (uint64_t)B << (8 * (b & 7));
                q[(b + 1) >> 3] |= (uint64_t)G << (8 * ((b + 1) & 7));
                q[(b + 2) >> 3] |= (uint64_t)R << (8 * ((b + 2) & 7));
            }
            store_bgr8(dst + (int64_t)f * dst_stride + ((int64_t)y * w + x0) * 3, q, w - x0);
        }
    }
}

// one lane of one frame: BGR frame S -> 4:2:0 payload Y, luma rows 2cy, 2cy+1 (the second clamped to h-1 at an odd bottom edge) x
// columns x0 .. x0+7 -> 16 Y, 4 Cb, 4 Cr.  Shared by the strided and the gathered conversion as a statement macro, not as an
// inline function: the inlined call changed the register allocation of bgr_to_yuv420_kernel, the macro keeps its
// instruction stream as it was.  Uses cy, x0, c0, h, w, cw, ch, k of the enclosing kernel.
#define DEMFI_BGR_TO_YUV420_STRIP(S_, Y_)                                                                \
    do {                                                                                                 \
    const uint8_t* Sp = (S_);                                                                               \
    uint8_t* Yp = (Y_);                                                                                     \
    int cbs[4] = {0, 0, 0, 0}, crs[4] = {0, 0, 0, 0};                                                    \
    for (int r = 0; r < 2; ++r) {                                                                        \
        const int y = min(2 * cy + r, h - 1);                                                            \
        uint64_t q[3];                                                                                   \
        load_bgr8(Sp + (int64_t)y * w * 3, x0, w, q);                                                     \
        uint64_t yo = 0;                                                                                 \
_Pragma("unroll")                                                                                          \
        for (int px = 0; px < SX; ++px) {                                                                \
            const int B = byte_of(q, 3 * px), G = byte_of(q, 3 * px + 1), R = byte_of(q, 3 * px + 2);    \
            const int yv = sat_shr<16>(k.y_r * R + k.y_g * G + k.y_b * B + (k.yoff << 16) + (1 << 15));  \
            yo |= (uint64_t)yv << (8 * px);                                                              \
            cbs[px >> 1] += k.cb_r * R + k.cb_g * G + k.cb_b * B;                                        \
            crs[px >> 1] += k.cr_r * R + k.cr_g * G + k.cr_b * B;                                        \
        }                                                                                                \
        if (2 * cy + r < h) store8(Yp + (int64_t)y * w + x0, yo, w - x0);                                 \
    }                                                                                                    \
    uint32_t cbo = 0, cro = 0;                                                                           \
    for (int i = 0; i < 4; ++i) {                                                                        \
        cbo |= (uint32_t)sat_shr<18>(cbs[i] + (128 << 18) + (1 << 17)) << (8 * i);                       \
        cro |= (uint32_t)sat_shr<18>(crs[i] + (128 << 18) + (1 << 17)) << (8 * i);                       \
    }                                                                                                    \
    uint8_t* pcb = Yp + (int64_t)h * w + (int64_t)cy * cw + c0;                                           \
    uint8_t* pcr = pcb + (int64_t)ch * cw;                                                               \
    if (c0 + 4 <= cw && ((uintptr_t)pcb & 3) == 0 && ((uintptr_t)pcr & 3) == 0) {                        \
        *gp<uint32_t>(pcb) = cbo;                                                                        \
        *gp<uint32_t>(pcr) = cro;                                                                        \
    } else {                                                                                             \
_Pragma("unroll")                                                                                          \
        for (int i = 0; i < 4; ++i) {                                                                    \
            if (i < cw - c0) {                                                                           \
                gp<uint8_t>(pcb)[i] = (uint8_t)(cbo >> (8 * i));                                         \
                gp<uint8_t>(pcr)[i] = (uint8_t)(cro >> (8 * i));                                         \
            }                                                                                            \
        }                                                                                                \
    }                                                                                                    \
    } while (0)

__global__ __launch_bounds__(NT) void bgr_to_yuv420_kernel(const uint8_t* __restrict__ src, int64_t src_stride, int group,
                                                          int64_t group_stride, uint8_t* __restrict__ dst, int64_t dst_stride, int n,
                                                          int h, int w, ToYuv8 k)
{
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1, ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ch * ns) return;
    const int cy = id / ns, x0 = (id - cy * ns) * SX, c0 = x0 >> 1;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const int g = f / group;
        const uint8_t* S = src + (int64_t)g * group_stride + (int64_t)(f - g * group) * src_stride;
        DEMFI_BGR_TO_YUV420_STRIP(S, dst + (int64_t)f * dst_stride);
    }
}

// frame f read at base + offs[f]: one (wave-uniform) offset load per frame, the rest as bgr_to_yuv420_kernel
__global__ __launch_bounds__(NT) void bgr_to_yuv420_gather_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs,
                                                                 uint8_t* __restrict__ dst, int64_t dst_stride, int n, int h, int w,
                                                                 ToYuv8 k)
{
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1, ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ch * ns) return;
    const int cy = id / ns, x0 = (id - cy * ns) * SX, c0 = x0 >> 1;
    for (int f = blockIdx.y; f < n; f += gridDim.y)
        DEMFI_BGR_TO_YUV420_STRIP(base + offs[f], dst + (int64_t)f * dst_stride);
}

// ---- the SAD of scene-cut detection, over either sample type ------------------------------------------------------------------
__device__ __forceinline__ uint32_t sad_one(uint8_t x, uint8_t y, uint32_t acc) { return __builtin_amdgcn_sad_u8(x, y, acc); }
__device__ __forceinline__ uint32_t sad_one(uint16_t x, uint16_t y, uint32_t acc) { return __builtin_amdgcn_sad_u16(x, y, acc); }

// 16 bytes at a (16-byte aligned) against 16 at b (sample-aligned, which global memory serves): four v_sad_u8 / v_sad_u16
__device__ __forceinline__ uint32_t sad_vec(const uint8_t* a, const uint8_t* b, uint32_t acc)
{
    const u4_t x = *(const DEMFI_GLOBAL u4_t*)a, y = *(const DEMFI_GLOBAL u4_a1*)b;
    acc = __builtin_amdgcn_sad_u8(x.x, y.x, acc);
    acc = __builtin_amdgcn_sad_u8(x.y, y.y, acc);
    acc = __builtin_amdgcn_sad_u8(x.z, y.z, acc);
    return __builtin_amdgcn_sad_u8(x.w, y.w, acc);
}

__device__ __forceinline__ uint32_t sad_vec(const uint16_t* a, const uint16_t* b, uint32_t acc)
{
    const u4_t x = *(const DEMFI_GLOBAL u4_t*)a, y = *(const DEMFI_GLOBAL u4_a2*)b;
    acc = __builtin_amdgcn_sad_u16(x.x, y.x, acc);
    acc = __builtin_amdgcn_sad_u16(x.y, y.y, acc);
    acc = __builtin_amdgcn_sad_u16(x.z, y.z, acc);
    return __builtin_amdgcn_sad_u16(x.w, y.w, acc);
}

// SAD of frame pair f: |a - b| summed over `samples` samples of T, a = base + a_offs[f], b = base + b_offs[f] (offsets in samples:
// any sample alignment of either).  VS = 16 / sizeof(T) samples make one 16-byte vector.  The samples before a's first 16-byte
// boundary (head) and after its last one (tail) go to the first VS lanes of block x = 0, one sample each; the body is one vector
// per lane and step (sad_vec).  A lane's partial stays below 2^32: up to 1024 blocks a lane takes one vector, and where the grid is
// cut at 1024 blocks it takes at most ceil(samples / VS / (1024 NT)) vectors of at most VS * (2^(8 sizeof(T)) - 1) each, which
// is below 2^20 (uint8) and 2^28 (uint16) for any payload up to 2^29 samples (16384 x 16384 4:2:0 has 1.5 * 2^28).  The wave and
// block sums are 64-bit, and each block adds its sum with ONE 64-bit atomic (integer adds are exact in any order).
template <typename T>
__global__ __launch_bounds__(NT) void yuv_sad_kernel(const T* __restrict__ base, const int64_t* __restrict__ a_offs,
                                                    const int64_t* __restrict__ b_offs, int n, int64_t samples,
                                                    unsigned long long* __restrict__ sad)
{
    constexpr int LB = sizeof(T) == 2 ? 1 : 0, LV = 4 - LB, VS = 1 << LV;      // log2 of bytes per sample, of samples per vector
    __shared__ unsigned long long part[NT / 64];
    const int tid = threadIdx.x;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* a = base + a_offs[f];
        const T* b = base + b_offs[f];
        const int64_t head = min((int64_t)(((16 - ((uintptr_t)a & 15)) & 15) >> LB), samples);
        const int64_t nvec = (samples - head) >> LV;
        const int64_t tail = head + (nvec << LV);             // samples - tail < VS
        uint32_t acc = 0;
        if (blockIdx.x == 0 && tid < VS) {
            if (tid < head) acc = sad_one(gcp<T>(a)[tid], gcp<T>(b)[tid], acc);
            if (tail + tid < samples) acc = sad_one(gcp<T>(a)[tail + tid], gcp<T>(b)[tail + tid], acc);
        }
        for (int64_t v = (int64_t)blockIdx.x * NT + tid; v < nvec; v += (int64_t)gridDim.x * NT)
            acc = sad_vec(a + head + VS * v, b + head + VS * v, acc);
        unsigned long long s = acc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((tid & 63) == 0) part[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            unsigned long long t = 0;
#pragma unroll
            for (int i = 0; i < NT / 64; ++i) t += part[i];
            if (t) atomicAdd(sad + f, t);
        }
        __syncthreads();                                      // part[] is reused by the next pair
    }
}

template <typename T>
int yuv_sad(const char* fn, const T* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int64_t samples, uint64_t* sad,
            void* stream)
{
    if (!base || !a_offsets || !b_offsets || !sad || n < 0 || samples <= 0 || ((uintptr_t)base & (sizeof(T) - 1)))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL%s buffer, n=%d or %s=%lld", fn, sizeof(T) == 2 ? " or odd" : "", n,
                               sizeof(T) == 2 ? "samples" : "payload", (long long)samples);
    if (n == 0) return DEMFI_OK;
    DEMFI_HIP_CHECK(hipMemsetAsync(sad, 0, (size_t)n * sizeof(uint64_t), (hipStream_t)stream));
    const int64_t blocks = (samples * (int64_t)sizeof(T) / 16 + NT - 1) / NT;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks), (unsigned)(n < 65535 ? n : 65535));
    hipLaunchKernelGGL(yuv_sad_kernel<T>, grid, dim3(NT), 0, (hipStream_t)stream, base, a_offsets, b_offsets, n, samples,
                       (unsigned long long*)sad);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

}  // namespace

extern "C" int demfi_yuv420_to_bgr(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int n, int h, int w,
                                   int matrix, int full_range, int siting, void* stream)
{
    int st = check_args("demfi_yuv420_to_bgr", src, dst, n, h, w, 8, matrix, full_range, 1);
    if (st < 0) return st;
    const int64_t payload = payload_of(DEMFI_YUV_420, h, w);
    if (siting != DEMFI_420JPEG && siting != DEMFI_420MPEG2)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_yuv420_to_bgr: chroma siting %d", siting);
    if (n > 1 && (src_stride < payload || dst_stride < (int64_t)h * w * 3))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_yuv420_to_bgr: strides %lld / %lld below the frame sizes %lld / %lld",
                               (long long)src_stride, (long long)dst_stride, (long long)payload, (long long)h * w * 3);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(yuv420_to_bgr_kernel, grid_for(n, (h + 1) / 2, w), dim3(NT), 0, (hipStream_t)stream, src, src_stride, dst,
                       dst_stride, n, h, w, siting == DEMFI_420MPEG2 ? 1 : 0, to_bgr_coefs8(matrix, full_range));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_bgr_to_yuv420(const uint8_t* src, int64_t src_stride, int group, int64_t group_stride, uint8_t* dst,
                                   int64_t dst_stride, int n, int h, int w, int matrix, int full_range, void* stream)
{
    int st = check_args("demfi_bgr_to_yuv420", src, dst, n, h, w, 8, matrix, full_range, 1);
    if (st < 0) return st;
    const int64_t payload = payload_of(DEMFI_YUV_420, h, w);
    if (group <= 0) group = n > 0 ? n : 1;
    if (n > 1 && (dst_stride < payload || (group > 1 && src_stride < (int64_t)h * w * 3) ||
                  (n > group && group_stride < (int64_t)(group - 1) * src_stride + (int64_t)h * w * 3)))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_bgr_to_yuv420: strides %lld / %lld (group %d) / %lld below the frame sizes",
                               (long long)src_stride, (long long)group_stride, group, (long long)dst_stride);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(bgr_to_yuv420_kernel, grid_for(n, (h + 1) / 2, w), dim3(NT), 0, (hipStream_t)stream, src, src_stride, group,
                       group_stride, dst, dst_stride, n, h, w, to_yuv_coefs8(matrix, full_range));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_bgr_to_yuv420_gather(const uint8_t* base, const int64_t* src_offsets, uint8_t* dst, int64_t dst_stride, int n,
                                          int h, int w, int matrix, int full_range, void* stream)
{
    int st = check_args("demfi_bgr_to_yuv420_gather", base, dst, n, h, w, 8, matrix, full_range, 1);
    if (st < 0) return st;
    if (!src_offsets)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_bgr_to_yuv420_gather: NULL src_offsets");
    const int64_t payload = payload_of(DEMFI_YUV_420, h, w);
    if (n > 1 && dst_stride < payload)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_bgr_to_yuv420_gather: dst_stride %lld below the payload %lld",
                               (long long)dst_stride, (long long)payload);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(bgr_to_yuv420_gather_kernel, grid_for(n, (h + 1) / 2, w), dim3(NT), 0, (hipStream_t)stream, base, src_offsets, dst,
                       dst_stride, n, h, w, to_yuv_coefs8(matrix, full_range));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_yuv420_sad(const uint8_t* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int64_t payload,
                                uint64_t* sad, void* stream)
{
    return yuv_sad<uint8_t>("demfi_yuv420_sad", base, a_offsets, b_offsets, n, payload, sad, stream);
}

extern "C" int demfi_yuv420p16_sad(const uint16_t* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int64_t samples,
                                   uint64_t* sad, void* stream)
{
    return yuv_sad<uint16_t>("demfi_yuv420p16_sad", base, a_offsets, b_offsets, n, samples, sad, stream);
}
