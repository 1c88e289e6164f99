// The kernel family of the Y4M stream edge over (sample type, chroma layout), on the sample accessors of yuv_common.h: YUV 4:2:2,
// 4:4:4 and mono <-> BGR (demfi_amd/video.py --any-layout) over 8-bit samples (uint8, strides and offsets in bytes) and over 16-bit
// samples at bit depth d = 10 .. 16 (uint16 holding 0 .. peak = 2^d - 1, strides and offsets in samples; d = 8 is accepted so that
// the two sample types can be compared value for value), and 4:2:0 over 16-bit samples (--high-depth; 8-bit 4:2:0 is yuv.hip).
//
// The definition is the numpy pair yuv_to_bgr16_np / bgr16_to_yuv_np in demfi_amd/y4m.py (yuv_to_bgr_np / bgr_to_yuv_np are its
// d = 8 instance); the kernels match it bit for bit.  The matrix step is the one yuv_common.h describes, the same for every layout.
// Only the resampling differs:
//   4:2:0  up: 420jpeg 9/3/3/1 over the 2x2 nearest chroma samples; 420mpeg2 co-sited horizontally (even x: the sample, odd x:
//          1/2 + 1/2), centred vertically (3/4 + 1/4); neighbours clamp to the edge;  down (always 420jpeg): the 2x2 box over f,
//          rounded once; at an odd edge the clamped neighbour repeats the pixel that exists.
//   4:4:4  up: 16 c[y,x];  down: f rounded once.
//   4:2:2  (co-sited horizontally, no vertical filter)  up: even x: 16 c[y,x/2], odd x: 8 (c[y,cx] + c[y,min(cx+1,cw-1)]);
//          down: the [1,2,1]/4 of f[y,max(2i-1,0)], f[y,2i], f[y,min(2i+1,w-1)], rounded once.
//   mono   up: no chroma term, B = G = R;  down: Y only.
// f = the full-resolution Q(8+d) chroma centred on 0.  8-bit samples accumulate in int32 (every sum stays below 2^29), 16-bit
// samples in true 64-bit sums of 32 x 32 -> 64 bit products (v_mad_i64_i32; a Q(8+d) coefficient is below 2^27, an operand in 1/16
// units below 2^21), exact like numpy's int64.
//
// Memory-bound on bytes, so every kernel keeps the lane layout of yuv.hip: a lane owns a strip of 8 luma pixels -- of one row where
// no layout couples rows, of two rows (one chroma row) for 4:2:0 -- Y as one access of 8 samples per row, the 24 samples of BGR as
// three, chroma as one access of 8 (4:4:4) or 4 (4:2:2, 4:2:0) samples per plane and row: 8- and 4-byte accesses for uint8, 16- and
// 8-byte ones for uint16.  Strips cut by the right edge or whose rows are not aligned to the access (payloads are only
// sample-aligned) take the sample path; the data are the same.
#include "yuv_common.h"

namespace {

constexpr bool has_chroma(int layout) { return layout != DEMFI_YUV_MONO; }

// one lane: row y x luma columns x0 .. x0+7 of one frame
template <typename T, int LAYOUT>
__global__ __launch_bounds__(NT) void yuvl_to_bgr_kernel(const T* __restrict__ src, int64_t src_stride, T* __restrict__ dst,
                                                        int64_t dst_stride, int n, int h, int w, ToBgr k)
{
    typedef typename Acc<T>::type A;
    const int ns = (w + SX - 1) / SX, cw = LAYOUT == DEMFI_YUV_422 ? (w + 1) >> 1 : w;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= h * ns) return;
    const int y = id / ns, x0 = (id - y * ns) * SX;
    const A rnd = (A)1 << (k.sh - 1), lim = ((A)(k.peak + 1) << k.sh) - 1;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* Y = src + (int64_t)f * src_stride;
        int yv[8], u[2][8], o[24];                 // u: chroma in 1/16 units, centred on 0
        load_n<T, 8>(Y + (int64_t)y * w, x0, w, yv);
        if (LAYOUT == DEMFI_YUV_444) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                int c[8];
                load_n<T, 8>(Y + (int64_t)(1 + pl) * h * w + (int64_t)y * w, x0, w, c);
#pragma unroll
                for (int px = 0; px < SX; ++px) u[pl][px] = 16 * c[px] - k.mid16;
            }
        } else if (LAYOUT == DEMFI_YUV_422) {
            const int c0 = x0 >> 1;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const T* row = Y + (int64_t)h * w + (int64_t)pl * h * cw + (int64_t)y * cw;
                int c[5];                          // samples c0 .. c0+4, clamped to cw-1
                load_n<T, 4>(row, c0, cw, c);
                c[4] = gcp<T>(row)[min(c0 + 4, cw - 1)];
#pragma unroll
                for (int px = 0; px < SX; ++px)
                    u[pl][px] = ((px & 1) ? 8 * (c[px >> 1] + c[(px >> 1) + 1]) : 16 * c[px >> 1]) - k.mid16;
            }
        }
#pragma unroll
        for (int px = 0; px < SX; ++px) {
            const A ly = mul<A>(k.cy, (yv[px] - k.yoff) * 16) + rnd;
            if (has_chroma(LAYOUT)) {
                const int cb = u[0][px], cr = u[1][px];
                o[3 * px] = sat_shr<A>(ly + mul<A>(k.b_cb, cb), k.sh, lim);
                o[3 * px + 1] = sat_shr<A>(ly + mul<A>(k.g_cb, cb) + mul<A>(k.g_cr, cr), k.sh, lim);
                o[3 * px + 2] = sat_shr<A>(ly + mul<A>(k.r_cr, cr), k.sh, lim);
            } else {
                o[3 * px] = o[3 * px + 1] = o[3 * px + 2] = sat_shr<A>(ly, k.sh, lim);
            }
        }
        store_bgr8<T>(dst + (int64_t)f * dst_stride + ((int64_t)y * w + x0) * 3, o, w - x0);
    }
}

// frame f read at base + offs[f]: BGR frame -> payload, row y x columns x0 .. x0+7 -> 8 Y and 8 (4:4:4) or 4 (4:2:2) Cb, Cr; one
// (wave-uniform) offset load per frame.  4:2:2: the strip's first chroma sample also reads the pixel left of the strip.
template <typename T, int LAYOUT>
__global__ __launch_bounds__(NT) void bgr_to_yuvl_gather_kernel(const T* __restrict__ base, const int64_t* __restrict__ offs,
                                                               T* __restrict__ dst, int64_t dst_stride, int n, int h, int w, ToYuv k)
{
    typedef typename Acc<T>::type A;
    const int ns = (w + SX - 1) / SX, cw = (w + 1) >> 1;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= h * ns) return;
    const int y = id / ns, x0 = (id - y * ns) * SX;
    const int csh = LAYOUT == DEMFI_YUV_422 ? k.q + 2 : k.q;          // 4:2:2 sums weights 1 + 2 + 1
    const A ylim = ((A)(k.peak + 1) << k.q) - 1, clim = ((A)(k.peak + 1) << csh) - 1;
    const A yadd = ((A)k.yoff << k.q) + ((A)1 << (k.q - 1));
    const A cadd = ((A)k.mid << csh) + ((A)1 << (csh - 1));
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* row = base + offs[f] + (int64_t)y * w * 3;
        T* Yp = dst + (int64_t)f * dst_stride;
        int v[24], yo[8];
        A fc[2][8];                                // full-resolution chroma of the strip's pixels, centred on 0
        load_bgr8<T>(row, x0, w, v);
#pragma unroll
        for (int px = 0; px < SX; ++px) {
            const int B = v[3 * px], G = v[3 * px + 1], R = v[3 * px + 2];
            yo[px] = sat_shr<A>(mul<A>(k.y_r, R) + mul<A>(k.y_g, G) + mul<A>(k.y_b, B) + yadd, k.q, ylim);
            if (has_chroma(LAYOUT)) {
                fc[0][px] = mul<A>(k.cb_r, R) + mul<A>(k.cb_g, G) + mul<A>(k.cb_b, B);
                fc[1][px] = mul<A>(k.cr_r, R) + mul<A>(k.cr_g, G) + mul<A>(k.cr_b, B);
            }
        }
        store_n<T, 8>(Yp + (int64_t)y * w + x0, yo, w - x0);
        if (LAYOUT == DEMFI_YUV_444) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                int co[8];
#pragma unroll
                for (int px = 0; px < SX; ++px) co[px] = sat_shr<A>(fc[pl][px] + cadd, csh, clim);
                store_n<T, 8>(Yp + (int64_t)(1 + pl) * h * w + (int64_t)y * w + x0, co, w - x0);
            }
        } else if (LAYOUT == DEMFI_YUV_422) {
            const int xl = max(x0 - 1, 0), c0 = x0 >> 1;
            const int B = gcp<T>(row)[3 * xl], G = gcp<T>(row)[3 * xl + 1], R = gcp<T>(row)[3 * xl + 2];
            const A left[2] = {mul<A>(k.cb_r, R) + mul<A>(k.cb_g, G) + mul<A>(k.cb_b, B),
                               mul<A>(k.cr_r, R) + mul<A>(k.cr_g, G) + mul<A>(k.cr_b, B)};
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                int co[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)        // pixel x0 + 2i + 1 past the right edge is the last pixel again (load_bgr8)
                    co[i] = sat_shr<A>((i ? fc[pl][2 * i - 1] : left[pl]) + 2 * fc[pl][2 * i] + fc[pl][2 * i + 1] + cadd, csh, clim);
                store_n<T, 4>(Yp + (int64_t)h * w + (int64_t)pl * h * cw + (int64_t)y * cw + c0, co, cw - c0);
            }
        }
    }
}

// ---- 4:2:0 over the same accessors: a lane owns 8 luma pixels x 2 rows (one chroma row) -------------------------------------------
// 6 chroma samples c0-1 .. c0+4 of one row, clamped to [0, cw-1]
template <typename T> __device__ __forceinline__ void load_c6(const T* row, int c0, int cw, int* c)
{
    c[0] = gcp<T>(row)[max(c0 - 1, 0)];
    load_n<T, 4>(row, c0, cw, c + 1);
    c[5] = gcp<T>(row)[min(c0 + 4, cw - 1)];
}

// one lane: chroma row cy (luma rows 2cy, 2cy+1) x luma columns x0 .. x0+7 of one frame
template <typename T>
__global__ __launch_bounds__(NT) void yuv420t_to_bgr_kernel(const T* __restrict__ src, int64_t src_stride, T* __restrict__ dst,
                                                          int64_t dst_stride, int n, int h, int w, int mpeg2, ToBgr k)
{
    typedef typename Acc<T>::type A;
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1, ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ch * ns) return;
    const int cy = id / ns, x0 = (id - cy * ns) * SX, c0 = x0 >> 1;
    const A rnd = (A)1 << (k.sh - 1), lim = ((A)(k.peak + 1) << k.sh) - 1;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* Y = src + (int64_t)f * src_stride;
        const T* planes[2] = {Y + (int64_t)h * w, Y + (int64_t)h * w + (int64_t)ch * cw};
        // vertical 3/4 + 1/4 (both sitings are centred vertically): V[r][plane][i], weight 4
        int V[2][2][6];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            int cm[6], c_[6], cp[6];
            load_c6<T>(planes[pl] + (int64_t)max(cy - 1, 0) * cw, c0, cw, cm);
            load_c6<T>(planes[pl] + (int64_t)cy * cw, c0, cw, c_);
            load_c6<T>(planes[pl] + (int64_t)min(cy + 1, ch - 1) * cw, c0, cw, cp);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                V[0][pl][i] = 3 * c_[i] + cm[i];
                V[1][pl][i] = 3 * c_[i] + cp[i];
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * cy + r;
            if (y >= h) continue;                  // the odd bottom edge has no second row
            int yv[8], o[24];
            load_n<T, 8>(Y + (int64_t)y * w, x0, w, yv);
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                const int li = (px >> 1) + 1;      // V index of the pixel's own chroma sample
                int u[2];
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    const int* v = V[r][pl];
                    if (mpeg2) u[pl] = (px & 1) ? 2 * (v[li] + v[li + 1]) : 4 * v[li];
                    else u[pl] = 3 * v[li] + ((px & 1) ? v[li + 1] : v[li - 1]);
                }
                const int yy = (yv[px] - k.yoff) * 16;
                const int cb = u[0] - k.mid16, cr = u[1] - k.mid16;
                const A ly = mul<A>(k.cy, yy) + rnd;
                o[3 * px] = sat_shr<A>(ly + mul<A>(k.b_cb, cb), k.sh, lim);
                o[3 * px + 1] = sat_shr<A>(ly + mul<A>(k.g_cb, cb) + mul<A>(k.g_cr, cr), k.sh, lim);
                o[3 * px + 2] = sat_shr<A>(ly + mul<A>(k.r_cr, cr), k.sh, lim);
            }
            store_bgr8<T>(dst + (int64_t)f * dst_stride + ((int64_t)y * w + x0) * 3, o, w - x0);
        }
    }
}

// frame f read at base + offs[f]: BGR frame -> 4:2:0 payload, luma rows 2cy, 2cy+1 (the second clamped to h-1 at an odd bottom
// edge) x columns x0 .. x0+7 -> 16 Y, 4 Cb, 4 Cr (the 2x2 box over the full-resolution chroma); one (wave-uniform) offset load per frame
template <typename T>
__global__ __launch_bounds__(NT) void bgr_to_yuv420t_gather_kernel(const T* __restrict__ base, const int64_t* __restrict__ offs,
                                                                 T* __restrict__ dst, int64_t dst_stride, int n, int h, int w, ToYuv k)
{
    typedef typename Acc<T>::type A;
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1, ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ch * ns) return;
    const int cy = id / ns, x0 = (id - cy * ns) * SX, c0 = x0 >> 1;
    const A ylim = ((A)(k.peak + 1) << k.q) - 1, clim = ((A)(k.peak + 1) << (k.q + 2)) - 1;
    const A yadd = ((A)k.yoff << k.q) + ((A)1 << (k.q - 1));
    const A cadd = ((A)k.mid << (k.q + 2)) + ((A)1 << (k.q + 1));
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* Sp = base + offs[f];
        T* Yp = dst + (int64_t)f * dst_stride;
        A cbs[4] = {0, 0, 0, 0}, crs[4] = {0, 0, 0, 0};
        for (int r = 0; r < 2; ++r) {
            const int y = min(2 * cy + r, h - 1);
            int v[24], yo[8];
            load_bgr8<T>(Sp + (int64_t)y * w * 3, x0, w, v);
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                const int B = v[3 * px], G = v[3 * px + 1], R = v[3 * px + 2];
                yo[px] = sat_shr<A>(mul<A>(k.y_r, R) + mul<A>(k.y_g, G) + mul<A>(k.y_b, B) + yadd, k.q, ylim);
                cbs[px >> 1] += mul<A>(k.cb_r, R) + mul<A>(k.cb_g, G) + mul<A>(k.cb_b, B);
                crs[px >> 1] += mul<A>(k.cr_r, R) + mul<A>(k.cr_g, G) + mul<A>(k.cr_b, B);
            }
            if (2 * cy + r < h) store_n<T, 8>(Yp + (int64_t)y * w + x0, yo, w - x0);
        }
        int cbo[4], cro[4];
        for (int i = 0; i < 4; ++i) {
            cbo[i] = sat_shr<A>(cbs[i] + cadd, k.q + 2, clim);
            cro[i] = sat_shr<A>(crs[i] + cadd, k.q + 2, clim);
        }
        T* pcb = Yp + (int64_t)h * w + (int64_t)cy * cw + c0;
        store_n<T, 4>(pcb, cbo, cw - c0);
        store_n<T, 4>(pcb + (int64_t)ch * cw, cro, cw - c0);
    }
}

int check_layout(const char* fn, int layout)
{
    if (layout != DEMFI_YUV_422 && layout != DEMFI_YUV_444 && layout != DEMFI_YUV_MONO)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: layout %d (4:2:2, 4:4:4 or mono; 4:2:0 has functions of its own)", fn, layout);
    return DEMFI_OK;
}

template <typename T>
int to_bgr(const char* fn, const T* src, int64_t src_stride, T* dst, int64_t dst_stride, int n, int h, int w, int depth, int layout,
           int matrix, int full_range, void* stream)
{
    int st = check_args(fn, src, dst, n, h, w, depth, matrix, full_range, (int)sizeof(T));
    if (st == DEMFI_OK) st = check_layout(fn, layout);
    if (st < 0) return st;
    const int64_t payload = payload_of(layout, h, w);
    if (n > 1 && (src_stride < payload || dst_stride < (int64_t)h * w * 3))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: strides %lld / %lld below the frame sizes %lld / %lld", fn, (long long)src_stride,
                               (long long)dst_stride, (long long)payload, (long long)h * w * 3);
    if (n == 0) return DEMFI_OK;
    const dim3 grid = grid_for(n, h, w);
    const ToBgr k = to_bgr_coefs(matrix, full_range, depth);
    hipStream_t s = (hipStream_t)stream;
    if (layout == DEMFI_YUV_422)
        hipLaunchKernelGGL((yuvl_to_bgr_kernel<T, DEMFI_YUV_422>), grid, dim3(NT), 0, s, src, src_stride, dst, dst_stride, n, h, w, k);
    else if (layout == DEMFI_YUV_444)
        hipLaunchKernelGGL((yuvl_to_bgr_kernel<T, DEMFI_YUV_444>), grid, dim3(NT), 0, s, src, src_stride, dst, dst_stride, n, h, w, k);
    else
        hipLaunchKernelGGL((yuvl_to_bgr_kernel<T, DEMFI_YUV_MONO>), grid, dim3(NT), 0, s, src, src_stride, dst, dst_stride, n, h, w, k);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

template <typename T>
int gather(const char* fn, const T* base, const int64_t* src_offsets, T* dst, int64_t dst_stride, int n, int h, int w, int depth, int layout,
           int matrix, int full_range, void* stream)
{
    int st = check_args(fn, base, dst, n, h, w, depth, matrix, full_range, (int)sizeof(T));
    if (st == DEMFI_OK) st = check_layout(fn, layout);
    if (st < 0) return st;
    if (!src_offsets)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL src_offsets", fn);
    const int64_t payload = payload_of(layout, h, w);
    if (n > 1 && dst_stride < payload)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride %lld below the payload %lld", fn, (long long)dst_stride, (long long)payload);
    if (n == 0) return DEMFI_OK;
    const dim3 grid = grid_for(n, h, w);
    const ToYuv k = to_yuv_coefs(matrix, full_range, depth);
    hipStream_t s = (hipStream_t)stream;
    if (layout == DEMFI_YUV_422)
        hipLaunchKernelGGL((bgr_to_yuvl_gather_kernel<T, DEMFI_YUV_422>), grid, dim3(NT), 0, s, base, src_offsets, dst, dst_stride, n, h, w, k);
    else if (layout == DEMFI_YUV_444)
        hipLaunchKernelGGL((bgr_to_yuvl_gather_kernel<T, DEMFI_YUV_444>), grid, dim3(NT), 0, s, base, src_offsets, dst, dst_stride, n, h, w, k);
    else
        hipLaunchKernelGGL((bgr_to_yuvl_gather_kernel<T, DEMFI_YUV_MONO>), grid, dim3(NT), 0, s, base, src_offsets, dst, dst_stride, n, h, w, k);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

}  // namespace

extern "C" int demfi_yuvl_to_bgr(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int n, int h, int w, int layout,
                                 int matrix, int full_range, void* stream)
{
    return to_bgr<uint8_t>("demfi_yuvl_to_bgr", src, src_stride, dst, dst_stride, n, h, w, 8, layout, matrix, full_range, stream);
}

extern "C" int demfi_bgr_to_yuvl_gather(const uint8_t* base, const int64_t* src_offsets, uint8_t* dst, int64_t dst_stride, int n, int h,
                                        int w, int layout, int matrix, int full_range, void* stream)
{
    return gather<uint8_t>("demfi_bgr_to_yuvl_gather", base, src_offsets, dst, dst_stride, n, h, w, 8, layout, matrix, full_range, stream);
}

extern "C" int demfi_yuvl16_to_bgr16(const uint16_t* src, int64_t src_stride, uint16_t* dst, int64_t dst_stride, int n, int h, int w,
                                     int depth, int layout, int matrix, int full_range, void* stream)
{
    return to_bgr<uint16_t>("demfi_yuvl16_to_bgr16", src, src_stride, dst, dst_stride, n, h, w, depth, layout, matrix, full_range, stream);
}

extern "C" int demfi_bgr16_to_yuvl16_gather(const uint16_t* base, const int64_t* src_offsets, uint16_t* dst, int64_t dst_stride, int n,
                                            int h, int w, int depth, int layout, int matrix, int full_range, void* stream)
{
    return gather<uint16_t>("demfi_bgr16_to_yuvl16_gather", base, src_offsets, dst, dst_stride, n, h, w, depth, layout, matrix, full_range,
                            stream);
}

// ---- 4:2:0 at 16-bit samples (the 8-bit entry points are those of yuv.hip) -------------------------------------------------------
extern "C" int demfi_yuv420p16_to_bgr16(const uint16_t* src, int64_t src_stride, uint16_t* dst, int64_t dst_stride, int n, int h, int w,
                                        int depth, int matrix, int full_range, int siting, void* stream)
{
    int st = check_args("demfi_yuv420p16_to_bgr16", src, dst, n, h, w, depth, matrix, full_range, 2);
    if (st < 0) return st;
    const int64_t payload = payload_of(DEMFI_YUV_420, h, w);
    if (siting != DEMFI_420JPEG && siting != DEMFI_420MPEG2)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_yuv420p16_to_bgr16: chroma siting %d", siting);
    if (n > 1 && (src_stride < payload || dst_stride < (int64_t)h * w * 3))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_yuv420p16_to_bgr16: strides %lld / %lld below the frame sizes %lld / %lld samples",
                               (long long)src_stride, (long long)dst_stride, (long long)payload, (long long)h * w * 3);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(yuv420t_to_bgr_kernel<uint16_t>, grid_for(n, (h + 1) / 2, w), dim3(NT), 0, (hipStream_t)stream, src, src_stride, dst,
                       dst_stride, n, h, w, siting == DEMFI_420MPEG2 ? 1 : 0, to_bgr_coefs(matrix, full_range, depth));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_bgr16_to_yuv420p16_gather(const uint16_t* base, const int64_t* src_offsets, uint16_t* dst, int64_t dst_stride, int n,
                                               int h, int w, int depth, int matrix, int full_range, void* stream)
{
    int st = check_args("demfi_bgr16_to_yuv420p16_gather", base, dst, n, h, w, depth, matrix, full_range, 2);
    if (st < 0) return st;
    if (!src_offsets)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_bgr16_to_yuv420p16_gather: NULL src_offsets");
    const int64_t payload = payload_of(DEMFI_YUV_420, h, w);
    if (n > 1 && dst_stride < payload)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_bgr16_to_yuv420p16_gather: dst_stride %lld below the payload of %lld samples",
                               (long long)dst_stride, (long long)payload);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(bgr_to_yuv420t_gather_kernel<uint16_t>, grid_for(n, (h + 1) / 2, w), dim3(NT), 0, (hipStream_t)stream, base,
                       src_offsets, dst, dst_stride, n, h, w, to_yuv_coefs(matrix, full_range, depth));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
