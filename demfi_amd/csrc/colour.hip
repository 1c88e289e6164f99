// Linear light at the Y4M stream edge (demfi_amd/video.py --linear-light): the two kernels around the unchanged mix and scale kernels.
//   demfi_bgr_to_linear_gather  BGR frames of codes (the network's outputs) -> LINEAR payloads: uint16 [3, h, w], planes B, G, R
//   demfi_linear_to_yuv         linear payloads -> Y'CbCr payloads of the run's depth and layout
// The definition is numpy code in demfi_amd/colour.py (linearize_np / encode_payload_np); the kernels match it bit for bit.  They compute
// no transfer function: fwd (code -> linear value, at most 4096 uint16) and inv (linear value -> the code nearest in light, 65536 uint16)
// are tables of colour.py.  Behind the inverse lookup the encode IS the gather of yuv_family.hip: the ToYuv coefficients, mul, sat_shr
// and the sample accessors of yuv_common.h, with three plane reads where that kernel has load_bgr8.
//
// Memory-bound on bytes, so both keep the lane layout of the gathers: a lane owns a strip of 8 pixels of one row (4:2:0 encode: of two
// rows, one chroma row), read and written with one access of 8 samples per plane and row.  Strips cut by the right edge or off the
// vector boundary (payloads are only sample-aligned) take the sample path; the data are the same.
//   fwd: at most 8 KiB; a workgroup copies it into LDS once and looks up from there (24 lookups a lane and frame).
//   inv: 128 KiB, read through L2 with 2-byte loads (profiles/linear_light.md has the measurement).
// 64-bit offsets throughout, no atomics.
#include "yuv_common.h"

namespace {

constexpr int MAXF = 4096;            // frames along the grid's y; a block walks the rest
constexpr int FWD_MAX = 4096;         // entries of fwd at 12 bits

inline dim3 lanes_grid(int n, int rows, int w)
{
    const int64_t lanes = (int64_t)rows * ((w + SX - 1) / SX);
    return dim3((unsigned)((lanes + NT - 1) / NT), (unsigned)min(n, MAXF));
}

// frame f read at base + offs[f] (samples of T): row y x columns x0 .. x0+7 -> 8 linear values in each of the three planes
template <typename T>
__global__ __launch_bounds__(NT) void bgr_to_linear_gather_kernel(const T* __restrict__ base, const int64_t* __restrict__ offs,
                                                                 uint16_t* __restrict__ dst, int64_t dst_stride, int n, int h, int w,
                                                                 int peak, const uint16_t* __restrict__ fwd)
{
    __shared__ uint16_t lut[FWD_MAX];
    for (int i = threadIdx.x; i <= peak; i += NT) lut[i] = gcp<uint16_t>(fwd)[i];
    __syncthreads();
    const int ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= h * ns) return;
    const int y = id / ns, x0 = (id - y * ns) * SX;
    const int64_t hw = (int64_t)h * w;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        int v[24];
        load_bgr8<T>(base + offs[f] + (int64_t)y * w * 3, x0, w, v);
        uint16_t* P = dst + (int64_t)f * dst_stride + (int64_t)y * w + x0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            int o[8];
#pragma unroll
            for (int px = 0; px < SX; ++px) o[px] = lut[min(v[3 * px + ch], peak)];     // a stored value past the peak must not leave the table
            store_n<uint16_t, 8>(P + ch * hw, o, w - x0);
        }
    }
}

// B, G, R codes of the 8 pixels x0 .. x0+7 of one row of a linear payload (past the right edge: the last pixel again) -> v[3 px + ch]
__device__ __forceinline__ void load_codes8(const uint16_t* P, int64_t hw, int64_t row, int x0, int w, const uint16_t* inv, int* v)
{
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        int t[8];
        load_n<uint16_t, 8>(P + ch * hw + row, x0, w, t);
#pragma unroll
        for (int px = 0; px < SX; ++px) v[3 * px + ch] = gcp<uint16_t>(inv)[t[px]];
    }
}

// payload f read at src + offs[f] BYTES.  4:2:2, 4:4:4, mono: row y x columns x0 .. x0+7 -> 8 Y and 8 / 4 / 0 Cb, Cr (the arithmetic of
// bgr_to_yuvl_gather_kernel).  4:2:0: luma rows 2cy, 2cy+1 x columns x0 .. x0+7 -> 16 Y, 4 Cb, 4 Cr (bgr_to_yuv420t_gather_kernel).
template <typename T, int LAYOUT>
__global__ __launch_bounds__(NT) void linear_to_yuv_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offs,
                                                          T* __restrict__ dst, int64_t dst_stride, int n, int h, int w, ToYuv k,
                                                          const uint16_t* __restrict__ inv)
{
    typedef typename Acc<T>::type A;
    constexpr bool box = LAYOUT == DEMFI_YUV_420, chroma = LAYOUT != DEMFI_YUV_MONO;
    const int ns = (w + SX - 1) / SX, cw = (w + 1) >> 1, ch = (h + 1) >> 1, rows = box ? ch : h;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= rows * ns) return;
    const int r0 = id / ns, x0 = (id - r0 * ns) * SX, c0 = x0 >> 1;
    const int csh = (LAYOUT == DEMFI_YUV_444) ? k.q : k.q + 2;         // 4:2:2 sums weights 1 + 2 + 1, 4:2:0 four pixels
    const A ylim = ((A)(k.peak + 1) << k.q) - 1, clim = ((A)(k.peak + 1) << csh) - 1;
    const A yadd = ((A)k.yoff << k.q) + ((A)1 << (k.q - 1));
    const A cadd = ((A)k.mid << csh) + ((A)1 << (csh - 1));
    const int64_t hw = (int64_t)h * w;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint16_t* P = (const uint16_t*)(src + offs[f]);
        T* Yp = dst + (int64_t)f * dst_stride;
        A fc[2][8];                                // chroma of the strip's pixels, centred on 0; 4:2:0: summed over the two rows
#pragma unroll
        for (int px = 0; px < SX; ++px) fc[0][px] = fc[1][px] = 0;
        for (int r = 0; r < (box ? 2 : 1); ++r) {
            const int y = box ? min(2 * r0 + r, h - 1) : r0;
            int v[24], yo[8];
            load_codes8(P, hw, (int64_t)y * w, x0, w, inv, v);
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                const int B = v[3 * px], G = v[3 * px + 1], R = v[3 * px + 2];
                yo[px] = sat_shr<A>(mul<A>(k.y_r, R) + mul<A>(k.y_g, G) + mul<A>(k.y_b, B) + yadd, k.q, ylim);
                if (chroma) {
                    fc[0][px] += mul<A>(k.cb_r, R) + mul<A>(k.cb_g, G) + mul<A>(k.cb_b, B);
                    fc[1][px] += mul<A>(k.cr_r, R) + mul<A>(k.cr_g, G) + mul<A>(k.cr_b, B);
                }
            }
            if (!box || 2 * r0 + r < h) store_n<T, 8>(Yp + (int64_t)y * w + x0, yo, w - x0);
        }
        if (LAYOUT == DEMFI_YUV_444) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                int co[8];
#pragma unroll
                for (int px = 0; px < SX; ++px) co[px] = sat_shr<A>(fc[pl][px] + cadd, csh, clim);
                store_n<T, 8>(Yp + (1 + pl) * hw + (int64_t)r0 * w + x0, co, w - x0);
            }
        } else if (LAYOUT == DEMFI_YUV_422) {      // the strip's first chroma sample also reads the pixel left of the strip
            const int64_t at = (int64_t)r0 * w + max(x0 - 1, 0);
            const int B = gcp<uint16_t>(inv)[gcp<uint16_t>(P)[at]], G = gcp<uint16_t>(inv)[gcp<uint16_t>(P)[hw + at]],
                      R = gcp<uint16_t>(inv)[gcp<uint16_t>(P)[2 * hw + at]];
            const A left[2] = {mul<A>(k.cb_r, R) + mul<A>(k.cb_g, G) + mul<A>(k.cb_b, B),
                               mul<A>(k.cr_r, R) + mul<A>(k.cr_g, G) + mul<A>(k.cr_b, B)};
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                int co[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)        // pixel x0 + 2i + 1 past the right edge is the last pixel again (load_codes8)
                    co[i] = sat_shr<A>((i ? fc[pl][2 * i - 1] : left[pl]) + 2 * fc[pl][2 * i] + fc[pl][2 * i + 1] + cadd, csh, clim);
                store_n<T, 4>(Yp + hw + (int64_t)pl * h * cw + (int64_t)r0 * cw + c0, co, cw - c0);
            }
        } else if (box) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                int co[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) co[i] = sat_shr<A>(fc[pl][2 * i] + fc[pl][2 * i + 1] + cadd, csh, clim);
                store_n<T, 4>(Yp + hw + (int64_t)pl * ch * cw + (int64_t)r0 * cw + c0, co, cw - c0);
            }
        }
    }
}

int check_frame(const char* fn, int n, int h, int w, int depth)
{
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (depth != 8 && depth != 10 && depth != 12)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: bit depth %d (8, 10 or 12: above, 16 bits of light do not tell the codes apart)", fn, depth);
    return DEMFI_OK;
}

template <typename T, int LAYOUT>
void launch_encode(dim3 grid, hipStream_t s, const uint8_t* src, const int64_t* offs, uint8_t* dst, int64_t dst_stride, int n, int h, int w,
                   const ToYuv& k, const uint16_t* inv)
{
    hipLaunchKernelGGL((linear_to_yuv_kernel<T, LAYOUT>), grid, dim3(NT), 0, s, src, offs, (T*)dst, dst_stride / (int64_t)sizeof(T), n, h, w, k,
                       inv);
}

template <typename T>
void launch_encode_layout(int layout, dim3 grid, hipStream_t s, const uint8_t* src, const int64_t* offs, uint8_t* dst, int64_t dst_stride,
                          int n, int h, int w, const ToYuv& k, const uint16_t* inv)
{
    if (layout == DEMFI_YUV_420) launch_encode<T, DEMFI_YUV_420>(grid, s, src, offs, dst, dst_stride, n, h, w, k, inv);
    else if (layout == DEMFI_YUV_422) launch_encode<T, DEMFI_YUV_422>(grid, s, src, offs, dst, dst_stride, n, h, w, k, inv);
    else if (layout == DEMFI_YUV_444) launch_encode<T, DEMFI_YUV_444>(grid, s, src, offs, dst, dst_stride, n, h, w, k, inv);
    else launch_encode<T, DEMFI_YUV_MONO>(grid, s, src, offs, dst, dst_stride, n, h, w, k, inv);
}

}  // namespace

extern "C" int demfi_bgr_to_linear_gather(const void* base, const int64_t* src_offsets, uint16_t* dst, int64_t dst_stride, int n, int h,
                                          int w, int sample_bytes, int depth, const uint16_t* fwd_table, void* stream)
{
    const char* fn = "demfi_bgr_to_linear_gather";
    if (!base || !src_offsets || !dst || !fwd_table) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    int st = check_frame(fn, n, h, w, depth);
    if (st < 0) return st;
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (sample_bytes == 1 && depth != 8)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d-bit codes in bytes", fn, depth);
    if (((uintptr_t)dst & 1) || ((uintptr_t)fwd_table & 1) || (sample_bytes == 2 && ((uintptr_t)base & 1)))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: buffers of 16-bit samples must be 2-byte aligned", fn);
    if (dst_stride < (int64_t)3 * h * w)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride %lld below the linear payload of %lld samples", fn, (long long)dst_stride,
                               (long long)3 * h * w);
    if (n == 0) return DEMFI_OK;
    const dim3 grid = lanes_grid(n, h, w);
    const int peak = (1 << depth) - 1;
    hipStream_t s = (hipStream_t)stream;
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(bgr_to_linear_gather_kernel<TAG_TYPE(t)>, grid, dim3(NT), 0, s, (const TAG_TYPE(t)*)base, src_offsets, dst, dst_stride, n,
                           h, w, peak, fwd_table);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_linear_to_yuv(const uint8_t* src, const int64_t* offsets, const int64_t* offsets_dev, int n, int h, int w, int depth,
                                   int layout, int matrix, int full_range, const uint16_t* inv_table, uint8_t* dst, int64_t dst_stride,
                                   void* stream)
{
    const char* fn = "demfi_linear_to_yuv";
    if (!src || !offsets || !offsets_dev || !inv_table || !dst) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    int st = check_frame(fn, n, h, w, depth);
    if (st < 0) return st;
    if (layout != DEMFI_YUV_420 && layout != DEMFI_YUV_422 && layout != DEMFI_YUV_444 && layout != DEMFI_YUV_MONO)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: layout %d", fn, layout);
    if ((matrix != DEMFI_BT601 && matrix != DEMFI_BT709) || (full_range != 0 && full_range != 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: matrix %d / full_range %d", fn, matrix, full_range);
    const int out_bytes = depth > 8 ? 2 : 1;
    const int64_t payload = payload_of(layout, h, w) * out_bytes;
    if (int st = check_dst_stride(fn, dst_stride, payload)) return st;
    uintptr_t odd = (uintptr_t)src | (uintptr_t)inv_table;
    if (out_bytes == 2) odd |= (uintptr_t)dst | (uintptr_t)dst_stride;
    if (int st = walk_offsets(fn, offsets, n, 1, 1, OFFS_ALL, 0, NO_LIMIT, 0, &odd)) return st;
    if (int st = check_even(fn, 2, odd)) return st;                     // the linear payloads are 16-bit whatever the output is
    if (n == 0) return DEMFI_OK;
    const dim3 grid = lanes_grid(n, layout == DEMFI_YUV_420 ? (h + 1) / 2 : h, w);
    const ToYuv k = to_yuv_coefs(matrix, full_range, depth);
    hipStream_t s = (hipStream_t)stream;
    if (out_bytes == 1) launch_encode_layout<uint8_t>(layout, grid, s, src, offsets_dev, dst, dst_stride, n, h, w, k, inv_table);
    else launch_encode_layout<uint16_t>(layout, grid, s, src, offsets_dev, dst, dst_stride, n, h, w, k, inv_table);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
