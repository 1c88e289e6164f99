// The uint16 frame I/O of a context (the 16-bit frame path of the Y4M stream edge, demfi_amd/video.py --high-depth): BGR uint16
// [h,w,3] frames holding 0 .. peak = 2^d - 1 at bit depth d = 8 .. 16 into the network's input, and the network's output frames back.
#include "common.h"

namespace {

constexpr int NT = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

// ---- uint16 frame I/O of a context: u8_ingest_kernel / frame_to_u8_kernel (pointwise.hip) with peak in place of 255 ---------------
struct U16Frames { const uint16_t* f[4]; };

// One thread per half-resolution pixel reads the 2x2 block of the 4 BGR uint16 [h,w,3] frames once and writes x (fp32 planes,
// (p/peak - 0.5)*2 in three fp32 steps, reflect-padded bottom / right to H x W), the space-to-depth record of FF_RDB (48 channels:
// (frame*3 + c)*4 + ry*2 + rx) and the overlay mean of B0, B1.
template <typename T>
__global__ void u16_ingest_kernel(U16Frames fr, float* __restrict__ x, T* __restrict__ s2d, float* __restrict__ ov, int h, int w,
                                  int H, int W, float peak)
{
    const int H2 = H >> 1, W2 = W >> 1;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= H2 * W2) return;
    const int x2 = i % W2, y2 = i / W2;
    T rec[48];
    float b01[2][3][4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int Y = 2 * y2 + (q >> 1), X = 2 * x2 + (q & 1);
            const int sx = X < w ? X : 2 * (w - 1) - X;
            const int sy = Y < h ? Y : 2 * (h - 1) - Y;
            const DEMFI_GLOBAL uint16_t* p = gcp<uint16_t>(fr.f[f]) + ((int64_t)sy * w + sx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = (float)p[c] / peak;
                v = v - 0.5f;
                v = v * 2.0f;
                x[((int64_t)(c * 4 + f) * H + Y) * W + X] = v;
                rec[(f * 3 + c) * 4 + q] = (T)v;
                if (f < 2) b01[f][c][q] = v;
            }
        }
    }
    T* o = s2d + (int64_t)i * 48;
#pragma unroll
    for (int k = 0; k < 48 * (int)sizeof(T) / 16; ++k) st_global16((char*)o + k * 16, ((const uint4*)rec)[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            ov[((int64_t)c * H + 2 * y2 + (q >> 1)) * W + 2 * x2 + (q & 1)] = (b01[0][c][q] + b01[1][c][q]) / 2.0f;
}

// Output side: clip((x + 1) / 2, 0, 1) * peak on the float64 copy of the fp32 frame, truncated (the reference's denorm255_np +
// astype rule at depth d), cropped to h x w, HWC.
__global__ void frame_to_u16_kernel(const float* __restrict__ fr, uint16_t* __restrict__ out, int h, int w, int H, int W, double peak)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= h * w) return;
    const int X = i % w, Y = i / w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v = ((double)fr[((int64_t)c * H + Y) * W + X] + 1.0) / 2.0;
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        gp<uint16_t>(out)[(int64_t)i * 3 + c] = (uint16_t)(v * peak);
    }
}

}  // namespace

extern "C" int demfi_u16_ingest(const uint16_t* const* frames, int h, int w, int depth, float* x, void* s2d, float* overlay, int dtype,
                                int H, int W, void* stream)
{
    if (!frames || !x || !s2d || !overlay || h < 2 || w < 2 || H < h || W < w || H - h >= h || W - w >= w || (H & 1) || (W & 1))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_u16_ingest: bad sizes %dx%d -> %dx%d", h, w, H, W);
    if (depth < 8 || depth > 16) return demfi_set_error(DEMFI_ERR_ARG, "demfi_u16_ingest: bit depth %d outside 8..16", depth);
    U16Frames fr;
    for (int i = 0; i < 4; ++i) {
        if (!frames[i] || ((uintptr_t)frames[i] & 1)) return demfi_set_error(DEMFI_ERR_ARG, "demfi_u16_ingest: frame %d is NULL or odd", i);
        fr.f[i] = frames[i];
    }
    const int64_t n = (int64_t)(H / 2) * (W / 2);
    const float peak = (float)((1 << depth) - 1);
    if (dtype == DEMFI_F16)
        hipLaunchKernelGGL(u16_ingest_kernel<half_t>, dim3(blocks_for(n)), dim3(NT), 0, (hipStream_t)stream, fr, x, (half_t*)s2d, overlay, h, w, H, W, peak);
    else if (dtype == DEMFI_F32)
        hipLaunchKernelGGL(u16_ingest_kernel<float>, dim3(blocks_for(n)), dim3(NT), 0, (hipStream_t)stream, fr, x, (float*)s2d, overlay, h, w, H, W, peak);
    else
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_u16_ingest: dtype");
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_frame_to_u16(const float* frame, uint16_t* out, int h, int w, int H, int W, int depth, void* stream)
{
    if (!frame || !out || ((uintptr_t)out & 1) || h <= 0 || w <= 0 || H < h || W < w || depth < 8 || depth > 16)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_frame_to_u16: bad args");
    hipLaunchKernelGGL(frame_to_u16_kernel, dim3(blocks_for((int64_t)h * w)), dim3(NT), 0, (hipStream_t)stream, frame, out, h, w, H, W,
                       (double)((1 << depth) - 1));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
