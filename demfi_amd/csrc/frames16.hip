// The uint16 frame I/O of a context (the 16-bit frame path of the Y4M stream edge, demfi_amd/video.py --high-depth): BGR uint16
// [h,w,3] frames holding 0 .. peak = 2^d - 1 at bit depth d = 8 .. 16 into the network's input, and the network's output frames back.
// The _rect forms address a tile inside full frames (--tile-high-depth): the ingest reads the tile's source rectangle through the
// frame's row pitch, the egress writes the tile's kept rectangle straight into the full output frame.
#include "yuv_common.h"

namespace {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

// ---- uint16 frame I/O of a context: u8_ingest_kernel / frame_to_u8_kernel (pointwise.hip) with peak in place of 255 ---------------
struct U16Frames { const uint16_t* f[4]; };

// One thread per half-resolution pixel reads the 2x2 block of the 4 BGR uint16 [h,w,3] frames once and writes x (fp32 planes,
// (p/peak - 0.5)*2 in three fp32 steps, reflect-padded bottom / right to H x W), the space-to-depth record of FF_RDB (48 channels:
// (frame*3 + c)*4 + ry*2 + rx) and the overlay mean of B0, B1.  The h x w pixels are rows of `pitch` pixels: a whole frame (pitch = w), or
// a rectangle of a wider one, whose origin the host has added to the four pointers; the reflection is in the rectangle's coordinates.
template <typename T>
__global__ void u16_ingest_kernel(U16Frames fr, float* __restrict__ x, T* __restrict__ s2d, float* __restrict__ ov, int h, int w,
                                  int pitch, int H, int W, float peak)
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
            const DEMFI_GLOBAL uint16_t* p = gcp<uint16_t>(fr.f[f]) + ((int64_t)sy * pitch + sx) * 3;
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

// frame_to_u16_kernel for the kept rectangle [ky0,ky1) x [kx0,kx1) of a tile whose plane pixel (0,0) is pixel (y0,x0) of the
// [fh,fw,3] frame `out`.  One lane per strip of SX pixels of one row; the strips of a row start where the destination is 16-byte
// aligned (6 bytes per pixel: every even address has such a pixel among 8 neighbours), so a whole strip leaves as three 16-byte
// stores and takes its three plane rows in as two 16-byte loads each where those are aligned; the strips cut by the rectangle's
// left and right edges go sample by sample.  Nothing outside the rectangle is read or written.
__global__ void frame_to_u16_rect_kernel(const float* __restrict__ fr, uint16_t* __restrict__ out, int fw, int y0, int x0, int ky0,
                                         int kx0, int ky1, int kx1, int H, int W, int ns, double peak)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= (ky1 - ky0) * ns) return;
    const int y = ky0 + i / ns;
    uint16_t* row = out + (int64_t)y * fw * 3;
    const int a = (int)(((uintptr_t)(row + 3 * (int64_t)kx0) & 15) >> 1);      // (a + 3 p) % 8 == 0 <=> pixel kx0 + p is aligned
    const int p = ((8 - a) * 3) & 7;                                            // 3 * 3 = 1 (mod 8)
    const int xs = kx0 + (p ? p - SX : 0) + SX * (i % ns);
    const int lo = max(xs, kx0), hi = min(xs + SX, kx1);
    if (lo >= hi) return;
    const bool whole = hi - lo == SX;
    const float* src = fr + (int64_t)(y - y0) * W + (xs - x0);
    int v[3 * SX];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* pl = src + (int64_t)c * H * W;
        float f[SX];
        if (whole && ((uintptr_t)pl & 15) == 0) {
#pragma unroll
            for (int k = 0; k < SX / 4; ++k) {
                const f4_t q = gcp<f4_t>(pl)[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) f[4 * k + j] = q[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < SX; ++j) f[j] = (xs + j >= lo && xs + j < hi) ? gcp<float>(pl)[j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < SX; ++j) {
            double d = ((double)f[j] + 1.0) / 2.0;
            d = d < 0.0 ? 0.0 : (d > 1.0 ? 1.0 : d);
            v[3 * j + c] = (int)(uint16_t)(d * peak);
        }
    }
    uint16_t* dst = row + 3 * (int64_t)xs;
    if (whole) {
        store_bgr8<uint16_t>(dst, v, SX);
        return;
    }
#pragma unroll
    for (int j = 0; j < SX; ++j)
        if (xs + j >= lo && xs + j < hi) {
#pragma unroll
            for (int c = 0; c < 3; ++c) gp<uint16_t>(dst)[3 * j + c] = (uint16_t)v[3 * j + c];
        }
}

// the checks and the launch of both ingest entry points; the rectangle is inside the frame
int ingest_u16(const char* fn, const uint16_t* const* frames, int pitch, int64_t origin, int h, int w, int depth, float* x, void* s2d,
               float* overlay, int dtype, int H, int W, void* stream)
{
    if (!frames || !x || !s2d || !overlay || h < 2 || w < 2 || H < h || W < w || H - h >= h || W - w >= w || (H & 1) || (W & 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: bad sizes %dx%d -> %dx%d", fn, h, w, H, W);
    if (depth < 8 || depth > 16) return demfi_set_error(DEMFI_ERR_ARG, "%s: bit depth %d outside 8..16", fn, depth);
    U16Frames fr;
    for (int i = 0; i < 4; ++i) {
        if (!frames[i] || ((uintptr_t)frames[i] & 1)) return demfi_set_error(DEMFI_ERR_ARG, "%s: frame %d is NULL or odd", fn, i);
        fr.f[i] = frames[i] + origin;
    }
    const int64_t n = (int64_t)(H / 2) * (W / 2);
    const float peak = (float)((1 << depth) - 1);
    if (dtype == DEMFI_F16)
        hipLaunchKernelGGL(u16_ingest_kernel<half_t>, dim3(blocks_for(n)), dim3(NT), 0, (hipStream_t)stream, fr, x, (half_t*)s2d, overlay, h, w, pitch, H, W, peak);
    else if (dtype == DEMFI_F32)
        hipLaunchKernelGGL(u16_ingest_kernel<float>, dim3(blocks_for(n)), dim3(NT), 0, (hipStream_t)stream, fr, x, (float*)s2d, overlay, h, w, pitch, H, W, peak);
    else
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dtype", fn);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

}  // namespace

extern "C" int demfi_u16_ingest(const uint16_t* const* frames, int h, int w, int depth, float* x, void* s2d, float* overlay, int dtype,
                                int H, int W, void* stream)
{
    return ingest_u16("demfi_u16_ingest", frames, w, 0, h, w, depth, x, s2d, overlay, dtype, H, W, stream);
}

extern "C" int demfi_u16_ingest_rect(const uint16_t* const* frames, int fh, int fw, int y0, int x0, int h, int w, int depth, float* x,
                                     void* s2d, float* overlay, int dtype, int H, int W, void* stream)
{
    if (fh < 2 || fw < 2 || fh > 16384 || fw > 16384 || y0 < 0 || x0 < 0 || h < 0 || w < 0 || (int64_t)y0 + h > fh || (int64_t)x0 + w > fw)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_u16_ingest_rect: the %dx%d rectangle at (%d, %d) leaves the %dx%d frame", h, w, y0, x0,
                               fh, fw);
    return ingest_u16("demfi_u16_ingest_rect", frames, fw, ((int64_t)y0 * fw + x0) * 3, h, w, depth, x, s2d, overlay, dtype, H, W, stream);
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

extern "C" int demfi_frame_to_u16_rect(const float* frame, uint16_t* out, int fh, int fw, int y0, int x0, int ky0, int kx0, int ky1, int kx1,
                                       int H, int W, int depth, void* stream)
{
    if (!frame || !out || ((uintptr_t)frame & 3) || ((uintptr_t)out & 1) || depth < 8 || depth > 16)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_frame_to_u16_rect: NULL or misaligned buffer, or bit depth %d outside 8..16", depth);
    if (fh < 1 || fw < 1 || fh > 16384 || fw > 16384 || H < 1 || W < 1 || H > 16384 || W > 16384 || y0 < 0 || x0 < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_frame_to_u16_rect: frame %dx%d, tile %dx%d at (%d, %d)", fh, fw, H, W, y0, x0);
    if (ky0 >= ky1 || kx0 >= kx1 || ky0 < y0 || kx0 < x0 || ky1 > y0 + H || kx1 > x0 + W || ky1 > fh || kx1 > fw)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_frame_to_u16_rect: the kept rectangle (%d, %d) .. (%d, %d) is empty or leaves its %dx%d "
                               "tile at (%d, %d) or the %dx%d frame", ky0, kx0, ky1, kx1, H, W, y0, x0, fh, fw);
    const int ns = (kx1 - kx0 + 2 * (SX - 1)) / SX;                 // strips of a row: the first may start up to SX - 1 pixels left of kx0
    hipLaunchKernelGGL(frame_to_u16_rect_kernel, dim3(blocks_for((int64_t)(ky1 - ky0) * ns)), dim3(NT), 0, (hipStream_t)stream, frame, out, fw,
                       y0, x0, ky0, kx0, ky1, kx1, H, W, ns, (double)((1 << depth) - 1));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
