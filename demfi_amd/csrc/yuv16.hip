// The 16-bit frame path of the Y4M stream edge (demfi_amd/video.py --high-depth): YUV 4:2:0 <-> BGR at bit depth d = 10 .. 16 (and
// 8, to anchor this path to yuv.hip value for value), the SAD of scene-cut detection over 16-bit samples, and the uint16
// ingest / egress of a context.  Samples and BGR values are unsigned 16-bit holding 0 .. peak = 2^d - 1.
//
// The definition is the numpy pair yuv420_to_bgr16_np / bgr16_to_yuv420_np in demfi_amd/y4m.py; the kernels match it bit for bit.
// It is the 8-bit definition (yuv.hip) with s = 2^(d-8): limited range Y 16s .. 235s, C 16s .. 240s, Y offset 16s, chroma centre
// 2^(d-1), scale factors peak / (219 s), peak / (224 s) and their inverses; coefficients rounded half up to Q(8+d) from the same
// float64 expressions as in y4m.py (built with -ffp-contract=off); ONE round-half-up, clamp to [0, peak].  A product of a
// Q(8+d) coefficient (below 2^27) and an operand (luma and chroma in 1/16 units: below 2^21) reaches 2^47: the accumulators are
// true 64-bit sums of 32 x 32 -> 64 bit products (v_mad_i64_i32), exact like numpy's int64.
//
// Memory-bound on bytes, so the lane layout of yuv.hip is kept: a lane owns a strip of 8 luma pixels x 2 rows (one chroma row):
// Y as one 16-byte access per row, the 48 bytes of BGR per row as three 16-byte accesses, 8 bytes per chroma plane.  Strips cut by
// the right edge or whose rows are not 16-byte aligned (payloads are only 2-byte aligned) take the sample path; the data are the same.
// Every stride and offset of this unit counts SAMPLES (uint16 elements), so any value is a valid alignment.
#include "common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SX = 8;                 // luma pixels per lane strip

struct ToBgr16 {                      // Q(8+d); chroma arrives in 1/16 units -> one shift by sh = 8 + d + 4
    int cy, r_cr, g_cb, g_cr, b_cb, yoff, mid16, sh;
};
struct ToYuv16 {                      // Q(8+d) over d-bit B, G, R; q = 8 + d; mid = 2^(d-1)
    int y_r, y_g, y_b, cb_r, cb_g, cb_b, cr_r, cr_g, cr_b, yoff, mid, q;
};

inline int fixq(double c, int q) { return (int)floor(c * (double)(1 << q) + 0.5); }

inline void kr_kb(int matrix, double* kr, double* kb)
{
    if (matrix == DEMFI_BT709) { *kr = 0.2126; *kb = 0.0722; }
    else { *kr = 0.299; *kb = 0.114; }
}

// y4m.py: to_bgr_coefs_depth
ToBgr16 to_bgr_coefs(int matrix, int full, int d)
{
    double kr, kb;
    kr_kb(matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    const int q = 8 + d, s = 1 << (d - 8), peak = (1 << d) - 1;
    const double ys = full ? 1.0 : peak / (219.0 * s), cs = full ? 1.0 : peak / (224.0 * s);
    ToBgr16 c;
    c.cy = fixq(ys, q);
    c.r_cr = fixq(cs * 2.0 * (1.0 - kr), q);
    c.g_cb = fixq(-(cs * 2.0 * kb * (1.0 - kb) / kg), q);
    c.g_cr = fixq(-(cs * 2.0 * kr * (1.0 - kr) / kg), q);
    c.b_cb = fixq(cs * 2.0 * (1.0 - kb), q);
    c.yoff = full ? 0 : 16 * s;
    c.mid16 = (1 << (d - 1)) * 16;
    c.sh = q + 4;
    return c;
}

// y4m.py: to_yuv_coefs_depth
ToYuv16 to_yuv_coefs(int matrix, int full, int d)
{
    double kr, kb;
    kr_kb(matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    const int q = 8 + d, s = 1 << (d - 8), peak = (1 << d) - 1;
    const double ys = full ? 1.0 : 219.0 * s / peak, cs = full ? 1.0 : 224.0 * s / peak;
    ToYuv16 c;
    c.y_r = fixq(ys * kr, q);
    c.y_g = fixq(ys * kg, q);
    c.y_b = fixq(ys * kb, q);
    c.cb_r = fixq(-(cs * kr / (2.0 * (1.0 - kb))), q);
    c.cb_g = fixq(-(cs * kg / (2.0 * (1.0 - kb))), q);
    c.cb_b = fixq(cs * 0.5, q);
    c.cr_r = fixq(cs * 0.5, q);
    c.cr_g = fixq(-(cs * kg / (2.0 * (1.0 - kr))), q);
    c.cr_b = fixq(-(cs * kb / (2.0 * (1.0 - kr))), q);
    c.yoff = full ? 0 : 16 * s;
    c.mid = 1 << (d - 1);
    c.q = q;
    return c;
}

// clamp(acc >> sh, 0, top), as a clamp of the accumulator and then the shift (same value for every acc); lim = ((top + 1) << sh) - 1
__device__ __forceinline__ int sat_shr(int64_t acc, int sh, int64_t lim)
{
    return (int)((acc < 0 ? 0 : (acc > lim ? lim : acc)) >> sh);
}

__device__ __forceinline__ int64_t mul64(int a, int b) { return (int64_t)a * (int64_t)b; }

__device__ __forceinline__ int lo16(uint32_t v) { return (int)(v & 0xffffu); }
__device__ __forceinline__ int hi16(uint32_t v) { return (int)(v >> 16); }

// 8 samples row[x0 .. x0+7] -> v; indices past the right edge repeat row[w-1]
__device__ __forceinline__ void load8(const uint16_t* row, int x0, int w, int* v)
{
    const uint16_t* p = row + x0;
    if (x0 + 8 <= w && ((uintptr_t)p & 15) == 0) {
        const u4_t t = *gcp<u4_t>(p);
        v[0] = lo16(t.x); v[1] = hi16(t.x); v[2] = lo16(t.y); v[3] = hi16(t.y);
        v[4] = lo16(t.z); v[5] = hi16(t.z); v[6] = lo16(t.w); v[7] = hi16(t.w);
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = gcp<uint16_t>(row)[min(x0 + i, w - 1)];
}

// store the first n (<= 8) of the 8 samples v at p
__device__ __forceinline__ void store8(uint16_t* p, const int* v, int n)
{
    if (n >= 8 && ((uintptr_t)p & 15) == 0) {
        u4_t t;
        t.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16); t.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
        t.z = (uint32_t)v[4] | ((uint32_t)v[5] << 16); t.w = (uint32_t)v[6] | ((uint32_t)v[7] << 16);
        *gp<u4_t>(p) = t;
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < n) gp<uint16_t>(p)[i] = (uint16_t)v[i];
}

// 6 chroma samples c0-1 .. c0+4 of one row, clamped to [0, cw-1]
__device__ __forceinline__ void load_c6(const uint16_t* row, int c0, int cw, int* c)
{
    c[0] = gcp<uint16_t>(row)[max(c0 - 1, 0)];
    const uint16_t* p = row + c0;
    if (c0 + 4 <= cw && ((uintptr_t)p & 7) == 0) {
        const uint64_t v = *gcp<uint64_t>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[1 + i] = (int)((v >> (16 * i)) & 0xffff);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) c[1 + i] = gcp<uint16_t>(row)[min(c0 + i, cw - 1)];
    }
    c[5] = gcp<uint16_t>(row)[min(c0 + 4, cw - 1)];
}

// store the first n (<= 4) of the 4 chroma samples v at p
__device__ __forceinline__ void store_c4(uint16_t* p, const int* v, int n)
{
    if (n >= 4 && ((uintptr_t)p & 7) == 0) {
        *gp<uint64_t>(p) = (uint64_t)v[0] | ((uint64_t)v[1] << 16) | ((uint64_t)v[2] << 32) | ((uint64_t)v[3] << 48);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) gp<uint16_t>(p)[i] = (uint16_t)v[i];
}

// the 24 samples of 8 BGR pixels (three 16-byte words); n = pixels inside the frame
__device__ __forceinline__ void store_bgr8(uint16_t* p, const int* v, int n)
{
    if (n >= 8 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u4_t t;
            t.x = (uint32_t)v[8 * i] | ((uint32_t)v[8 * i + 1] << 16); t.y = (uint32_t)v[8 * i + 2] | ((uint32_t)v[8 * i + 3] << 16);
            t.z = (uint32_t)v[8 * i + 4] | ((uint32_t)v[8 * i + 5] << 16); t.w = (uint32_t)v[8 * i + 6] | ((uint32_t)v[8 * i + 7] << 16);
            gp<u4_t>(p)[i] = t;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 24; ++i)                   // edge / unaligned strip: constant sample positions, guarded
        if (i < 3 * n) gp<uint16_t>(p)[i] = (uint16_t)v[i];
}

__device__ __forceinline__ void load_bgr8(const uint16_t* row, int x0, int w, int* v)
{
    const uint16_t* p = row + 3 * x0;
    if (x0 + 8 <= w && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const u4_t t = gcp<u4_t>(p)[i];
            v[8 * i] = lo16(t.x); v[8 * i + 1] = hi16(t.x); v[8 * i + 2] = lo16(t.y); v[8 * i + 3] = hi16(t.y);
            v[8 * i + 4] = lo16(t.z); v[8 * i + 5] = hi16(t.z); v[8 * i + 6] = lo16(t.w); v[8 * i + 7] = hi16(t.w);
        }
        return;
    }
#pragma unroll
    for (int px = 0; px < 8; ++px) {               // past the right edge: the last pixel again
        const int x = min(x0 + px, w - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[3 * px + ch] = gcp<uint16_t>(row)[3 * x + ch];
    }
}

// one lane: chroma row cy (luma rows 2cy, 2cy+1) x luma columns x0 .. x0+7 of one frame
__global__ __launch_bounds__(NT) void yuv420p16_to_bgr16_kernel(const uint16_t* __restrict__ src, int64_t src_stride,
                                                               uint16_t* __restrict__ dst, int64_t dst_stride, int n, int h, int w,
                                                               int mpeg2, int peak, ToBgr16 k)
{
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1, ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ch * ns) return;
    const int cy = id / ns, x0 = (id - cy * ns) * SX, c0 = x0 >> 1;
    const int64_t rnd = (int64_t)1 << (k.sh - 1), lim = ((int64_t)(peak + 1) << k.sh) - 1;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint16_t* Y = src + (int64_t)f * src_stride;
        const uint16_t* planes[2] = {Y + (int64_t)h * w, Y + (int64_t)h * w + (int64_t)ch * cw};
        // vertical 3/4 + 1/4 (both sitings are centred vertically): V[r][plane][i], weight 4
        int V[2][2][6];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            int cm[6], c_[6], cp[6];
            load_c6(planes[pl] + (int64_t)max(cy - 1, 0) * cw, c0, cw, cm);
            load_c6(planes[pl] + (int64_t)cy * cw, c0, cw, c_);
            load_c6(planes[pl] + (int64_t)min(cy + 1, ch - 1) * cw, c0, cw, cp);
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
            load8(Y + (int64_t)y * w, x0, w, yv);
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
                const int64_t ly = mul64(k.cy, yy) + rnd;
                o[3 * px] = sat_shr(ly + mul64(k.b_cb, cb), k.sh, lim);
                o[3 * px + 1] = sat_shr(ly + mul64(k.g_cb, cb) + mul64(k.g_cr, cr), k.sh, lim);
                o[3 * px + 2] = sat_shr(ly + mul64(k.r_cr, cr), k.sh, lim);
            }
            store_bgr8(dst + (int64_t)f * dst_stride + ((int64_t)y * w + x0) * 3, o, w - x0);
        }
    }
}

// frame f read at base + offs[f] (samples): BGR frame -> 4:2:0 payload, luma rows 2cy, 2cy+1 (the second clamped to h-1 at an odd
// bottom edge) x columns x0 .. x0+7 -> 16 Y, 4 Cb, 4 Cr; one (wave-uniform) offset load per frame
__global__ __launch_bounds__(NT) void bgr16_to_yuv420p16_gather_kernel(const uint16_t* __restrict__ base, const int64_t* __restrict__ offs,
                                                                      uint16_t* __restrict__ dst, int64_t dst_stride, int n, int h, int w,
                                                                      int peak, ToYuv16 k)
{
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1, ns = (w + SX - 1) / SX;
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ch * ns) return;
    const int cy = id / ns, x0 = (id - cy * ns) * SX, c0 = x0 >> 1;
    const int64_t ylim = ((int64_t)(peak + 1) << k.q) - 1, clim = ((int64_t)(peak + 1) << (k.q + 2)) - 1;
    const int64_t yadd = ((int64_t)k.yoff << k.q) + ((int64_t)1 << (k.q - 1));
    const int64_t cadd = ((int64_t)k.mid << (k.q + 2)) + ((int64_t)1 << (k.q + 1));
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint16_t* Sp = base + offs[f];
        uint16_t* Yp = dst + (int64_t)f * dst_stride;
        int64_t cbs[4] = {0, 0, 0, 0}, crs[4] = {0, 0, 0, 0};
        for (int r = 0; r < 2; ++r) {
            const int y = min(2 * cy + r, h - 1);
            int v[24], yo[8];
            load_bgr8(Sp + (int64_t)y * w * 3, x0, w, v);
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                const int B = v[3 * px], G = v[3 * px + 1], R = v[3 * px + 2];
                yo[px] = sat_shr(mul64(k.y_r, R) + mul64(k.y_g, G) + mul64(k.y_b, B) + yadd, k.q, ylim);
                cbs[px >> 1] += mul64(k.cb_r, R) + mul64(k.cb_g, G) + mul64(k.cb_b, B);
                crs[px >> 1] += mul64(k.cr_r, R) + mul64(k.cr_g, G) + mul64(k.cr_b, B);
            }
            if (2 * cy + r < h) store8(Yp + (int64_t)y * w + x0, yo, w - x0);
        }
        int cbo[4], cro[4];
        for (int i = 0; i < 4; ++i) {
            cbo[i] = sat_shr(cbs[i] + cadd, k.q + 2, clim);
            cro[i] = sat_shr(crs[i] + cadd, k.q + 2, clim);
        }
        uint16_t* pcb = Yp + (int64_t)h * w + (int64_t)cy * cw + c0;
        store_c4(pcb, cbo, cw - c0);
        store_c4(pcb + (int64_t)ch * cw, cro, cw - c0);
    }
}

// SAD of frame pair f over 16-bit samples: |a - b| summed over `samples` samples, a = base + a_offs[f], b = base + b_offs[f]
// (offsets in samples: any 2-byte alignment of either).  The samples before a's first 16-byte boundary (head) and after its last
// one (tail) go to the first 8 lanes of block x = 0, one sample each; the body is 16-byte loads, aligned for a (b's loads may be
// unaligned, which global memory serves) and four v_sad_u16 per load pair (two samples per dword).  A lane's partial stays below
// 2^32 (at most ceil(samples / 8 / (1024 NT)) * 8 * 65535 < 2^27 for payloads up to 16384 x 16384 4:2:0); the wave and block sums
// are 64-bit, and each block adds its sum with ONE 64-bit atomic (integer adds are exact in any order).
__global__ __launch_bounds__(NT) void yuv420p16_sad_kernel(const uint16_t* __restrict__ base, const int64_t* __restrict__ a_offs,
                                                          const int64_t* __restrict__ b_offs, int n, int64_t samples,
                                                          unsigned long long* __restrict__ sad)
{
    typedef u4_t u4_unaligned __attribute__((aligned(2)));
    __shared__ unsigned long long part[NT / 64];
    const int tid = threadIdx.x;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint16_t* a = base + a_offs[f];
        const uint16_t* b = base + b_offs[f];
        const int64_t head = min((int64_t)(((16 - ((uintptr_t)a & 15)) & 15) >> 1), samples);
        const int64_t nvec = (samples - head) >> 3;
        const int64_t tail = head + (nvec << 3);              // samples - tail < 8
        uint32_t acc = 0;
        if (blockIdx.x == 0 && tid < 8) {
            if (tid < head) acc = __builtin_amdgcn_sad_u16(gcp<uint16_t>(a)[tid], gcp<uint16_t>(b)[tid], acc);
            if (tail + tid < samples) acc = __builtin_amdgcn_sad_u16(gcp<uint16_t>(a)[tail + tid], gcp<uint16_t>(b)[tail + tid], acc);
        }
        for (int64_t v = (int64_t)blockIdx.x * NT + tid; v < nvec; v += (int64_t)gridDim.x * NT) {
            const u4_t x = *(const DEMFI_GLOBAL u4_t*)(a + head + 8 * v);
            const u4_t y = *(const DEMFI_GLOBAL u4_unaligned*)(b + head + 8 * v);
            acc = __builtin_amdgcn_sad_u16(x.x, y.x, acc);
            acc = __builtin_amdgcn_sad_u16(x.y, y.y, acc);
            acc = __builtin_amdgcn_sad_u16(x.z, y.z, acc);
            acc = __builtin_amdgcn_sad_u16(x.w, y.w, acc);
        }
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

int check_common(const char* fn, const void* src, const void* dst, int n, int h, int w, int depth, int matrix, int full_range)
{
    if (!src || !dst || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    if (((uintptr_t)src & 1) || ((uintptr_t)dst & 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: buffers of 16-bit samples must be 2-byte aligned", fn);
    if (h < 2 || w < 2 || h > 16384 || w > 16384)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: frame size %dx%d outside 2..16384", fn, h, w);
    if (depth < 8 || depth > 16)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: bit depth %d outside 8..16", fn, depth);
    if ((matrix != DEMFI_BT601 && matrix != DEMFI_BT709) || (full_range != 0 && full_range != 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: matrix %d / full_range %d", fn, matrix, full_range);
    return DEMFI_OK;
}

dim3 grid_for(int n, int h, int w)
{
    const int64_t lanes = (int64_t)((h + 1) / 2) * ((w + SX - 1) / SX);
    return dim3((unsigned)((lanes + NT - 1) / NT), (unsigned)min(n, 65535));
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace

extern "C" int demfi_yuv420p16_to_bgr16(const uint16_t* src, int64_t src_stride, uint16_t* dst, int64_t dst_stride, int n, int h, int w,
                                        int depth, int matrix, int full_range, int siting, void* stream)
{
    int st = check_common("demfi_yuv420p16_to_bgr16", src, dst, n, h, w, depth, matrix, full_range);
    if (st < 0) return st;
    const int64_t payload = (int64_t)h * w + 2 * (int64_t)((h + 1) / 2) * ((w + 1) / 2);
    if (siting != DEMFI_420JPEG && siting != DEMFI_420MPEG2)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_yuv420p16_to_bgr16: chroma siting %d", siting);
    if (n > 1 && (src_stride < payload || dst_stride < (int64_t)h * w * 3))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_yuv420p16_to_bgr16: strides %lld / %lld below the frame sizes %lld / %lld samples",
                               (long long)src_stride, (long long)dst_stride, (long long)payload, (long long)h * w * 3);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(yuv420p16_to_bgr16_kernel, grid_for(n, h, w), dim3(NT), 0, (hipStream_t)stream, src, src_stride, dst, dst_stride, n,
                       h, w, siting == DEMFI_420MPEG2 ? 1 : 0, (1 << depth) - 1, to_bgr_coefs(matrix, full_range, depth));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_bgr16_to_yuv420p16_gather(const uint16_t* base, const int64_t* src_offsets, uint16_t* dst, int64_t dst_stride, int n,
                                               int h, int w, int depth, int matrix, int full_range, void* stream)
{
    int st = check_common("demfi_bgr16_to_yuv420p16_gather", base, dst, n, h, w, depth, matrix, full_range);
    if (st < 0) return st;
    if (!src_offsets)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_bgr16_to_yuv420p16_gather: NULL src_offsets");
    const int64_t payload = (int64_t)h * w + 2 * (int64_t)((h + 1) / 2) * ((w + 1) / 2);
    if (n > 1 && dst_stride < payload)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_bgr16_to_yuv420p16_gather: dst_stride %lld below the payload of %lld samples",
                               (long long)dst_stride, (long long)payload);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(bgr16_to_yuv420p16_gather_kernel, grid_for(n, h, w), dim3(NT), 0, (hipStream_t)stream, base, src_offsets, dst,
                       dst_stride, n, h, w, (1 << depth) - 1, to_yuv_coefs(matrix, full_range, depth));
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_yuv420p16_sad(const uint16_t* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int64_t samples,
                                   uint64_t* sad, void* stream)
{
    if (!base || !a_offsets || !b_offsets || !sad || n < 0 || samples <= 0 || ((uintptr_t)base & 1))
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_yuv420p16_sad: NULL or odd buffer, n=%d or samples=%lld", n, (long long)samples);
    if (n == 0) return DEMFI_OK;
    DEMFI_HIP_CHECK(hipMemsetAsync(sad, 0, (size_t)n * sizeof(uint64_t), (hipStream_t)stream));
    const int64_t blocks = ((samples >> 3) + NT - 1) / NT;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks), (unsigned)(n < 65535 ? n : 65535));
    hipLaunchKernelGGL(yuv420p16_sad_kernel, grid, dim3(NT), 0, (hipStream_t)stream, base, a_offsets, b_offsets, n, samples,
                       (unsigned long long*)sad);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

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
