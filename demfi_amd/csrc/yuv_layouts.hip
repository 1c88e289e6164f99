// The chroma layouts of the Y4M stream edge beside 4:2:0 (demfi_amd/video.py --any-layout): YUV 4:2:2, 4:4:4 and mono <-> BGR, over
// 8-bit samples (uint8, strides and offsets in bytes) and over 16-bit samples at bit depth d = 10 .. 16 (uint16 holding 0 .. peak =
// 2^d - 1, strides and offsets in samples; d = 8 is accepted so that the two sample types can be compared value for value).
//
// The definition is the numpy pair yuv_to_bgr16_np / bgr16_to_yuv_np in demfi_amd/y4m.py (yuv_to_bgr_np / bgr_to_yuv_np are its
// d = 8 instance); the kernels match it bit for bit.  The matrix step is that of yuv.hip / yuv16.hip, unchanged: Q(8+d)
// coefficients rounded half up from the same float64 expressions (built with -ffp-contract=off), chroma in 1/16 units, ONE
// round-half-up, clamp to [0, peak].  Only the resampling differs:
//   4:4:4  up: 16 c[y,x];  down: f rounded once.
//   4:2:2  (co-sited horizontally, no vertical filter)  up: even x: 16 c[y,x/2], odd x: 8 (c[y,cx] + c[y,min(cx+1,cw-1)]);
//          down: the [1,2,1]/4 of f[y,max(2i-1,0)], f[y,2i], f[y,min(2i+1,w-1)], rounded once.
//   mono   up: no chroma term, B = G = R;  down: Y only.
// f = the full-resolution Q(8+d) chroma centred on 0.  One kernel family over (sample type, layout): 8-bit samples accumulate in
// int32 (every sum stays below 2^29), 16-bit samples in true 64-bit sums of 32 x 32 -> 64 bit products, exact like numpy's int64.
//
// Memory-bound on bytes, so the lane layout of yuv.hip / yuv16.hip is kept, on one row instead of two (no layout here couples
// rows): a lane owns a strip of 8 luma pixels of one row -- Y as one access of 8 samples, the 24 samples of BGR as three, chroma as
// one access of 8 (4:4:4) or 4 (4:2:2) samples per plane: 8- and 4-byte accesses for uint8, 16- and 8-byte ones for uint16.  Strips
// cut by the right edge or whose rows are not aligned to the access (payloads are only sample-aligned) take the sample path; the
// data are the same.
#include "common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SX = 8;                 // luma pixels per lane strip

struct ToBgrL {                       // Q(8+d); chroma arrives in 1/16 units -> one shift by sh = 8 + d + 4
    int cy, r_cr, g_cb, g_cr, b_cb, yoff, mid16, sh, peak;
};
struct ToYuvL {                       // Q(8+d) over d-bit B, G, R; q = 8 + d; mid = 2^(d-1)
    int y_r, y_g, y_b, cb_r, cb_g, cb_b, cr_r, cr_g, cr_b, yoff, mid, q, peak;
};

inline int fixq(double c, int q) { return (int)floor(c * (double)(1 << q) + 0.5); }

inline void kr_kb(int matrix, double* kr, double* kb)
{
    if (matrix == DEMFI_BT709) { *kr = 0.2126; *kb = 0.0722; }
    else { *kr = 0.299; *kb = 0.114; }
}

// y4m.py: to_bgr_coefs_depth
ToBgrL to_bgr_coefs(int matrix, int full, int d)
{
    double kr, kb;
    kr_kb(matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    const int q = 8 + d, s = 1 << (d - 8), peak = (1 << d) - 1;
    const double ys = full ? 1.0 : peak / (219.0 * s), cs = full ? 1.0 : peak / (224.0 * s);
    ToBgrL c;
    c.cy = fixq(ys, q);
    c.r_cr = fixq(cs * 2.0 * (1.0 - kr), q);
    c.g_cb = fixq(-(cs * 2.0 * kb * (1.0 - kb) / kg), q);
    c.g_cr = fixq(-(cs * 2.0 * kr * (1.0 - kr) / kg), q);
    c.b_cb = fixq(cs * 2.0 * (1.0 - kb), q);
    c.yoff = full ? 0 : 16 * s;
    c.mid16 = (1 << (d - 1)) * 16;
    c.sh = q + 4;
    c.peak = peak;
    return c;
}

// y4m.py: to_yuv_coefs_depth
ToYuvL to_yuv_coefs(int matrix, int full, int d)
{
    double kr, kb;
    kr_kb(matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    const int q = 8 + d, s = 1 << (d - 8), peak = (1 << d) - 1;
    const double ys = full ? 1.0 : 219.0 * s / peak, cs = full ? 1.0 : 224.0 * s / peak;
    ToYuvL c;
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
    c.peak = peak;
    return c;
}

// ---- the two sample types -------------------------------------------------------------------------------------------------
template <typename T> struct Acc;                                   // accumulator of a sample type
template <> struct Acc<uint8_t> { typedef int type; };
template <> struct Acc<uint16_t> { typedef int64_t type; };

template <int BYTES> struct Word;                                   // the access of BYTES bytes
template <> struct Word<4> { typedef uint32_t type; };
template <> struct Word<8> { typedef uint64_t type; };
template <> struct Word<16> { typedef u4_t type; };
template <int K> struct Dwords { uint32_t d[K]; };

// N samples of T in one word <-> ints (values 0 .. 2^bits - 1)
template <typename T, int N> __device__ __forceinline__ void unpack(const typename Word<N * sizeof(T)>::type wv, int* v)
{
    constexpr int K = N * (int)sizeof(T) / 4, SPD = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    const Dwords<K> d = __builtin_bit_cast(Dwords<K>, wv);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (int)((d.d[i / SPD] >> (BITS * (i % SPD))) & ((1u << BITS) - 1u));
}

template <typename T, int N> __device__ __forceinline__ typename Word<N * sizeof(T)>::type pack(const int* v)
{
    constexpr int K = N * (int)sizeof(T) / 4, SPD = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    Dwords<K> d;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < SPD; ++i) t |= (uint32_t)v[j * SPD + i] << (BITS * i);
        d.d[j] = t;
    }
    return __builtin_bit_cast(typename Word<N * sizeof(T)>::type, d);
}

// N samples row[x0 .. x0+N-1] -> v; indices past the right edge repeat row[w-1]
template <typename T, int N> __device__ __forceinline__ void load_n(const T* row, int x0, int w, int* v)
{
    typedef typename Word<N * sizeof(T)>::type W;
    const T* p = row + x0;
    if (x0 + N <= w && ((uintptr_t)p & (N * sizeof(T) - 1)) == 0) {
        unpack<T, N>(*gcp<W>(p), v);
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = gcp<T>(row)[min(x0 + i, w - 1)];
}

// store the first n (<= N) of the N samples v at p
template <typename T, int N> __device__ __forceinline__ void store_n(T* p, const int* v, int n)
{
    typedef typename Word<N * sizeof(T)>::type W;
    if (n >= N && ((uintptr_t)p & (N * sizeof(T) - 1)) == 0) {
        *gp<W>(p) = pack<T, N>(v);
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i < n) gp<T>(p)[i] = (T)v[i];
}

// the 24 samples of 8 BGR pixels (three words of 8 samples); n = pixels inside the frame
template <typename T> __device__ __forceinline__ void store_bgr8(T* p, const int* v, int n)
{
    typedef typename Word<8 * sizeof(T)>::type W;
    if (n >= 8 && ((uintptr_t)p & (8 * sizeof(T) - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) gp<W>(p)[i] = pack<T, 8>(v + 8 * i);
        return;
    }
#pragma unroll
    for (int i = 0; i < 24; ++i)                   // edge / unaligned strip: constant sample positions, guarded
        if (i < 3 * n) gp<T>(p)[i] = (T)v[i];
}

template <typename T> __device__ __forceinline__ void load_bgr8(const T* row, int x0, int w, int* v)
{
    typedef typename Word<8 * sizeof(T)>::type W;
    const T* p = row + 3 * x0;
    if (x0 + 8 <= w && ((uintptr_t)p & (8 * sizeof(T) - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) unpack<T, 8>(gcp<W>(p)[i], v + 8 * i);
        return;
    }
#pragma unroll
    for (int px = 0; px < 8; ++px) {               // past the right edge: the last pixel again
        const int x = min(x0 + px, w - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[3 * px + ch] = gcp<T>(row)[3 * x + ch];
    }
}

// clamp(acc >> sh, 0, top), as a clamp of the accumulator and then the shift (same value for every acc); lim = ((top + 1) << sh) - 1
template <typename A> __device__ __forceinline__ int sat_shr(A acc, int sh, A lim)
{
    return (int)((acc < 0 ? (A)0 : (acc > lim ? lim : acc)) >> sh);
}

template <typename A> __device__ __forceinline__ A mul(int a, int b) { return (A)a * (A)b; }

constexpr bool has_chroma(int layout) { return layout != DEMFI_YUV_MONO; }

// one lane: row y x luma columns x0 .. x0+7 of one frame
template <typename T, int LAYOUT>
__global__ __launch_bounds__(NT) void yuvl_to_bgr_kernel(const T* __restrict__ src, int64_t src_stride, T* __restrict__ dst,
                                                        int64_t dst_stride, int n, int h, int w, ToBgrL k)
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
                                                               T* __restrict__ dst, int64_t dst_stride, int n, int h, int w, ToYuvL k)
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

int64_t payload_of(int layout, int h, int w)
{
    const int64_t hw = (int64_t)h * w;
    return layout == DEMFI_YUV_422 ? hw + 2 * (int64_t)h * ((w + 1) / 2) : layout == DEMFI_YUV_444 ? 3 * hw : hw;
}

int check_common(const char* fn, const void* src, const void* dst, int n, int h, int w, int depth, int layout, int matrix, int full_range,
                 int sample_bytes)
{
    if (!src || !dst || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    if (sample_bytes == 2 && (((uintptr_t)src & 1) || ((uintptr_t)dst & 1)))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: buffers of 16-bit samples must be 2-byte aligned", fn);
    if (h < 2 || w < 2 || h > 16384 || w > 16384)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: frame size %dx%d outside 2..16384", fn, h, w);
    if (depth < 8 || depth > 16)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: bit depth %d outside 8..16", fn, depth);
    if (layout != DEMFI_YUV_422 && layout != DEMFI_YUV_444 && layout != DEMFI_YUV_MONO)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: layout %d (4:2:2, 4:4:4 or mono; 4:2:0 has functions of its own)", fn, layout);
    if ((matrix != DEMFI_BT601 && matrix != DEMFI_BT709) || (full_range != 0 && full_range != 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: matrix %d / full_range %d", fn, matrix, full_range);
    return DEMFI_OK;
}

dim3 grid_for(int n, int h, int w)
{
    const int64_t lanes = (int64_t)h * ((w + SX - 1) / SX);
    return dim3((unsigned)((lanes + NT - 1) / NT), (unsigned)min(n, 65535));
}

template <typename T>
int to_bgr(const char* fn, const T* src, int64_t src_stride, T* dst, int64_t dst_stride, int n, int h, int w, int depth, int layout,
           int matrix, int full_range, void* stream)
{
    int st = check_common(fn, src, dst, n, h, w, depth, layout, matrix, full_range, (int)sizeof(T));
    if (st < 0) return st;
    const int64_t payload = payload_of(layout, h, w);
    if (n > 1 && (src_stride < payload || dst_stride < (int64_t)h * w * 3))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: strides %lld / %lld below the frame sizes %lld / %lld", fn, (long long)src_stride,
                               (long long)dst_stride, (long long)payload, (long long)h * w * 3);
    if (n == 0) return DEMFI_OK;
    const dim3 grid = grid_for(n, h, w);
    const ToBgrL k = to_bgr_coefs(matrix, full_range, depth);
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
    int st = check_common(fn, base, dst, n, h, w, depth, layout, matrix, full_range, (int)sizeof(T));
    if (st < 0) return st;
    if (!src_offsets)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL src_offsets", fn);
    const int64_t payload = payload_of(layout, h, w);
    if (n > 1 && dst_stride < payload)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride %lld below the payload %lld", fn, (long long)dst_stride, (long long)payload);
    if (n == 0) return DEMFI_OK;
    const dim3 grid = grid_for(n, h, w);
    const ToYuvL k = to_yuv_coefs(matrix, full_range, depth);
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
