// What the colour conversions of the Y4M stream edge share (yuv.hip, yuv_family.hip, deint.hip, colour.hip): the matrix coefficients,
// the argument check and launch grid of the host side, and the device-side access to samples of either type.  The packed-word typedefs,
// Acc<T> and the small argument checks are payload_kit.h's, which every payload stage shares.
//
// The definition of every conversion is numpy code in demfi_amd/y4m.py; the kernels match it bit for bit.  Samples and BGR values at
// bit depth d hold 0 .. peak = 2^d - 1, in uint8 (d = 8) or uint16 (d = 8 .. 16).  With s = 2^(d-8): limited range is Y 16s .. 235s
// and C 16s .. 240s, the Y offset 16s, the chroma centre 2^(d-1), the scale factors peak / (219 s), peak / (224 s) and their
// inverses.  Coefficients are rounded half up to Q(8+d) from the same float64 expressions as in y4m.py (built with
// -ffp-contract=off); chroma enters the matrix in 1/16 units; ONE round-half-up, clamp to [0, peak].  d = 8 gives the Q16
// coefficients of the 8-bit kernels exactly (255 / (219 * 1) and 219 * 1 / 255 are the same float64 values as 255 / 219, 219 / 255).
#pragma once
#include "payload_kit.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SX = 8;                 // luma pixels per lane strip

struct ToBgr {                        // Q(8+d); chroma arrives in 1/16 units -> one shift by sh = 8 + d + 4
    int cy, r_cr, g_cb, g_cr, b_cb, yoff, mid16, sh, peak;
};
struct ToYuv {                        // Q(8+d) over d-bit B, G, R; q = 8 + d; mid = 2^(d-1)
    int y_r, y_g, y_b, cb_r, cb_g, cb_b, cr_r, cr_g, cr_b, yoff, mid, q, peak;
};

inline int fixq(double c, int q) { return (int)floor(c * (double)(1 << q) + 0.5); }

inline void kr_kb(int matrix, double* kr, double* kb)
{
    if (matrix == DEMFI_BT709) { *kr = 0.2126; *kb = 0.0722; }
    else { *kr = 0.299; *kb = 0.114; }
}

// y4m.py: to_bgr_coefs_depth
inline ToBgr to_bgr_coefs(int matrix, int full, int d)
{
    double kr, kb;
    kr_kb(matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    const int q = 8 + d, s = 1 << (d - 8), peak = (1 << d) - 1;
    const double ys = full ? 1.0 : peak / (219.0 * s), cs = full ? 1.0 : peak / (224.0 * s);
    ToBgr c;
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
inline ToYuv to_yuv_coefs(int matrix, int full, int d)
{
    double kr, kb;
    kr_kb(matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    const int q = 8 + d, s = 1 << (d - 8), peak = (1 << d) - 1;
    const double ys = full ? 1.0 : 219.0 * s / peak, cs = full ? 1.0 : 224.0 * s / peak;
    ToYuv c;
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

// samples of one payload: Y [h,w], then Cb and Cr of the layout's chroma shape
inline int64_t payload_of(int layout, int h, int w)
{
    const int64_t hw = (int64_t)h * w, cw = (w + 1) / 2;
    return layout == DEMFI_YUV_420 ? hw + 2 * (int64_t)((h + 1) / 2) * cw
         : layout == DEMFI_YUV_422 ? hw + 2 * (int64_t)h * cw
         : layout == DEMFI_YUV_444 ? 3 * hw : hw;
}

// The arguments every conversion takes (the layouts family checks its layout argument itself: only there can it be wrong).
inline int check_args(const char* fn, const void* src, const void* dst, int n, int h, int w, int depth, int matrix, int full_range,
                      int sample_bytes)
{
    if (!src || !dst || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    if (sample_bytes == 2 && (((uintptr_t)src & 1) || ((uintptr_t)dst & 1)))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: buffers of 16-bit samples must be 2-byte aligned", fn);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (depth < 8 || depth > 16)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: bit depth %d outside 8..16", fn, depth);
    if ((matrix != DEMFI_BT601 && matrix != DEMFI_BT709) || (full_range != 0 && full_range != 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: matrix %d / full_range %d", fn, matrix, full_range);
    return DEMFI_OK;
}

// one lane per strip of SX luma pixels of each of `rows` rows (4:2:0: chroma rows), frames along y
inline dim3 grid_for(int n, int rows, int w)
{
    const int64_t lanes = (int64_t)rows * ((w + SX - 1) / SX);
    return dim3((unsigned)((lanes + NT - 1) / NT), (unsigned)min(n, 65535));
}

// ---- the two sample types -------------------------------------------------------------------------------------------------
// Acc<T>, the accumulator of a sample type, is payload_kit.h's
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

}  // namespace
