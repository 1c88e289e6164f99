// Interlaced output of the Y4M video path (demfi_amd/interlace.py, --interlace): output payload r weaves two progressive payloads, the
// first field's frame and the second's, plane by plane: output row y of a plane comes from the first source when y mod 2 == q0, else
// from the second, and is low-passed vertically within the ONE source that owns it (rows clamped to the plane):
//   off:      c                                    linear:  (a + 2 c + b + 2) >> 2
//   complex:  v = clip((4 + 6 c + 2 (a + b) - a2 - b2) >> 3, 0, peak);  a + b > 2 c ? max(v, c) : min(v, c)
// with c = src[y], a / b = src[y -/+ 1], a2 / b2 = src[y -/+ 2], in signed 32-bit integers (|4 + 6 c + 2 (a + b) - a2 - b2| < 2^20,
// >> an arithmetic shift).  The definition is interlace.weave_payload_np; this kernel gives the same integers.
//
// A pure stream: no LDS, no atomics.  Row r of the launch has two byte offsets from base (equal for an odd tail).  blockIdx.y strides
// over the (payload, plane) pairs, blockIdx.x over chunks of NT items of the plane.
//
// The wide path: an item is a 16-byte column of the plane and a strip of STRIP = 8 consecutive output rows (items run along the row
// first, so a wave reads 1 KiB of a row at a stretch).  The thread walks down its strip and keeps the live rows of EACH source in
// registers, 2 HALO + 1 words of 16 bytes per source (HALO = 1 for linear, 2 for complex): every step loads row y + HALO of both
// sources (both are needed, each source owns every other output row and its filter reads the rows around them), filters the owner's
// window sample by sample and writes 16 bytes with one streaming store (the output is read by the copy engine only).  So every source
// row is loaded once per strip: the launch reads 2 P plus 2 HALO rows per strip and source, and writes P.  ``off`` loads only the
// owner's row: P read, P written.  The strip is short on purpose: a 720p payload is 10.8 k threads at 8 rows, a batch of them still far
// fewer than the part holds, and the halo rows are the neighbouring strips' own rows, read at about the same time, so they come from
// the L2 and not from memory.
//
// The wide path needs every row start on a 16-byte boundary: base + both offsets, every plane's first byte, cols * sample_bytes of every
// plane, dst and dst_stride.  The entry point decides that PER LAUNCH, from the host copy of the offsets and the plane list: 720p and
// 1080p 4:2:0 meet it on all three planes.  Otherwise (mono, odd widths, 1918-wide frames) the whole launch goes sample by sample: an
// item is one sample, consecutive lanes take consecutive samples of a row, and a thread reads the owner's 1, 3 or 5 samples itself
// (the rows repeat in the caches); the arithmetic is the same.
#include "common.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int MAXP = 3;                 // planes of a payload at most
constexpr int STRIP = 8;                // output rows a thread of the wide path walks down (even: a wave's rows share their parity)
enum { LP_OFF = 0, LP_LINEAR = 1, LP_COMPLEX = 2 };

struct Planes {
    int n;
    int rows[MAXP], cols[MAXP];
    int64_t start[MAXP];                // first sample of the plane in the payload
};

template <typename T> struct Samples;   // the 16 / sizeof(T) samples of a 16-byte word
template <> struct Samples<uint8_t> {
    static constexpr int N = 16;
    static __device__ __forceinline__ int at(const u4_t& v, int i) { return (int)((v[i >> 2] >> (8 * (i & 3))) & 0xffu); }
    static __device__ __forceinline__ void put(u4_t& v, int i, uint32_t x) { v[i >> 2] |= x << (8 * (i & 3)); }
};
template <> struct Samples<uint16_t> {
    static constexpr int N = 8;
    static __device__ __forceinline__ int at(const u4_t& v, int i) { return (int)((v[i >> 1] >> (16 * (i & 1))) & 0xffffu); }
    static __device__ __forceinline__ void put(u4_t& v, int i, uint32_t x) { v[i >> 1] |= x << (16 * (i & 1)); }
};

// the filter of one sample: a2, a, c, b, b2 = the owner's rows y-2 .. y+2 (clamped) at the sample's column
template <int MODE> __device__ __forceinline__ uint32_t lowpass(int a2, int a, int c, int b, int b2, int peak)
{
    if (MODE == LP_OFF) return (uint32_t)c;
    if (MODE == LP_LINEAR) return (uint32_t)((a + 2 * c + b + 2) >> 2);
    const int v = min(max((4 + 6 * c + 2 * (a + b) - a2 - b2) >> 3, 0), peak);
    return (uint32_t)(a + b > 2 * c ? max(v, c) : min(v, c));
}

// w[0 .. 2 HALO] = the rows y - HALO .. y + HALO of the owner at one 16-byte column
template <typename T, int MODE, int HALO> __device__ __forceinline__ u4_t filter_word(const u4_t* w, int peak)
{
    u4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < Samples<T>::N; ++i) {
        const int c = Samples<T>::at(w[HALO], i);
        const int a = HALO >= 1 ? Samples<T>::at(w[HALO - 1], i) : c, b = HALO >= 1 ? Samples<T>::at(w[HALO >= 1 ? HALO + 1 : 0], i) : c;
        const int a2 = HALO >= 2 ? Samples<T>::at(w[0], i) : c, b2 = HALO >= 2 ? Samples<T>::at(w[2 * HALO], i) : c;
        Samples<T>::put(o, i, lowpass<MODE>(a2, a, c, b, b2, peak));
    }
    return o;
}

__device__ __forceinline__ int clamp_row(int y, int rows) { return min(max(y, 0), rows - 1); }

// grid: x = chunks of NT items of a plane (strided), y = (payload, plane) pairs (strided).  Wide path: item = strip * words + word.
template <typename T, int MODE>
__global__ __launch_bounds__(NT) void payload_weave_wide_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n,
                                                               Planes pl, int peak, int q0, uint8_t* __restrict__ dst,
                                                               int64_t dst_stride)
{
    constexpr int HALO = MODE == LP_OFF ? 0 : MODE == LP_LINEAR ? 1 : 2;
    constexpr int R = 2 * HALO + 1;
    constexpr int es = (int)sizeof(T);
    for (int rp = blockIdx.y; rp < n * pl.n; rp += gridDim.y) {
        const int r = rp / pl.n, p = rp - r * pl.n;
        const int rows = pl.rows[p];
        const int64_t pitch = (int64_t)pl.cols[p] * es;                      // a multiple of 16
        const uint32_t words = (uint32_t)(pitch >> 4);
        const uint32_t items = words * (uint32_t)((rows + STRIP - 1) / STRIP);
        const uint8_t* A = base + offs[2 * r] + pl.start[p] * es;
        const uint8_t* B = base + offs[2 * r + 1] + pl.start[p] * es;
        uint8_t* out = dst + (int64_t)r * dst_stride + pl.start[p] * es;
        for (uint32_t it = blockIdx.x * NT + threadIdx.x; it < items; it += gridDim.x * NT) {
            const uint32_t s = it / words, c = it - s * words;
            const int y0 = (int)s * STRIP, y1 = min(rows, y0 + STRIP);
            const uint8_t* a = A + (int64_t)c * 16;
            const uint8_t* b = B + (int64_t)c * 16;
            uint8_t* o = out + (int64_t)c * 16;
            if (HALO == 0) {
                for (int y = y0; y < y1; ++y) {
                    const u4_t v = *gcp<u4_t>(((y & 1) == q0 ? a : b) + y * pitch);
                    __builtin_nontemporal_store(v, gp<u4_t>(o + y * pitch));
                }
            } else {
                u4_t wa[R], wb[R];
#pragma unroll
                for (int k = 0; k < R - 1; ++k) {
                    const int64_t at = clamp_row(y0 - HALO + k, rows) * pitch;
                    wa[k] = *gcp<u4_t>(a + at);
                    wb[k] = *gcp<u4_t>(b + at);
                }
                for (int y = y0; y < y1; ++y) {
                    const int64_t at = clamp_row(y + HALO, rows) * pitch;
                    wa[R - 1] = *gcp<u4_t>(a + at);
                    wb[R - 1] = *gcp<u4_t>(b + at);
                    const u4_t v = (y & 1) == q0 ? filter_word<T, MODE, HALO>(wa, peak) : filter_word<T, MODE, HALO>(wb, peak);
                    __builtin_nontemporal_store(v, gp<u4_t>(o + y * pitch));
#pragma unroll
                    for (int k = 0; k < R - 1; ++k) { wa[k] = wa[k + 1]; wb[k] = wb[k + 1]; }
                }
            }
        }
    }
}

// the sample-by-sample path: item = one sample of the plane, y * cols + x
template <typename T, int MODE>
__global__ __launch_bounds__(NT) void payload_weave_sample_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n,
                                                                 Planes pl, int peak, int q0, uint8_t* __restrict__ dst, int64_t dst_stride)
{
    constexpr int es = (int)sizeof(T);
    for (int rp = blockIdx.y; rp < n * pl.n; rp += gridDim.y) {
        const int r = rp / pl.n, p = rp - r * pl.n;
        const int rows = pl.rows[p];
        const uint32_t cols = (uint32_t)pl.cols[p], items = cols * (uint32_t)rows;
        const auto A = gcp<T>(base + offs[2 * r] + pl.start[p] * es);
        const auto B = gcp<T>(base + offs[2 * r + 1] + pl.start[p] * es);
        const auto out = gp<T>(dst + (int64_t)r * dst_stride + pl.start[p] * es);
        for (uint32_t it = blockIdx.x * NT + threadIdx.x; it < items; it += gridDim.x * NT) {
            const int y = (int)(it / cols);
            const uint32_t x = it - (uint32_t)y * cols;
            const auto src = ((y & 1) == q0 ? A : B) + x;
            const int c = src[(int64_t)y * cols];
            int a = c, b = c, a2 = c, b2 = c;
            if (MODE != LP_OFF) {
                a = src[(int64_t)clamp_row(y - 1, rows) * cols];
                b = src[(int64_t)clamp_row(y + 1, rows) * cols];
            }
            if (MODE == LP_COMPLEX) {
                a2 = src[(int64_t)clamp_row(y - 2, rows) * cols];
                b2 = src[(int64_t)clamp_row(y + 2, rows) * cols];
            }
            out[it] = (T)lowpass<MODE>(a2, a, c, b, b2, peak);
        }
    }
}

}  // namespace

extern "C" int demfi_payload_weave(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes,
                                   int n_planes, int sample_bytes, int peak, int q0, int lowpass, uint8_t* dst, int64_t dst_stride,
                                   void* stream)
{
    const char* fn = "demfi_payload_weave";
    if (n <= 0) return DEMFI_OK;
    if (!base || !offsets || !offsets_dev || !planes || !dst) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n_planes < 1 || n_planes > MAXP) return demfi_set_error(DEMFI_ERR_ARG, "%s: %d planes (1..%d)", fn, n_planes, MAXP);
    if (sample_bytes != 1 && sample_bytes != 2)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d bytes per sample (1 or 2)", fn, sample_bytes);
    if (peak < 1 || peak > 65535 || (sample_bytes == 1 && peak > 255))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: peak=%d outside 1..%d", fn, peak, sample_bytes == 1 ? 255 : 65535);
    if (q0 != 0 && q0 != 1) return demfi_set_error(DEMFI_ERR_ARG, "%s: q0=%d (0 or 1)", fn, q0);
    if (lowpass < LP_OFF || lowpass > LP_COMPLEX) return demfi_set_error(DEMFI_ERR_ARG, "%s: low-pass mode %d (0, 1 or 2)", fn, lowpass);
    Planes pl = {};
    pl.n = n_planes;
    int64_t P = 0;
    uintptr_t low = (uintptr_t)base | (uintptr_t)dst | (uintptr_t)dst_stride;    // the low bits of every row start the kernel forms
    for (int p = 0; p < n_planes; ++p) {
        const int rows = planes[2 * p], cols = planes[2 * p + 1];
        if (rows < 1 || cols < 1 || rows > 32768 || cols > 32768)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d is %d x %d (1..32768 each)", fn, p, rows, cols);
        pl.rows[p] = rows, pl.cols[p] = cols, pl.start[p] = P;
        low |= (uintptr_t)(P * sample_bytes) | (uintptr_t)((int64_t)cols * sample_bytes);
        P += (int64_t)rows * cols;
    }
    if (dst_stride < P * sample_bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride=%lld below the %lld bytes of a payload", fn, (long long)dst_stride,
                               (long long)(P * sample_bytes));
    uintptr_t odd = (uintptr_t)base | (uintptr_t)dst | (uintptr_t)dst_stride;
    for (int64_t i = 0; i < 2 * (int64_t)n; ++i) {
        if (offsets[i] < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: row %lld offset %d is %lld", fn, (long long)(i / 2), (int)(i & 1),
                                                   (long long)offsets[i]);
        low |= (uintptr_t)offsets[i];
        odd |= (uintptr_t)offsets[i];
    }
    if (sample_bytes == 2 && (odd & 1)) return demfi_set_error(DEMFI_ERR_ARG, "%s: 16-bit samples at an odd address or stride", fn);
    const bool wide = (low & 15) == 0;
    const int64_t pairs = (int64_t)n * n_planes;
    const hipStream_t st = (hipStream_t)stream;
    if (wide) {
        int64_t most = 0;
        for (int p = 0; p < n_planes; ++p)
            most = max(most, ((int64_t)pl.cols[p] * sample_bytes / 16) * ((pl.rows[p] + STRIP - 1) / STRIP));
        const dim3 grid((unsigned)min((most + NT - 1) / NT, (int64_t)4096), (unsigned)min(pairs, (int64_t)4096));
#define WEAVE_WIDE(T, M) \
    hipLaunchKernelGGL((payload_weave_wide_kernel<T, M>), grid, dim3(NT), 0, st, base, offsets_dev, n, pl, peak, q0, dst, dst_stride)
        if (sample_bytes == 1) {
            if (lowpass == LP_OFF) WEAVE_WIDE(uint8_t, LP_OFF); else if (lowpass == LP_LINEAR) WEAVE_WIDE(uint8_t, LP_LINEAR); else WEAVE_WIDE(uint8_t, LP_COMPLEX);
        } else {
            if (lowpass == LP_OFF) WEAVE_WIDE(uint16_t, LP_OFF); else if (lowpass == LP_LINEAR) WEAVE_WIDE(uint16_t, LP_LINEAR); else WEAVE_WIDE(uint16_t, LP_COMPLEX);
        }
#undef WEAVE_WIDE
    } else {
        int64_t most = 0;
        for (int p = 0; p < n_planes; ++p) most = max(most, (int64_t)pl.rows[p] * pl.cols[p]);
        const dim3 grid((unsigned)min((most + NT - 1) / NT, (int64_t)4096), (unsigned)min(pairs, (int64_t)4096));
#define WEAVE_SAMPLE(T, M) \
    hipLaunchKernelGGL((payload_weave_sample_kernel<T, M>), grid, dim3(NT), 0, st, base, offsets_dev, n, pl, peak, q0, dst, dst_stride)
        if (sample_bytes == 1) {
            if (lowpass == LP_OFF) WEAVE_SAMPLE(uint8_t, LP_OFF); else if (lowpass == LP_LINEAR) WEAVE_SAMPLE(uint8_t, LP_LINEAR); else WEAVE_SAMPLE(uint8_t, LP_COMPLEX);
        } else {
            if (lowpass == LP_OFF) WEAVE_SAMPLE(uint16_t, LP_OFF); else if (lowpass == LP_LINEAR) WEAVE_SAMPLE(uint16_t, LP_LINEAR); else WEAVE_SAMPLE(uint16_t, LP_COMPLEX);
        }
#undef WEAVE_SAMPLE
    }
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
