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
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int STRIP = 8;                // output rows a thread of the wide path walks down (even: a wave's rows share their parity)
enum { LP_OFF = 0, LP_LINEAR = 1, LP_COMPLEX = 2 };

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

// grid: x = chunks of NT items of a plane (strided), y = (payload, plane) pairs (strided).  Wide path: item = strip * words + word.
template <typename T, int MODE>
__global__ __launch_bounds__(NT) void payload_weave_wide_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n,
                                                               PlaneList pl, int peak, int q0, uint8_t* __restrict__ dst,
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
                                                                 PlaneList pl, int peak, int q0, uint8_t* __restrict__ dst, int64_t dst_stride)
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
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (int st = check_peak(fn, peak, sample_bytes)) return st;
    if (int st = check_flag(fn, "q0", q0)) return st;
    if (lowpass < LP_OFF || lowpass > LP_COMPLEX) return demfi_set_error(DEMFI_ERR_ARG, "%s: low-pass mode %d (0, 1 or 2)", fn, lowpass);
    PlaneSet ps;
    if (int st = parse_planes(fn, planes, n_planes, 32768, (int64_t)32768 * 32768, false, &ps)) return st;
    const PlaneList& pl = ps.pl;
    if (int st = check_dst_stride(fn, dst_stride, ps.P * sample_bytes)) return st;
    uintptr_t low = (uintptr_t)base | (uintptr_t)dst | (uintptr_t)dst_stride;    // the low bits of every row start the kernel forms
    if (int st = walk_offsets(fn, offsets, n, 2, 2, OFFS_ALL, 0, NO_LIMIT, 0, &low)) return st;
    if (int st = check_even(fn, sample_bytes, low)) return st;
    for (int p = 0; p < n_planes; ++p) low |= (uintptr_t)(pl.start[p] * sample_bytes) | (uintptr_t)((int64_t)pl.cols[p] * sample_bytes);
    const bool wide = (low & 15) == 0;
    int64_t most = 0;                                                    // items of the largest plane: 16-byte columns x strips, or samples
    for (int p = 0; p < n_planes; ++p)
        most = max(most, wide ? ((int64_t)pl.cols[p] * sample_bytes / 16) * ((pl.rows[p] + STRIP - 1) / STRIP) : (int64_t)pl.rows[p] * pl.cols[p]);
    const dim3 grid = planes_grid(most, NT, n, n_planes);
    by_sample(sample_bytes, [&](auto t) {
        by_int<LP_OFF, LP_COMPLEX>(lowpass, [&](auto m) {
            if (wide)
                hipLaunchKernelGGL((payload_weave_wide_kernel<TAG_TYPE(t), TAG_VALUE(m)>), grid, dim3(NT), 0, (hipStream_t)stream, base, offsets_dev,
                                   n, pl, peak, q0, dst, dst_stride);
            else
                hipLaunchKernelGGL((payload_weave_sample_kernel<TAG_TYPE(t), TAG_VALUE(m)>), grid, dim3(NT), 0, (hipStream_t)stream, base,
                                   offsets_dev, n, pl, peak, q0, dst, dst_stride);
        });
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
