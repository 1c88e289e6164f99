// Temporal denoising of the Y4M video path in front of the network (demfi_amd/denoise.py, --denoise): frame i of a launch has TAPS =
// 2 R + 1 source payloads in frame order, the centre in the middle, and every stored sample (bytes, or little-endian 16-bit samples) of
// its output is the rounded mean of the centre's sample and of those neighbours' samples that the serial walk of each side accepts:
// a side walks outward from the centre, adds up d = |x - c|, and stops for good at the first d > A, the first accumulated d > B, or the
// first absent payload.  out = (2 sum + n) / (2 n), n = 1 .. 7.  The definition is denoise.denoise_payload_np; this kernel gives the same
// integers.
//
// A pure stream: no LDS, no atomics, no tables.  Row i of the launch has TAPS byte offsets into src (-1: absent) and one byte offset into
// dst; they are the same for every lane of a workgroup, so they and the branches on them stay scalar.  A thread owns 16 output bytes: it
// issues the 16-byte loads of the centre and of every present neighbour (a wave reads 1 KiB of a payload at a stretch), walks the 16 or 8
// samples in registers and writes 16 bytes with one plain store -- the conversion to frames reads them next, so they should stay in L2.
// The division by 2 n is a multiplication with MAGIC[n] = 2^32 / (2 n) + 1 and a shift by 32: v = 2 sum + n < 2^20 and MAGIC[n] * 2 n -
// 2^32 <= 2 n <= 14, so the error term v * 14 / 2^32 is below 1 / (2 n) and the quotient is exact (tests/test_denoise.py walks every n
// and every sum).  n differs from sample to sample; the constant is picked by six selects, not looked up.
//
// The vector form needs src + every present offset and dst + every destination offset on 16-byte boundaries; the entry point decides that
// from the host copy of the offsets, for the launch as a whole.  The last P * es mod 16 bytes of a payload go sample by sample.  Otherwise
// (mono frames of odd size have an odd P) a thread owns one sample at a time, consecutive lanes consecutive samples; the arithmetic is the
// same.  Every byte offset and every index inside a payload is 64-bit: the payload ring of 8K 16-bit video passes 4 GiB.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup: 4 KiB of a payload
constexpr int NMAX = 64;                // frames of a launch at most

// (2 s + n) / (2 n), exact for s <= n * 65535, n = 1 .. 7
__device__ __forceinline__ uint32_t mean_of(uint32_t s, uint32_t n)
{
    // MAGIC[n - 1] = 2^32 / (2 n) + 1 (demfi_amd/denoise.py MAGIC; tests/test_denoise.py reads the next line)
    constexpr uint32_t MAGIC[7] = {2147483649u, 1073741825u, 715827883u, 536870913u, 429496730u, 357913942u, 306783379u};
    uint32_t m = MAGIC[0];
#pragma unroll
    for (uint32_t k = 2; k <= 7; ++k) m = n == k ? MAGIC[k - 1] : m;
    return __umulhi(2u * s + n, m);
}

// One step of a side's walk: the sample x of the next frame outward.  alive: the side has not stopped yet.
__device__ __forceinline__ void step(uint32_t c, uint32_t x, uint32_t A, uint32_t B, uint32_t& acc, bool& alive, uint32_t& sum, uint32_t& n)
{
    const uint32_t d = x > c ? x - c : c - x;
    acc += d;
    alive = alive && d <= A && acc <= B;
    sum += alive ? x : 0u;
    n += alive ? 1u : 0u;
}

// grid: x = chunks of NT units of a payload (strided), y = frames (strided).  A unit is a 16-byte word (VEC) or one sample.  T: the sample
// type; R: frames on each side; P counts samples, offsets count bytes.  Row r of offs: 2 R + 1 source offsets, then the destination's.
template <typename T, int R, bool VEC>
__global__ __launch_bounds__(NT) void payload_denoise_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offs, int n, int64_t P,
                                                            uint32_t A, uint32_t B, uint8_t* __restrict__ dst)
{
    constexpr int N = Samples<T>::N, TAPS = 2 * R + 1;
    const int64_t full = P / N;                                          // whole 16-byte words of a payload
    const int64_t units = VEC ? full + (P - full * N) : P;               // VEC: the words, then the samples of the tail one by one
    for (int r = blockIdx.y; r < n; r += gridDim.y) {
        const int64_t* ro = offs + (int64_t)r * (TAPS + 1);
        if (ro[R] < 0) continue;                                         // refused by the entry point; nothing to denoise
        const uint8_t* centre = src + ro[R];
        uint8_t* out = dst + ro[TAPS];
        // side 0 walks f-1, f-2, ..; side 1 walks f+1, f+2, ..; cnt: the present payloads of a side, which end at the first absent one
        int64_t so[2][R];
        int cnt[2] = {0, 0};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bool there = true;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                so[s][j] = ro[s ? R + 1 + j : R - 1 - j];
                there = there && so[s][j] >= 0;
                cnt[s] += there ? 1 : 0;
            }
        }
        for (int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x; c < units; c += (int64_t)gridDim.x * NT) {
            if (VEC && c < full) {
                u4_t v[2][R];
                const u4_t vc = *gcp<u4_t>(centre + c * 16);
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < R; ++j)                          // all loads before the walk
                        if (j < cnt[s]) v[s][j] = *gcp<u4_t>(src + so[s][j] + c * 16);
                u4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const uint32_t x0 = Samples<T>::at(vc, i);
                    uint32_t sum = x0, k = 1;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        uint32_t acc = 0;
                        bool alive = true;
#pragma unroll
                        for (int j = 0; j < R; ++j)
                            if (j < cnt[s]) step(x0, Samples<T>::at(v[s][j], i), A, B, acc, alive, sum, k);
                    }
                    Samples<T>::put(o, i, mean_of(sum, k));
                }
                *gp<u4_t>(out + c * 16) = o;
            } else {                                                     // one sample: consecutive lanes, consecutive samples
                const int64_t p = VEC ? full * N + (c - full) : c;
                const uint32_t x0 = gcp<T>(centre)[p];
                uint32_t x[2][R];
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < R; ++j)
                        if (j < cnt[s]) x[s][j] = gcp<T>(src + so[s][j])[p];
                uint32_t sum = x0, k = 1;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    uint32_t acc = 0;
                    bool alive = true;
#pragma unroll
                    for (int j = 0; j < R; ++j)
                        if (j < cnt[s]) step(x0, x[s][j], A, B, acc, alive, sum, k);
                }
                gp<T>(out)[p] = (T)mean_of(sum, k);
            }
        }
    }
}

}  // namespace

extern "C" int demfi_payload_denoise(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int64_t* offsets_dev, int n, int taps,
                                     int64_t P, int sample_bytes, int thr_a, int thr_b, uint8_t* dst, int64_t dst_bytes, void* stream)
{
    const char* fn = "demfi_payload_denoise";
    if (!src || !offsets || !offsets_dev || !dst) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n < 0 || n > NMAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d outside 0..%d", fn, n, NMAX);
    if (taps != 3 && taps != 5 && taps != 7) return demfi_set_error(DEMFI_ERR_ARG, "%s: taps=%d (3, 5 or 7)", fn, taps);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    const int peak = sample_bytes == 1 ? 255 : 65535;
    if (thr_a < 0 || thr_b < thr_a || thr_b > peak)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: thresholds A=%d, B=%d need 0 <= A <= B <= %d", fn, thr_a, thr_b, peak);
    if (P < 1 || P > ((int64_t)1 << 40)) return demfi_set_error(DEMFI_ERR_ARG, "%s: P=%lld samples", fn, (long long)P);
    const int64_t pb = P * sample_bytes;
    if (src_bytes < pb || dst_bytes < pb)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: buffers of %lld and %lld bytes for payloads of %lld", fn, (long long)src_bytes,
                               (long long)dst_bytes, (long long)pb);
    if (int st = check_even(fn, sample_bytes, (uintptr_t)src | (uintptr_t)dst)) return st;
    if ((uintptr_t)src < (uintptr_t)dst + (uintptr_t)dst_bytes && (uintptr_t)dst < (uintptr_t)src + (uintptr_t)src_bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: the source and the destination buffer overlap", fn);
    const int R = taps / 2, width = taps + 1;
    uintptr_t low = 0;                                                   // the low bits of every address the kernel forms
    // the sources: absent anywhere but at the centre, a whole payload inside src; then the destinations, inside dst
    if (int st = walk_offsets(fn, offsets, n, width, taps, OFFS_BUT_CENTRE, R, src_bytes - pb, (uintptr_t)src, &low)) return st;
    if (int st = walk_offsets(fn, offsets + taps, n, width, 1, OFFS_ALL, 0, dst_bytes - pb, (uintptr_t)dst, &low)) return st;
    if (int st = check_even(fn, sample_bytes, low)) return st;
    for (int i = 0; i < n; ++i) {
        const int64_t d = offsets[(int64_t)i * width + taps];
        for (int j = 0; j < i; ++j) {
            const int64_t e = offsets[(int64_t)j * width + taps];
            if (e > d - pb && e < d + pb)
                return demfi_set_error(DEMFI_ERR_ARG, "%s: frames %d and %d write the same destination", fn, j, i);
        }
    }
    if (n == 0) return DEMFI_OK;
    const bool vec = (low & 15) == 0;
    const dim3 grid = rows_grid(stream_units(P, sample_bytes, vec), NT, n);
    by_sample(sample_bytes, [&](auto t) {
        by_int<1, 3>(R, [&](auto r) {
            by_bool(vec, [&](auto v) {
                hipLaunchKernelGGL((payload_denoise_kernel<TAG_TYPE(t), TAG_VALUE(r), TAG_VALUE(v)>), grid, dim3(NT), 0, (hipStream_t)stream, src,
                                   offsets_dev, n, P, (uint32_t)thr_a, (uint32_t)thr_b, dst);
            });
        });
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
