// Synthesized motion blur of the Y4M video path (demfi_amd/shutter.py, --shutter): written payload r is the rounded box average of
// the k_r fine payloads it keeps, out[p] = (2 * sum x_g[p] + k) / (2 k) per stored sample (bytes, or little-endian 16-bit samples).
// The definition is shutter.mix_np; this kernel gives the same integers.
//
// A pure stream: no LDS, no atomics.  Row r of the launch has smax byte offsets from base, the kept ones first and -1 behind them;
// they and k are the same for every lane of a workgroup, so they stay in scalar registers.  A thread owns 16 output bytes: it loads
// the 16 bytes of each kept source (a wave reads 1 KiB of a source at a stretch), adds them up sample by sample in 32-bit
// integers (32 x 65535 < 2^21), divides and writes 16 bytes with one store.  The division by 2 k is a multiplication with
// magic(k) = 2^32 / (2 k) + 1 and a shift by 32: n = 2 sum + k < 2^22 and magic(k) * 2 k - 2^32 <= 2 k <= 64, so the error term
// n * 64 / 2^32 is below 1 / (2 k) and the quotient is exact (tests/test_shutter.py walks every k and every sum).  The output is
// written once and read by the copy engine only: a streaming store keeps the L2 for the sources, which the gather has just written.
//
// The vector form needs base + every kept offset, dst and dst_stride on 16-byte boundaries; the entry point decides that from the
// host copy of the offsets, for the launch as a whole.  The last P * es mod 16 bytes of a row go sample by sample.  Otherwise (mono
// frames of odd size have an odd P) a thread owns one sample at a time, consecutive lanes consecutive samples, so a wave still reads
// and writes one contiguous run per source; the arithmetic is the same.
#include "common.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup: 4 KiB of a row
constexpr int SMAX = 32;                // kept sources of a row at most

struct Magic { uint32_t m[SMAX + 1]; };
constexpr Magic make_magic()
{
    Magic t = {};
    for (int k = 1; k <= SMAX; ++k) t.m[k] = (uint32_t)((1ull << 32) / (2u * k)) + 1u;
    return t;
}
__constant__ Magic kMagic = make_magic();

// (2 s + k) / (2 k), exact for s <= k * 65535, k <= 32
__device__ __forceinline__ uint32_t mix_div(uint32_t s, uint32_t k, uint32_t magic) { return __umulhi(2u * s + k, magic); }

template <typename T> struct Samples;   // the 16 / sizeof(T) samples of a 16-byte word
template <> struct Samples<uint8_t> {
    static constexpr int N = 16;
    static __device__ __forceinline__ uint32_t at(const u4_t& v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xffu; }
    static __device__ __forceinline__ void put(u4_t& v, int i, uint32_t x) { v[i >> 2] |= x << (8 * (i & 3)); }
};
template <> struct Samples<uint16_t> {
    static constexpr int N = 8;
    static __device__ __forceinline__ uint32_t at(const u4_t& v, int i) { return (v[i >> 1] >> (16 * (i & 1))) & 0xffffu; }
    static __device__ __forceinline__ void put(u4_t& v, int i, uint32_t x) { v[i >> 1] |= x << (16 * (i & 1)); }
};

// grid: x = chunks of NT units of a row (strided), y = rows (strided).  A unit is a 16-byte word (VEC) or one sample.  T: the sample type;
// P counts samples, offsets count bytes.
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void payload_mix_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n, int smax,
                                                        int64_t P, uint8_t* __restrict__ dst, int64_t dst_stride)
{
    constexpr int N = Samples<T>::N;
    const int64_t full = P / N;                                          // whole 16-byte words of a row
    const int64_t units = VEC ? full + (P - full * N) : P;               // VEC: the words, then the samples of the tail one by one
    for (int r = blockIdx.y; r < n; r += gridDim.y) {
        const int64_t* ro = offs + (int64_t)r * smax;
        int k = 0;
        while (k < smax && ro[k] >= 0) ++k;                              // kept ones first
        if (k == 0) continue;                                            // refused by the entry point; nothing to average
        const uint32_t magic = kMagic.m[k];
        uint8_t* out = dst + (int64_t)r * dst_stride;
        for (int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x; c < units; c += (int64_t)gridDim.x * NT) {
            if (VEC && c < full) {
                uint32_t acc[N];
#pragma unroll
                for (int i = 0; i < N; ++i) acc[i] = 0;
                int j = 0;
                for (; j + 4 <= k; j += 4) {                             // four loads in flight
                    u4_t v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = *gcp<u4_t>(base + ro[j + u] + c * 16);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int i = 0; i < N; ++i) acc[i] += Samples<T>::at(v[u], i);
                }
                for (; j < k; ++j) {
                    const u4_t v = *gcp<u4_t>(base + ro[j] + c * 16);
#pragma unroll
                    for (int i = 0; i < N; ++i) acc[i] += Samples<T>::at(v, i);
                }
                u4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < N; ++i) Samples<T>::put(o, i, mix_div(acc[i], (uint32_t)k, magic));
                __builtin_nontemporal_store(o, gp<u4_t>(out + c * 16));
            } else {                                                     // one sample: consecutive lanes, consecutive samples
                const int64_t s = VEC ? full * N + (c - full) : c;
                uint32_t acc = 0;
                for (int j = 0; j < k; ++j) acc += gcp<T>(base + ro[j])[s];
                gp<T>(out)[s] = (T)mix_div(acc, (uint32_t)k, magic);
            }
        }
    }
}

}  // namespace

extern "C" int demfi_payload_mix(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, int smax, int64_t P,
                                 int sample_bytes, uint8_t* dst, int64_t dst_stride, void* stream)
{
    const char* fn = "demfi_payload_mix";
    if (n <= 0) return DEMFI_OK;
    if (!base || !offsets || !offsets_dev || !dst) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (smax < 1 || smax > SMAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: smax=%d outside 1..%d", fn, smax, SMAX);
    if (sample_bytes != 1 && sample_bytes != 2)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d bytes per sample (1 or 2)", fn, sample_bytes);
    if (P < 1 || P > ((int64_t)1 << 40)) return demfi_set_error(DEMFI_ERR_ARG, "%s: P=%lld samples", fn, (long long)P);
    if (dst_stride < P * sample_bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride=%lld below the %lld bytes of a payload", fn, (long long)dst_stride,
                               (long long)(P * sample_bytes));
    uintptr_t low = (uintptr_t)dst | (uintptr_t)dst_stride;              // the low bits of every address the kernel forms
    for (int r = 0; r < n; ++r) {
        const int64_t* ro = offsets + (int64_t)r * smax;
        if (ro[0] < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: row %d keeps no source (its first offset is %lld)", fn, r, (long long)ro[0]);
        bool ended = false;
        for (int j = 0; j < smax; ++j) {
            if (ro[j] < -1) return demfi_set_error(DEMFI_ERR_ARG, "%s: row %d offset %d is %lld", fn, r, j, (long long)ro[j]);
            if (ro[j] < 0) ended = true;
            else if (ended) return demfi_set_error(DEMFI_ERR_ARG, "%s: row %d has a kept offset behind a -1", fn, r);
            else low |= (uintptr_t)(base + ro[j]);
        }
    }
    if (sample_bytes == 2 && (low & 1)) return demfi_set_error(DEMFI_ERR_ARG, "%s: 16-bit samples at an odd address or stride", fn);
    const bool vec = (low & 15) == 0;
    const int per = 16 / sample_bytes;                                   // samples of a 16-byte word
    const int64_t units = vec ? P / per + P % per : P;                   // what the kernel strides over: words and tail samples, or samples
    const int64_t chunks = (units + NT - 1) / NT;
    const dim3 grid((unsigned)min(chunks, (int64_t)4096), (unsigned)min(n, 4096));
    const hipStream_t st = (hipStream_t)stream;
#define MIX_LAUNCH(T, V) \
    hipLaunchKernelGGL((payload_mix_kernel<T, V>), grid, dim3(NT), 0, st, base, offsets_dev, n, smax, P, dst, dst_stride)
    if (sample_bytes == 1) { if (vec) MIX_LAUNCH(uint8_t, true); else MIX_LAUNCH(uint8_t, false); }
    else                   { if (vec) MIX_LAUNCH(uint16_t, true); else MIX_LAUNCH(uint16_t, false); }
#undef MIX_LAUNCH
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

// ---- weighted windows (--shutter-window, shutter.window_weights) -----------------------------------------------------------------
// out[p] = (2 * sum_j w_j x_j[p] + W_k) / (2 W_k) over the k kept sources of a row, W_k = w_0 + .. + w_(k-1): the kept sources are
// always a prefix of the row's S samples, so one weight vector serves every row of a launch and W_k is a prefix sum.  The kernel has
// the shape of the box kernel above (16 bytes a thread or one sample, rows and chunks strided, streaming store, no LDS, no atomics).
// The weights, W_k and the divisor constants of every k come by value in the kernel's arguments: uniform, read with scalar loads.
// With sum w <= 4096 the numerator 2 * 4096 * 65535 + 4096 stays below 2^30.  The division by 2 W is shutter.magic_w: with
// s = bit_length(n_max * 2 W), n_max = 2 W 65535 + W, and M = 2^s / (2 W) + 1, M * 2 W exceeds 2^s by at most 2 W, so n M / 2^s is off
// by less than n_max * 2 W / (2 W * 2^s) < 1 / (2 W) quotient steps: exact.  Folded to one multiply-high: (n * mul) >> 32 >> sh with
// mul = M << (32 - s), sh = 0 for s < 32, else mul = M (< 2^30), sh = s - 32.  The entry point computes them on the host.
namespace {

constexpr int WSUM_MAX = 4096;          // sum of a launch's weights at most

struct MixWeights {
    uint32_t w[SMAX];                   // weight of sample j
    uint32_t W[SMAX + 1];               // W_k: the sum of the first k weights
    uint32_t mul[SMAX + 1];             // magic_w(W_k)
    uint32_t sh[SMAX + 1];
};

// (2 s + W) / (2 W), exact for s <= W * 65535, W <= 4096
__device__ __forceinline__ uint32_t mix_div_w(uint32_t s, uint32_t W, uint32_t mul, uint32_t sh) { return __umulhi(2u * s + W, mul) >> sh; }

template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void payload_mix_w_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n, int smax,
                                                          int64_t P, uint8_t* __restrict__ dst, int64_t dst_stride, const MixWeights wt)
{
    constexpr int N = Samples<T>::N;
    const int64_t full = P / N;
    const int64_t units = VEC ? full + (P - full * N) : P;
    for (int r = blockIdx.y; r < n; r += gridDim.y) {
        const int64_t* ro = offs + (int64_t)r * smax;
        int k = 0;
        while (k < smax && ro[k] >= 0) ++k;
        if (k == 0) continue;
        const uint32_t W = wt.W[k], mul = wt.mul[k], sh = wt.sh[k];
        uint8_t* out = dst + (int64_t)r * dst_stride;
        for (int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x; c < units; c += (int64_t)gridDim.x * NT) {
            if (VEC && c < full) {
                uint32_t acc[N];
#pragma unroll
                for (int i = 0; i < N; ++i) acc[i] = 0;
                int j = 0;
                for (; j + 4 <= k; j += 4) {                             // four loads in flight
                    u4_t v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = *gcp<u4_t>(base + ro[j + u] + c * 16);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t w = wt.w[j + u];
#pragma unroll
                        for (int i = 0; i < N; ++i) acc[i] += w * Samples<T>::at(v[u], i);
                    }
                }
                for (; j < k; ++j) {
                    const u4_t v = *gcp<u4_t>(base + ro[j] + c * 16);
                    const uint32_t w = wt.w[j];
#pragma unroll
                    for (int i = 0; i < N; ++i) acc[i] += w * Samples<T>::at(v, i);
                }
                u4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < N; ++i) Samples<T>::put(o, i, mix_div_w(acc[i], W, mul, sh));
                __builtin_nontemporal_store(o, gp<u4_t>(out + c * 16));
            } else {
                const int64_t s = VEC ? full * N + (c - full) : c;
                uint32_t acc = 0;
                for (int j = 0; j < k; ++j) acc += wt.w[j] * gcp<T>(base + ro[j])[s];
                gp<T>(out)[s] = (T)mix_div_w(acc, W, mul, sh);
            }
        }
    }
}

}  // namespace

extern "C" int demfi_payload_mix_w(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, int smax, int64_t P,
                                   int sample_bytes, uint8_t* dst, int64_t dst_stride, const int32_t* weights, void* stream)
{
    const char* fn = "demfi_payload_mix_w";
    if (n <= 0) return DEMFI_OK;
    if (!base || !offsets || !offsets_dev || !dst || !weights) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (smax < 1 || smax > SMAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: smax=%d outside 1..%d", fn, smax, SMAX);
    if (sample_bytes != 1 && sample_bytes != 2)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d bytes per sample (1 or 2)", fn, sample_bytes);
    if (P < 1 || P > ((int64_t)1 << 40)) return demfi_set_error(DEMFI_ERR_ARG, "%s: P=%lld samples", fn, (long long)P);
    if (dst_stride < P * sample_bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride=%lld below the %lld bytes of a payload", fn, (long long)dst_stride,
                               (long long)(P * sample_bytes));
    MixWeights wt = {};
    for (int k = 1; k <= smax; ++k) {
        const int32_t w = weights[k - 1];
        if (w < 1 || w > WSUM_MAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: weight %d is %d (1..%d)", fn, k - 1, (int)w, WSUM_MAX);
        const uint64_t W = (uint64_t)wt.W[k - 1] + (uint32_t)w;
        if (W > WSUM_MAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: the weights sum to more than %d", fn, WSUM_MAX);
        const uint64_t top = (2 * W * 65535 + W) * 2 * W;                // n_max * 2 W < 2^43
        int s = 0;
        while ((top >> s) != 0) ++s;                                     // bit_length
        const uint64_t M = ((uint64_t)1 << s) / (2 * W) + 1;
        wt.w[k - 1] = (uint32_t)w;
        wt.W[k] = (uint32_t)W;
        wt.mul[k] = (uint32_t)(s < 32 ? M << (32 - s) : M);
        wt.sh[k] = (uint32_t)(s < 32 ? 0 : s - 32);
    }
    uintptr_t low = (uintptr_t)dst | (uintptr_t)dst_stride;              // the low bits of every address the kernel forms
    for (int r = 0; r < n; ++r) {
        const int64_t* ro = offsets + (int64_t)r * smax;
        if (ro[0] < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: row %d keeps no source (its first offset is %lld)", fn, r, (long long)ro[0]);
        bool ended = false;
        for (int j = 0; j < smax; ++j) {
            if (ro[j] < -1) return demfi_set_error(DEMFI_ERR_ARG, "%s: row %d offset %d is %lld", fn, r, j, (long long)ro[j]);
            if (ro[j] < 0) ended = true;
            else if (ended) return demfi_set_error(DEMFI_ERR_ARG, "%s: row %d has a kept offset behind a -1", fn, r);
            else low |= (uintptr_t)(base + ro[j]);
        }
    }
    if (sample_bytes == 2 && (low & 1)) return demfi_set_error(DEMFI_ERR_ARG, "%s: 16-bit samples at an odd address or stride", fn);
    const bool vec = (low & 15) == 0;
    const int per = 16 / sample_bytes;
    const int64_t units = vec ? P / per + P % per : P;
    const int64_t chunks = (units + NT - 1) / NT;
    const dim3 grid((unsigned)min(chunks, (int64_t)4096), (unsigned)min(n, 4096));
    const hipStream_t st = (hipStream_t)stream;
#define MIX_W_LAUNCH(T, V) \
    hipLaunchKernelGGL((payload_mix_w_kernel<T, V>), grid, dim3(NT), 0, st, base, offsets_dev, n, smax, P, dst, dst_stride, wt)
    if (sample_bytes == 1) { if (vec) MIX_W_LAUNCH(uint8_t, true); else MIX_W_LAUNCH(uint8_t, false); }
    else                   { if (vec) MIX_W_LAUNCH(uint16_t, true); else MIX_W_LAUNCH(uint16_t, false); }
#undef MIX_W_LAUNCH
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
