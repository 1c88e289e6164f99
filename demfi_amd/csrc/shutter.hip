// Synthesized motion blur of the Y4M video path (demfi_amd/shutter.py, --shutter): written payload r is the rounded weighted average
// of the k_r fine payloads it keeps, per stored sample (bytes, or little-endian 16-bit samples).  Two weightings, one kernel template:
//   box (demfi_payload_mix, shutter.mix_np):                out[p] = (2 * sum x_g[p] + k) / (2 k)
//   weighted (demfi_payload_mix_w, shutter.window_weights): out[p] = (2 * sum_j w_j x_j[p] + W_k) / (2 W_k),  W_k = w_0 + .. + w_(k-1)
// The kernel gives the integers of the numpy definitions.
//
// A pure stream: no LDS, no atomics.  Row r of the launch has smax byte offsets from base, the kept ones first and -1 behind them;
// they and k are the same for every lane of a workgroup, so they stay in scalar registers.  A thread owns 16 output bytes: it loads
// the 16 bytes of each kept source (a wave reads 1 KiB of a source at a stretch), adds them up sample by sample in 32-bit
// integers, divides and writes 16 bytes with one store.  The output is written once and read by the copy engine only: a streaming
// store keeps the L2 for the sources, which the gather has just written.
//
// The vector form needs base + every kept offset, dst and dst_stride on 16-byte boundaries; the entry point decides that from the
// host copy of the offsets, for the launch as a whole.  The last P * es mod 16 bytes of a row go sample by sample.  Otherwise (mono
// frames of odd size have an odd P) a thread owns one sample at a time, consecutive lanes consecutive samples, so a wave still reads
// and writes one contiguous run per source; the arithmetic is the same.
//
// Box: 32 x 65535 < 2^21.  The division by 2 k is a multiplication with magic(k) = 2^32 / (2 k) + 1 and a shift by 32: n = 2 sum + k
// < 2^22 and magic(k) * 2 k - 2^32 <= 2 k <= 64, so the error term n * 64 / 2^32 is below 1 / (2 k) and the quotient is exact
// (tests/test_shutter.py walks every k and every sum).
//
// Weighted: the kept sources are always a prefix of the row's S samples, so one weight vector serves every row of a launch and W_k is
// a prefix sum.  The weights, W_k and the divisor constants of every k come by value in the kernel's arguments: uniform, read with
// scalar loads.  With sum w <= 4096 the numerator 2 * 4096 * 65535 + 4096 stays below 2^30.  The division by 2 W is shutter.magic_w:
// with s = bit_length(n_max * 2 W), n_max = 2 W 65535 + W, and M = 2^s / (2 W) + 1, M * 2 W exceeds 2^s by at most 2 W, so n M / 2^s is
// off by less than n_max * 2 W / (2 W * 2^s) < 1 / (2 W) quotient steps: exact.  Folded to one multiply-high: (n * mul) >> 32 >> sh with
// mul = M << (32 - s), sh = 0 for s < 32, else mul = M (< 2^30), sh = s - 32.  The entry point computes them on the host.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup: 4 KiB of a row
constexpr int SMAX = 32;                // kept sources of a row at most
constexpr int WSUM_MAX = 4096;          // sum of a launch's weights at most

struct Magic { uint32_t m[SMAX + 1]; };
constexpr Magic make_magic()
{
    Magic t = {};
    for (int k = 1; k <= SMAX; ++k) t.m[k] = (uint32_t)((1ull << 32) / (2u * k)) + 1u;
    return t;
}
__constant__ Magic kMagic = make_magic();

// A weighting: a kernel argument.  weight(j) of kept source j; divisor(k) of a row that keeps k; mean(s, d) = (2 s + D) / (2 D).
struct BoxMix {                         // exact for s <= k * 65535, k <= 32
    struct Div { uint32_t k, magic; };
    __device__ __forceinline__ uint32_t weight(int) const { return 1u; }
    __device__ __forceinline__ Div divisor(int k) const { return Div{(uint32_t)k, kMagic.m[k]}; }
    static __device__ __forceinline__ uint32_t mean(uint32_t s, const Div& d) { return __umulhi(2u * s + d.k, d.magic); }
    int fill(const char*, const int32_t*, int) { return DEMFI_OK; }
};
struct WeightedMix {                    // exact for s <= W * 65535, W <= 4096
    uint32_t w[SMAX];                   // weight of sample j
    uint32_t W[SMAX + 1];               // W_k: the sum of the first k weights
    uint32_t mul[SMAX + 1];             // magic_w(W_k)
    uint32_t sh[SMAX + 1];
    struct Div { uint32_t W, mul, sh; };
    __device__ __forceinline__ uint32_t weight(int j) const { return w[j]; }
    __device__ __forceinline__ Div divisor(int k) const { return Div{W[k], mul[k], sh[k]}; }
    static __device__ __forceinline__ uint32_t mean(uint32_t s, const Div& d) { return __umulhi(2u * s + d.W, d.mul) >> d.sh; }
    int fill(const char* fn, const int32_t* weights, int smax)
    {
        if (!weights) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
        for (int k = 1; k <= smax; ++k) {
            const int32_t wk = weights[k - 1];
            if (wk < 1 || wk > WSUM_MAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: weight %d is %d (1..%d)", fn, k - 1, (int)wk, WSUM_MAX);
            const uint64_t Wk = (uint64_t)W[k - 1] + (uint32_t)wk;
            if (Wk > WSUM_MAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: the weights sum to more than %d", fn, WSUM_MAX);
            const uint64_t top = (2 * Wk * 65535 + Wk) * 2 * Wk;             // n_max * 2 W < 2^43
            int s = 0;
            while ((top >> s) != 0) ++s;                                     // bit_length
            const uint64_t M = ((uint64_t)1 << s) / (2 * Wk) + 1;
            w[k - 1] = (uint32_t)wk;
            W[k] = (uint32_t)Wk;
            mul[k] = (uint32_t)(s < 32 ? M << (32 - s) : M);
            sh[k] = (uint32_t)(s < 32 ? 0 : s - 32);
        }
        return DEMFI_OK;
    }
};

// grid: x = chunks of NT units of a row (strided), y = rows (strided).  A unit is a 16-byte word (VEC) or one sample.  T: the sample type;
// P counts samples, offsets count bytes.
template <typename T, bool VEC, typename MIX>
__global__ __launch_bounds__(NT) void payload_mix_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n, int smax,
                                                        int64_t P, uint8_t* __restrict__ dst, int64_t dst_stride, const MIX mix)
{
    constexpr int N = Samples<T>::N;
    const int64_t full = P / N;                                          // whole 16-byte words of a row
    const int64_t units = VEC ? full + (P - full * N) : P;               // VEC: the words, then the samples of the tail one by one
    for (int r = blockIdx.y; r < n; r += gridDim.y) {
        const int64_t* ro = offs + (int64_t)r * smax;
        int k = 0;
        while (k < smax && ro[k] >= 0) ++k;                              // kept ones first
        if (k == 0) continue;                                            // refused by the entry point; nothing to average
        const typename MIX::Div div = mix.divisor(k);
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
                        const uint32_t w = mix.weight(j + u);
#pragma unroll
                        for (int i = 0; i < N; ++i) acc[i] += w * Samples<T>::at(v[u], i);
                    }
                }
                for (; j < k; ++j) {
                    const u4_t v = *gcp<u4_t>(base + ro[j] + c * 16);
                    const uint32_t w = mix.weight(j);
#pragma unroll
                    for (int i = 0; i < N; ++i) acc[i] += w * Samples<T>::at(v, i);
                }
                u4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < N; ++i) Samples<T>::put(o, i, MIX::mean(acc[i], div));
                __builtin_nontemporal_store(o, gp<u4_t>(out + c * 16));
            } else {                                                     // one sample: consecutive lanes, consecutive samples
                const int64_t s = VEC ? full * N + (c - full) : c;
                uint32_t acc = 0;
                for (int j = 0; j < k; ++j) acc += mix.weight(j) * gcp<T>(base + ro[j])[s];
                gp<T>(out)[s] = (T)MIX::mean(acc, div);
            }
        }
    }
}

// both entry points
template <typename MIX>
int payload_mix(const char* fn, const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, int smax, int64_t P,
                int sample_bytes, uint8_t* dst, int64_t dst_stride, const int32_t* weights, void* stream)
{
    if (n <= 0) return DEMFI_OK;
    if (!base || !offsets || !offsets_dev || !dst) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (smax < 1 || smax > SMAX) return demfi_set_error(DEMFI_ERR_ARG, "%s: smax=%d outside 1..%d", fn, smax, SMAX);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (P < 1 || P > ((int64_t)1 << 40)) return demfi_set_error(DEMFI_ERR_ARG, "%s: P=%lld samples", fn, (long long)P);
    if (int st = check_dst_stride(fn, dst_stride, P * sample_bytes)) return st;
    MIX mix = {};
    if (int st = mix.fill(fn, weights, smax)) return st;
    uintptr_t low = (uintptr_t)dst | (uintptr_t)dst_stride;              // the low bits of every address the kernel forms
    if (int st = walk_offsets(fn, offsets, n, smax, smax, OFFS_PREFIX, 0, NO_LIMIT, (uintptr_t)base, &low)) return st;
    if (int st = check_even(fn, sample_bytes, low)) return st;
    const bool vec = (low & 15) == 0;
    const dim3 grid = rows_grid(stream_units(P, sample_bytes, vec), NT, n);
    by_sample(sample_bytes, [&](auto t) {
        by_bool(vec, [&](auto v) {
            hipLaunchKernelGGL((payload_mix_kernel<TAG_TYPE(t), TAG_VALUE(v), MIX>), grid, dim3(NT), 0, (hipStream_t)stream, base, offsets_dev,
                               n, smax, P, dst, dst_stride, mix);
        });
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

}  // namespace

extern "C" int demfi_payload_mix(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, int smax, int64_t P,
                                 int sample_bytes, uint8_t* dst, int64_t dst_stride, void* stream)
{
    return payload_mix<BoxMix>("demfi_payload_mix", base, offsets, offsets_dev, n, smax, P, sample_bytes, dst, dst_stride, nullptr, stream);
}

extern "C" int demfi_payload_mix_w(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, int smax, int64_t P,
                                   int sample_bytes, uint8_t* dst, int64_t dst_stride, const int32_t* weights, void* stream)
{
    return payload_mix<WeightedMix>("demfi_payload_mix_w", base, offsets, offsets_dev, n, smax, P, sample_bytes, dst, dst_stride, weights,
                                    stream);
}
