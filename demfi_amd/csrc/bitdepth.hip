// Bit depth of the Y4M video path (demfi_amd/bitdepth.py, --work-depth / --out-depth): payload r of the launch is the source payload at
// base + offsets[r] with every sample taken from d_in to d_out bits,
//   out = clip(off_out + floor(((v - off_in) * num + T) / den), 0, peak_out)
// limited range: off = 0 and a pure shift, v << k going up, (v + T) >> k going down; full range: (num, den) = (peak_out, peak_in), off = 0
// for luma and 2^(d - 1) for chroma.  T = den / 2, or going down under the ordered dither ((2 B + 1) * den) >> 7 with B the 8x8 index of
// the sample's (x, y) within its plane (y = row >> 1 when the payload holds fields).  The definition is bitdepth.convert_payload_np; these
// kernels give the same integers.  demfi_payload_promote goes up, demfi_payload_requant goes down; both are this one kernel.
//
// A pure stream: no LDS, no atomics.  blockIdx.y strides over the (payload, plane) pairs, blockIdx.x over chunks of NT items of the plane.
//
// The wide path: an item is 8 consecutive samples of a row, 16 bytes of the wider side (one side always has 16-bit samples) and 8 of a
// byte side; items run along the row first, so a wave reads and writes one contiguous run.  One 128-bit (64-bit) load, one streaming
// store (the promoted payload is read next by another launch, but it is far larger than this one's reads are worth keeping; the
// requantised one is read by the copy engine only).  An item starts at a column that is a multiple of 8, so sample i of it has x mod 8 = i and B
// is (F(i) ^ F(y)) | G(y) with F(i) a constant of the unrolled loop: the interleave is linear over xor.  B is computed, never loaded.
//
// The wide path needs every row start on an item boundary on both sides: base + every offset and every plane's first byte and row
// length on 8 source samples, dst and dst_stride on 8 output samples.  The entry point decides that PER LAUNCH from the host copy of the
// offsets and the plane list: 720p and 1080p 4:2:0 meet it on all three planes.  Otherwise (odd sizes, shifted bases) the whole launch
// goes sample by sample: an item is one sample, consecutive lanes take consecutive samples; the arithmetic is the same.
//
// Full range divides by den = peak_in, a constant of the launch: floor(n / den) = (t + ((n - t) >> 1)) >> s with t = umulhi(m, n), the
// round-up reciprocal of Granlund and Montgomery, exact for EVERY 32-bit n (bitdepth.reciprocal; tests/test_bitdepth.py holds it to the
// floor).  (v - off_in) * num + T is negative for chroma below neutral and reaches 65535 * 65535 + 65534 for stored samples above their
// peak, so a signed value or a bias would need 64 bits (bitdepth.accumulator_bounds); the kernel divides magnitudes instead: for a =
// v - off_in >= 0 the quotient of a num + T, for a < 0 minus the quotient of |a| num + (den - 1 - T), both below 2^32.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
enum { M_UP = 0, M_DOWN = 1, M_FULL = 2 };

struct Rule {                           // uniform over the launch; off[0] luma, off[1] chroma
    int off_in[2], off_out[2];
    uint32_t num, den, magic;
    int shift;                          // limited range: |d_out - d_in|; full range: s of the reciprocal
    int peak, bayer, field_rows;
};

// bits 0, 1, 2 of a -> bits 5, 3, 1; G = F >> 1.  B(x, y) = F((x ^ y) & 7) | G(y & 7)
__host__ __device__ constexpr uint32_t bayer_f(uint32_t a) { return ((a & 1u) << 5) | ((a & 2u) << 2) | ((a & 4u) >> 1); }

__device__ __forceinline__ uint32_t div_den(uint32_t n, const Rule& r)
{
    const uint32_t t = __umulhi(r.magic, n);
    return (t + ((n - t) >> 1)) >> r.shift;
}

// the threshold of a sample whose dither index is B (ignored unless the launch dithers)
template <int MODE> __device__ __forceinline__ uint32_t threshold(uint32_t B, const Rule& r)
{
    if (MODE == M_UP) return 0u;                                             // den = 1
    if (MODE == M_DOWN) return r.bayer ? ((2u * B + 1u) << r.shift) >> 7 : 1u << (r.shift - 1);
    return r.bayer ? ((2u * B + 1u) * r.den) >> 7 : r.den >> 1;
}

template <int MODE> __device__ __forceinline__ uint32_t convert(uint32_t v, uint32_t T, int chroma, const Rule& r)
{
    if (MODE == M_UP) return min(v << r.shift, (uint32_t)r.peak);            // v < 2^16, shift <= 8
    if (MODE == M_DOWN) return min((v + T) >> r.shift, (uint32_t)r.peak);
    const int a = (int)v - r.off_in[chroma];
    const int o = a >= 0 ? r.off_out[chroma] + (int)div_den((uint32_t)a * r.num + T, r)
                         : r.off_out[chroma] - (int)div_den((uint32_t)(-a) * r.num + (r.den - 1u - T), r);
    return (uint32_t)min(max(o, 0), r.peak);
}

// grid: x = chunks of NT items of a plane (strided), y = (payload, plane) pairs (strided).  WIDE: item = row * words + word of 8 samples;
// else item = row * cols + column.
template <typename TI, typename TO, int MODE, bool WIDE>
__global__ __launch_bounds__(NT) void payload_depth_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n, PlaneList pl,
                                                          Rule rule, uint8_t* __restrict__ dst, int64_t dst_stride)
{
    constexpr int ei = (int)sizeof(TI), eo = (int)sizeof(TO);
    for (int rp = blockIdx.y; rp < n * pl.n; rp += gridDim.y) {
        const int r = rp / pl.n, p = rp - r * pl.n;
        const int chroma = p > 0;
        const uint32_t cols = (uint32_t)pl.cols[p], rows = (uint32_t)pl.rows[p];
        const uint8_t* src = base + offs[r] + pl.start[p] * ei;
        uint8_t* out = dst + (int64_t)r * dst_stride + pl.start[p] * eo;
        if (WIDE) {
            const uint32_t words = cols >> 3, items = words * rows;         // <= 2^27
            for (uint32_t it = blockIdx.x * NT + threadIdx.x; it < items; it += gridDim.x * NT) {
                const uint32_t y = it / words, c = it - y * words;
                const int64_t at = (int64_t)y * cols + (int64_t)c * 8;       // the item's first sample in the plane
                const typename Strip<TI>::V v = *gcp<typename Strip<TI>::V>(src + at * ei);   // an item of the wide path is aligned
                const uint32_t yy = (rule.field_rows ? y >> 1 : y) & 7u;
                const uint32_t fy = bayer_f(yy), gy = fy >> 1;
                typename Strip<TO>::V o = Strip<TO>::zero();
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    Strip<TO>::put(o, i, convert<MODE>(Strip<TI>::at(v, i), threshold<MODE>((bayer_f((uint32_t)i) ^ fy) | gy, rule), chroma, rule));
                __builtin_nontemporal_store(o, gp<typename Strip<TO>::V>(out + at * eo));
            }
        } else {
            const uint32_t items = cols * rows;                             // <= 2^30
            const auto s = gcp<TI>(src);
            const auto d = gp<TO>(out);
            for (uint32_t it = blockIdx.x * NT + threadIdx.x; it < items; it += gridDim.x * NT) {
                const uint32_t y = it / cols, x = it - y * cols;
                const uint32_t yy = rule.field_rows ? y >> 1 : y;
                const uint32_t B = bayer_f((x ^ yy) & 7u) | (bayer_f(yy & 7u) >> 1);
                d[it] = (TO)convert<MODE>(s[it], threshold<MODE>(B, rule), chroma, rule);
            }
        }
    }
}

// both entry points: ``up`` says which way the depths must go
int payload_depth(const char* fn, bool up, const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes,
                  int n_planes, int in_bytes, int out_bytes, int depth_in, int depth_out, int full_range, int dither, int field_rows,
                  uint8_t* dst, int64_t dst_stride, void* stream)
{
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (!base || !offsets || !offsets_dev || !planes || !dst) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (!is_depth(depth_in) || !is_depth(depth_out) || (up ? depth_out <= depth_in : depth_out >= depth_in))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d -> %d bits (8, 10, 12, 14 or 16 each, going %s)", fn, depth_in, depth_out, up ? "up" : "down");
    if (in_bytes != (depth_in > 8 ? 2 : 1) || out_bytes != (depth_out > 8 ? 2 : 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d and %d bytes per sample for %d and %d bits (1 at 8 bits, 2 above)", fn, in_bytes, out_bytes,
                               depth_in, depth_out);
    if ((full_range | 1) != 1 || (dither | 1) != 1 || (field_rows | 1) != 1)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: full_range=%d, dither=%d, field_rows=%d (0 or 1 each)", fn, full_range, dither, field_rows);
    PlaneSet ps;
    if (int st = parse_planes(fn, planes, n_planes, 1 << 20, (int64_t)1 << 30, false, &ps)) return st;
    const PlaneList& pl = ps.pl;
    bool by8 = true;                                                         // every plane starts and every row ends on 8 samples
    for (int p = 0; p < n_planes; ++p) by8 = by8 && pl.start[p] % 8 == 0 && pl.cols[p] % 8 == 0;
    if (int st = check_dst_stride(fn, dst_stride, ps.P * out_bytes)) return st;
    uintptr_t lo_in = (uintptr_t)base, lo_out = (uintptr_t)dst | (uintptr_t)dst_stride;   // the low bits of every address the kernel forms
    if (int st = walk_offsets(fn, offsets, n, 1, 1, OFFS_ALL, 0, NO_LIMIT, 0, &lo_in)) return st;
    if (int st = check_even(fn, in_bytes, lo_in)) return st;
    if (int st = check_even(fn, out_bytes, lo_out)) return st;
    if (n == 0) return DEMFI_OK;
    const bool wide = by8 && (lo_in & (uintptr_t)(8 * in_bytes - 1)) == 0 && (lo_out & (uintptr_t)(8 * out_bytes - 1)) == 0;

    Rule rule = {};
    rule.peak = (1 << depth_out) - 1, rule.bayer = !up && dither, rule.field_rows = field_rows;
    int mode;
    if (!full_range) {
        mode = up ? M_UP : M_DOWN;
        rule.shift = up ? depth_out - depth_in : depth_in - depth_out;
        rule.num = up ? 1u << rule.shift : 1u, rule.den = up ? 1u : 1u << rule.shift;
    } else {
        mode = M_FULL;
        rule.off_in[1] = 1 << (depth_in - 1), rule.off_out[1] = 1 << (depth_out - 1);
        rule.num = (1u << depth_out) - 1u, rule.den = (1u << depth_in) - 1u;
        const int l = depth_in;                                              // ceil(log2(2^d - 1)) for d >= 2
        rule.magic = (uint32_t)(((1ull << 32) * ((1ull << l) - rule.den)) / rule.den + 1ull);
        rule.shift = l - 1;
    }
    const dim3 grid = planes_grid(wide ? ps.most / 8 : ps.most, NT, n, n_planes);
    // storage: 0 = bytes -> 16 bits, 1 = 16 bits -> bytes, 2 = 16 -> 16 (a byte source always has a 16-bit destination)
    by_int<0, 2>(in_bytes == 1 ? 0 : out_bytes == 1 ? 1 : 2, [&](auto s) {
        typedef typename std::conditional<TAG_VALUE(s) == 0, uint8_t, uint16_t>::type TI;
        typedef typename std::conditional<TAG_VALUE(s) == 1, uint8_t, uint16_t>::type TO;
        by_int<M_UP, M_FULL>(mode, [&](auto m) {
            by_bool(wide, [&](auto w) {
                hipLaunchKernelGGL((payload_depth_kernel<TI, TO, TAG_VALUE(m), TAG_VALUE(w)>), grid, dim3(NT), 0, (hipStream_t)stream, base,
                                   offsets_dev, n, pl, rule, dst, dst_stride);
            });
        });
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

}  // namespace

extern "C" int demfi_payload_promote(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes,
                                     int n_planes, int in_bytes, int out_bytes, int depth_in, int depth_out, int full_range, uint8_t* dst,
                                     int64_t dst_stride, void* stream)
{
    return payload_depth("demfi_payload_promote", true, base, offsets, offsets_dev, n, planes, n_planes, in_bytes, out_bytes, depth_in,
                         depth_out, full_range, 0, 0, dst, dst_stride, stream);
}

extern "C" int demfi_payload_requant(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes,
                                     int n_planes, int in_bytes, int out_bytes, int depth_in, int depth_out, int full_range, int dither,
                                     int field_rows, uint8_t* dst, int64_t dst_stride, void* stream)
{
    return payload_depth("demfi_payload_requant", false, base, offsets, offsets_dev, n, planes, n_planes, in_bytes, out_bytes, depth_in,
                         depth_out, full_range, dither, field_rows, dst, dst_stride, stream);
}
