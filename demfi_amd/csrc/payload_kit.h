// What the payload stages of the Y4M edge share (shutter, denoise, deblock, dering, nlmeans, deband, interlace, bitdepth, grain, scale, crop, ivtc, dedup, tile and,
// through yuv_common.h, the colour conversions): packed-word typedefs and sample accessors on the device side; on the host side the
// argument checks every demfi_payload_* entry point makes before its first HIP call, the launch grids and the dispatch from run-time
// values to template arguments.  The rules differ from entry point to entry point (plane sizes, what an offset row may hold, which
// addresses decide the wide path): those are parameters here, and every message carries the entry point's name.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

// ---- packed words: <vector>_a<N> is the vector at an address that is only N-byte aligned (global memory serves such loads) ----
typedef unsigned int u2_t __attribute__((ext_vector_type(2)));
typedef u2_t u2_a1 __attribute__((aligned(1)));
typedef u4_t u4_a1 __attribute__((aligned(1)));
typedef u4_t u4_a2 __attribute__((aligned(2)));

template <typename T> struct Acc;       // accumulator of a sample type
template <> struct Acc<uint8_t> { typedef int type; };
template <> struct Acc<uint16_t> { typedef int64_t type; };

// sample i of a vector of dwords; i is a constant of an unrolled loop wherever this is used
template <typename T, typename V> __device__ __forceinline__ uint32_t sample_at(const V& v, int i)
{
    constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    return (v[i / PER] >> (BITS * (i % PER))) & ((1u << BITS) - 1u);
}
template <typename T, typename V> __device__ __forceinline__ void sample_put(V& v, int i, uint32_t x)     // into a zeroed vector
{
    constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    v[i / PER] |= x << (BITS * (i % PER));
}

template <typename T> struct Samples {  // the 16 / sizeof(T) samples of a 16-byte word
    static constexpr int N = 16 / (int)sizeof(T);
    static __device__ __forceinline__ uint32_t at(const u4_t& v, int i) { return sample_at<T>(v, i); }
    static __device__ __forceinline__ void put(u4_t& v, int i, uint32_t x) { sample_put<T>(v, i, x); }
};

template <typename T> struct Strip {    // 8 consecutive samples as one packed word: 8 bytes, or 16 bytes of 16-bit samples
    typedef typename std::conditional<sizeof(T) == 1, u2_t, u4_t>::type V;
    typedef typename std::conditional<sizeof(T) == 1, u2_a1, u4_a2>::type V_sample_aligned;
    static __device__ __forceinline__ V load(const T* p) { return *(const DEMFI_GLOBAL V_sample_aligned*)p; }   // any sample address
    static __device__ __forceinline__ uint32_t at(const V& v, int i) { return sample_at<T>(v, i); }
    static __device__ __forceinline__ void put(V& v, int i, uint32_t x) { sample_put<T>(v, i, x); }
    static __device__ __forceinline__ V zero() { return V(0u); }
    static __device__ __forceinline__ uint32_t sad(const V& a, const V& b, uint32_t acc)                     // acc + sum |a_i - b_i|
    {
#pragma unroll
        for (int d = 0; d < (int)(sizeof(V) / 4); ++d)
            acc = sizeof(T) == 1 ? __builtin_amdgcn_sad_u8(a[d], b[d], acc) : __builtin_amdgcn_sad_u16(a[d], b[d], acc);
        return acc;
    }
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int clamp_row(int y, int rows) { return clampi(y, 0, rows - 1); }

// ---- host: the small checks.  Each returns DEMFI_OK or sets the error and returns its code -------------------------------------
inline bool is_depth(int d) { return d == 8 || d == 10 || d == 12 || d == 14 || d == 16; }

inline int check_sample_bytes(const char* fn, int sample_bytes)
{
    if (sample_bytes != 1 && sample_bytes != 2) return demfi_set_error(DEMFI_ERR_ARG, "%s: %d bytes per sample (1 or 2)", fn, sample_bytes);
    return DEMFI_OK;
}

inline int check_frame_size(const char* fn, int h, int w)
{
    if (h < 2 || w < 2 || h > 16384 || w > 16384) return demfi_set_error(DEMFI_ERR_ARG, "%s: frame size %dx%d outside 2..16384", fn, h, w);
    return DEMFI_OK;
}

inline int check_peak(const char* fn, int peak, int sample_bytes)
{
    const int top = sample_bytes == 1 ? 255 : 65535;
    if (peak < 1 || peak > top) return demfi_set_error(DEMFI_ERR_ARG, "%s: peak=%d outside 1..%d", fn, peak, top);
    return DEMFI_OK;
}

inline int check_flag(const char* fn, const char* name, int v)
{
    if (v != 0 && v != 1) return demfi_set_error(DEMFI_ERR_ARG, "%s: %s=%d (0 or 1)", fn, name, v);
    return DEMFI_OK;
}

inline int check_dst_stride(const char* fn, int64_t dst_stride, int64_t payload_bytes)
{
    if (dst_stride < payload_bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride=%lld below the %lld bytes of a payload", fn, (long long)dst_stride,
                               (long long)payload_bytes);
    return DEMFI_OK;
}

// low: the OR of every address, offset and stride that must be even when samples have 16 bits
inline int check_even(const char* fn, int sample_bytes, uintptr_t low)
{
    if (sample_bytes == 2 && (low & 1)) return demfi_set_error(DEMFI_ERR_ARG, "%s: 16-bit samples at an odd address, offset or stride", fn);
    return DEMFI_OK;
}

// ---- host: the plane list ---------------------------------------------------------------------------------------------------------
constexpr int MAXP = 3;                 // planes of a payload at most

struct PlaneList {                      // a kernel argument of interlace.hip and bitdepth.hip
    int n;
    int rows[MAXP], cols[MAXP];
    int64_t start[MAXP];                // first sample of the plane in the payload
};
struct PlaneSet {
    PlaneList pl;
    int64_t P, most;                    // samples of a payload; of its largest plane
};

// planes: int32 [2 n_planes], rows and columns of each.  The entry point's own limits: 1 .. max_side each way, max_samples a plane,
// and one to three planes or (one_or_three) no two.
inline int parse_planes(const char* fn, const int32_t* planes, int n_planes, int max_side, int64_t max_samples, bool one_or_three, PlaneSet* out)
{
    if (n_planes < 1 || n_planes > MAXP || (one_or_three && n_planes == 2))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d planes (%s%d)", fn, n_planes, one_or_three ? "1 or " : "1..", MAXP);
    *out = PlaneSet{};
    out->pl.n = n_planes;
    for (int p = 0; p < n_planes; ++p) {
        const int rows = planes[2 * p], cols = planes[2 * p + 1];
        if (rows < 1 || cols < 1 || rows > max_side || cols > max_side || (int64_t)rows * cols > max_samples)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d is %d x %d (1..%d each, %lld samples at most)", fn, p, rows, cols, max_side,
                                   (long long)max_samples);
        out->pl.rows[p] = rows, out->pl.cols[p] = cols, out->pl.start[p] = out->P;
        out->most = max(out->most, (int64_t)rows * cols);
        out->P += (int64_t)rows * cols;
    }
    return DEMFI_OK;
}

// ---- host: the offset table -------------------------------------------------------------------------------------------------------
enum OffsetRule {
    OFFS_ALL,                           // every offset present
    OFFS_PREFIX,                        // the first present, then -1 only behind the last present one
    OFFS_BUT_CENTRE,                    // -1 anywhere but in column `centre`
};
constexpr int64_t NO_LIMIT = INT64_MAX;

// Row r of the HOST copy of a table: the `cols` byte offsets at offs[r * stride ..].  Refuses what `rule` forbids, every other negative
// and every offset above `limit`; ORs origin + offset of every present one into *low (the entry point picks the origin: the buffer's
// address, or 0 where it takes the buffer into the OR itself).
inline int walk_offsets(const char* fn, const int64_t* offs, int n, int stride, int cols, OffsetRule rule, int centre, int64_t limit,
                        uintptr_t origin, uintptr_t* low)
{
    for (int r = 0; r < n; ++r) {
        const int64_t* ro = offs + (int64_t)r * stride;
        bool ended = false;
        for (int j = 0; j < cols; ++j) {
            const int64_t o = ro[j];
            if (o == -1 && (rule == OFFS_PREFIX ? j > 0 : rule == OFFS_BUT_CENTRE && j != centre)) {
                ended = true;
                continue;
            }
            if (o < 0 || o > limit || (rule == OFFS_PREFIX && ended))
                return demfi_set_error(DEMFI_ERR_ARG, "%s: row %d offset %d of %d is %lld (%s%s%lld at most)", fn, r, j, cols, (long long)o,
                                       rule == OFFS_PREFIX ? "-1 only behind the last kept one; " : rule == OFFS_BUT_CENTRE ? "-1 = absent, " : "",
                                       rule == OFFS_BUT_CENTRE && j == centre ? "which this one cannot be; " : "", (long long)limit);
            *low |= origin + (uintptr_t)o;
        }
    }
    return DEMFI_OK;
}

// ---- host: grids and dispatch -----------------------------------------------------------------------------------------------------
// what a streaming kernel strides over: 16-byte words and the tail's samples (vec), or samples
inline int64_t stream_units(int64_t P, int sample_bytes, bool vec)
{
    const int per = 16 / sample_bytes;
    return vec ? P / per + P % per : P;
}
// x = chunks of nt items (strided), y = rows (strided)
inline dim3 rows_grid(int64_t items, int nt, int64_t rows)
{
    return dim3((unsigned)min((items + nt - 1) / nt, (int64_t)4096), (unsigned)min(rows, (int64_t)4096));
}
// x = chunks of nt items of the largest plane (strided), y = (payload, plane) pairs (strided)
inline dim3 planes_grid(int64_t most_items, int nt, int n, int n_planes) { return rows_grid(most_items, nt, (int64_t)n * n_planes); }

template <typename T> struct type_tag { typedef T type; };
#define TAG_TYPE(t) typename decltype(t)::type
#define TAG_VALUE(t) decltype(t)::value

// f(type_tag<uint8_t>) or f(type_tag<uint16_t>); f(std::bool_constant<b>); f(std::integral_constant<int, v>) for LO <= v <= HI
template <typename F> inline void by_sample(int sample_bytes, F&& f)
{
    if (sample_bytes == 1) f(type_tag<uint8_t>{}); else f(type_tag<uint16_t>{});
}
template <typename F> inline void by_bool(bool b, F&& f)
{
    if (b) f(std::true_type{}); else f(std::false_type{});
}
template <int LO, int HI, typename F> inline void by_int(int v, F&& f)
{
    if constexpr (LO < HI) {
        if (v == LO) f(std::integral_constant<int, LO>{}); else by_int<LO + 1, HI>(v, f);
    } else {
        f(std::integral_constant<int, HI>{});
    }
}

}  // namespace
