// Inverse telecine of the Y4M video path (demfi_amd/telecine.py, --ivtc): comb scores of virtual woven frames and the SAD between
// two of them.  The definitions are telecine.comb_counts_np and telecine.woven_sad_np; these kernels give the same integers.
//
// A woven frame W(top, bot) is never built: its even rows are read from the luma plane (the first h*w samples) of payload `top`
// and its odd rows from that of payload `bot`.  A sample of row y, 2 <= y <= h-3, is combed when, with d1 = W[y] - W[y-1] and
// d2 = W[y] - W[y+1], (d1 > T and d2 > T) or (d1 < -T and d2 < -T), and |W[y-2] + 4 W[y] + W[y+2] - 3 (W[y-1] + W[y+1])| > 6 T.
// The plane is cut into 16x16 blocks from the top-left corner; the score is (most combed samples in a block, combed samples).
//
// luma_comb_counts scores the three candidates c, p, n of an entry in one pass: they share their even rows.  One lane owns half
// a block, 8 columns by 16 rows, and walks down it two rows at a time with the rows y-2 .. y+3 of its strip in registers: three
// even rows of the top payload, and three odd rows of each present candidate, as packed words (8 bytes, or 16 bytes of 16-bit
// samples).  Every row of every source is loaded once per strip (plus the two-row halo), consecutive lanes own consecutive strips
// of a block row, so a wave reads contiguous runs of 512 bytes (1 KiB); a row starts at any alignment and the loads are unaligned
// ones, as in dedup.hip.  A strip cut by the right edge goes sample by sample.  The two lanes of a block add their counts, then
// the wave reduces: one atomicMax and one atomicAdd per wave and candidate (integer results are exact in any order).
#include "payload_kit.h"

namespace {

constexpr int NT = 64;                  // comb: a workgroup is one wave
constexpr int BS = 16;                  // block side
constexpr int SW = 8;                   // strip width: half a block
constexpr int SAD_NT = 256;
constexpr int SAD_WGS = 128;
constexpr int MAX_THRESH = 1 << 20;     // 6 T and every sum of five samples stay far inside 32 bits

__device__ __forceinline__ bool is_combed(int c, int up, int dn, int up2, int dn2, int t)
{
    const int d1 = c - up, d2 = c - dn;
    const bool spike = (d1 > t && d2 > t) || (d1 < -t && d2 < -t);
    return spike && abs(up2 + 4 * c + dn2 - 3 * (up + dn)) > 6 * t;
}

// combed samples among the 8 of a row: centre c, the rows next to it, the rows two away
template <typename T>
__device__ __forceinline__ int row_combed(const typename Strip<T>::V& c, const typename Strip<T>::V& up,
                                          const typename Strip<T>::V& dn, const typename Strip<T>::V& up2,
                                          const typename Strip<T>::V& dn2, int t)
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < SW; ++i)
        k += is_combed(Strip<T>::at(c, i), Strip<T>::at(up, i), Strip<T>::at(dn, i), Strip<T>::at(up2, i), Strip<T>::at(dn2, i), t);
    return k;
}

// row r of a plane's strip, or nothing for a row outside the plane (such a row is never used)
template <typename T> __device__ __forceinline__ typename Strip<T>::V strip_row(const T* plane, int r, int h, int w, int x0)
{
    typename Strip<T>::V z = {};
    return r >= 0 && r < h ? Strip<T>::load(plane + (int64_t)r * w + x0) : z;
}

// grid: x = waves over the strips of a plane (two per block, the second possibly empty), y = entries (strided)
template <typename T>
__global__ __launch_bounds__(NT) void luma_comb_counts_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ top_offs,
                                                             const int64_t* __restrict__ bot_offs, int n, int h, int w, int t,
                                                             uint32_t* __restrict__ out)
{
    typedef typename Strip<T>::V W;
    const int nbx = (w + BS - 1) / BS, nby = (h + BS - 1) / BS, nsx = 2 * nbx;
    const int si = blockIdx.x * NT + threadIdx.x;
    const bool live = si < nsx * nby;
    const int sy = live ? si / nsx : 0, sx = live ? si - sy * nsx : 0;
    const int x0 = sx * SW, y0 = sy * BS;
    const int sw = live ? max(min(SW, w - x0), 0) : 0;      // columns of this strip inside the plane
    // rows that can be combed in this strip: ya (even: y0 is) .. yb - 1
    const int ya = max(y0, 2), yb = min(y0 + BS, h - 2);
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* top = (const T*)(base + top_offs[f]);
        const T* bot[3];
        bool has[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t o = bot_offs[3 * f + k];
            has[k] = o >= 0;
            bot[k] = (const T*)(base + (has[k] ? o : 0));
        }
        int cnt[3] = {0, 0, 0};
        if (sw == SW && ya < yb) {
            // even rows y-2, y, y+2 of the top payload; odd rows y-1, y+1, y+3 of each candidate
            W t0 = strip_row(top, ya - 2, h, w, x0), t1 = strip_row(top, ya, h, w, x0), t2 = strip_row(top, ya + 2, h, w, x0);
            W b0[3], b1[3], b2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                b0[k] = b1[k] = b2[k] = t0;
                if (has[k]) {
                    b0[k] = strip_row(bot[k], ya - 1, h, w, x0);
                    b1[k] = strip_row(bot[k], ya + 1, h, w, x0);
                    b2[k] = strip_row(bot[k], ya + 3, h, w, x0);
                }
            }
            for (int y = ya; y < yb; y += 2) {
                const bool odd_in = y + 1 < yb;              // row y + 1 has rows y - 1 .. y + 3 inside the plane
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (has[k]) {
                        cnt[k] += row_combed<T>(t1, b0[k], b1[k], t0, t2, t);
                        if (odd_in) cnt[k] += row_combed<T>(b1[k], t1, t2, b0[k], b2[k], t);
                    }
                t0 = t1;
                t1 = t2;
                t2 = strip_row(top, y + 4, h, w, x0);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (has[k]) {
                        b0[k] = b1[k];
                        b1[k] = b2[k];
                        b2[k] = strip_row(bot[k], y + 5, h, w, x0);
                    }
            }
        } else if (sw > 0) {
            for (int y = ya; y < yb; ++y)
                for (int x = x0; x < x0 + sw; ++x)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (has[k]) {
                            const T* cur = (y & 1) ? bot[k] : top;      // rows y, y-2, y+2
                            const T* oth = (y & 1) ? top : bot[k];      // rows y-1, y+1
                            const int64_t at = (int64_t)y * w + x;
                            cnt[k] += is_combed((int)gcp<T>(cur)[at], (int)gcp<T>(oth)[at - w], (int)gcp<T>(oth)[at + w],
                                                (int)gcp<T>(cur)[at - 2 * w], (int)gcp<T>(cur)[at + 2 * w], t);
                        }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int blk = cnt[k] + __shfl_xor(cnt[k], 1), tot = cnt[k];      // lanes 2j and 2j+1 own the halves of one block
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                blk = max(blk, __shfl_xor(blk, s));
                tot += __shfl_xor(tot, s);
            }
            if (threadIdx.x == 0 && tot) {
                atomicMax(out + 6 * f + 2 * k, (uint32_t)blk);
                atomicAdd(out + 6 * f + 2 * k + 1, (uint32_t)tot);
            }
        }
    }
}

// grid: x = at most SAD_WGS workgroups over the 8-sample pieces of the plane's rows (strided), y = entries (strided).  The waves of
// a workgroup add up in LDS first: every atomic of an entry lands on the same word, and those serialise.
template <typename T>
__global__ __launch_bounds__(SAD_NT) void luma_woven_sad_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n,
                                                               int h, int w, unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long part[SAD_NT / 64];
    const int npx = (w + SW - 1) / SW;
    const int pieces = h * npx;                            // at most 16384 * 2048
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* a[2] = {(const T*)(base + offs[4 * f]), (const T*)(base + offs[4 * f + 1])};           // even rows, odd rows
        const T* b[2] = {(const T*)(base + offs[4 * f + 2]), (const T*)(base + offs[4 * f + 3])};
        uint64_t acc = 0;
        for (int i = blockIdx.x * SAD_NT + threadIdx.x; i < pieces; i += gridDim.x * SAD_NT) {
            const int y = i / npx, x0 = (i - y * npx) * SW;
            const T* pa = a[y & 1] + (int64_t)y * w + x0;
            const T* pb = b[y & 1] + (int64_t)y * w + x0;
            if (x0 + SW <= w) {
                acc += Strip<T>::sad(Strip<T>::load(pa), Strip<T>::load(pb), 0u);
            } else {
                for (int x = 0; x < w - x0; ++x) {
                    const int p = (int)gcp<T>(pa)[x], q = (int)gcp<T>(pb)[x];
                    acc += (uint32_t)(p > q ? p - q : q - p);
                }
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor((unsigned long long)acc, s);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {                              // one atomic per workgroup: they all land on one word
            unsigned long long sum = 0;
#pragma unroll
            for (int v = 0; v < SAD_NT / 64; ++v) sum += part[v];
            if (sum) atomicAdd(out + f, sum);
        }
        __syncthreads();
    }
}

int check_plane(const char* fn, const void* base, int h, int w, int sample_bytes)
{
    if (int st = check_frame_size(fn, h, w)) return st;
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (int st = check_even(fn, sample_bytes, (uintptr_t)base)) return st;
    return DEMFI_OK;
}

}  // namespace

extern "C" int demfi_luma_comb_counts(const uint8_t* base, const int64_t* top_offsets, const int64_t* bot_offsets, int n, int h, int w,
                                      int sample_bytes, int thresh_s, uint32_t* out, void* stream)
{
    const char* fn = "demfi_luma_comb_counts";
    if (!base || !top_offsets || !bot_offsets || !out || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    const int st = check_plane(fn, base, h, w, sample_bytes);
    if (st < 0) return st;
    if (thresh_s < 0 || thresh_s > MAX_THRESH)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: threshold %d outside 0..2^20", fn, thresh_s);
    if (n == 0) return DEMFI_OK;
    DEMFI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n * 6 * sizeof(uint32_t), (hipStream_t)stream));
    const int strips = 2 * ((w + BS - 1) / BS) * ((h + BS - 1) / BS);
    const dim3 grid((unsigned)((strips + NT - 1) / NT), (unsigned)min(n, 65535));
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(luma_comb_counts_kernel<TAG_TYPE(t)>, grid, dim3(NT), 0, (hipStream_t)stream, base, top_offsets, bot_offsets, n, h, w,
                           thresh_s, out);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_luma_woven_sad(const uint8_t* base, const int64_t* offsets, int n, int h, int w, int sample_bytes, uint64_t* out,
                                    void* stream)
{
    const char* fn = "demfi_luma_woven_sad";
    if (!base || !offsets || !out || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    const int st = check_plane(fn, base, h, w, sample_bytes);
    if (st < 0) return st;
    if (n == 0) return DEMFI_OK;
    DEMFI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n * sizeof(uint64_t), (hipStream_t)stream));
    const int pieces = h * ((w + SW - 1) / SW);
    const dim3 grid((unsigned)min((pieces + SAD_NT - 1) / SAD_NT, SAD_WGS), (unsigned)min(n, 65535));
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(luma_woven_sad_kernel<TAG_TYPE(t)>, grid, dim3(SAD_NT), 0, (hipStream_t)stream, base, offsets, n, h, w,
                           (unsigned long long*)out);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
