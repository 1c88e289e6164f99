// Letterbox and pillarbox bars of the Y4M video path (demfi_amd/letterbox.py, --crop auto): for every row and every column of a
// luma plane, how many samples are strictly greater than a threshold.  The definition is letterbox.line_counts_np; this kernel
// gives the same integers.
//
// The luma plane is the first h*w samples of a payload (bytes, or 16-bit samples above 8 bits).  It is cut into tiles of
// TW = 512 columns by TH = 128 rows from the top-left corner.  A workgroup of four waves owns one tile; wave v walks down the
// RS = 32 rows y0 + 32 v .. of it, lane l owning the 8 columns x0 + 8 l .. x0 + 8 l + 7: per row a lane loads its 8 samples as one
// packed word (8 bytes, or 16 bytes of 16-bit samples), so a wave reads one contiguous run of 512 bytes (1 KiB) and every sample
// of the plane is loaded exactly once.  A row starts at any alignment and the loads are unaligned ones, as in dedup.hip; a lane
// whose 8 columns are cut by the right edge goes sample by sample.  The lane keeps the counters of its 8 columns in registers
// for the whole walk and leaves its count of each row (0..8) as one byte in LDS.  Behind a barrier thread t adds up the 64
// bytes of row t of the tile and sends them off with ONE atomicAdd per (row, tile column), the four waves add their column
// counters in LDS and thread t sends columns t and t + 256 off with ONE atomicAdd per (column, tile row): consecutive lanes,
// consecutive words.  Zero sums (bars) send nothing.  Integer adds are exact in any order.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // four waves
constexpr int SW = 8;                   // columns of a lane
constexpr int TW = 64 * SW;             // tile width
constexpr int RS = 32;                  // rows of a wave
constexpr int TH = (NT / 64) * RS;      // tile height
constexpr int RB = 64 + 4;              // bytes of a row's lane counts in LDS: 17 words, so the row sums read without bank conflicts

// grid: x = the tiles of a plane, y = planes (strided).  T: the sample type; offsets count bytes.
template <typename T>
__global__ __launch_bounds__(NT) void luma_line_counts_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n,
                                                             int h, int w, uint32_t thresh, uint32_t* __restrict__ rows,
                                                             uint32_t* __restrict__ cols)
{
    __shared__ __attribute__((aligned(4))) uint8_t row_part[TH * RB];     // [tile row][lane]: the lane's count of that row
    __shared__ uint32_t col_sum[TW];
    const int ntx = (w + TW - 1) / TW;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = tx * TW + lane * SW;                                  // this lane's first column
    const int r0 = wave * RS, y0 = ty * TH + r0;                         // this wave's first row, in the tile and in the plane
    const int nr = max(min(RS, h - y0), 0);                              // its rows inside the plane
    const int sw = max(min(SW, w - x0), 0);                              // this lane's columns inside the plane
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T* p = (const T*)(base + offs[f]) + (int64_t)y0 * w + x0;
        uint32_t cnt[SW] = {0, 0, 0, 0, 0, 0, 0, 0};
        col_sum[threadIdx.x] = 0;
        col_sum[threadIdx.x + NT] = 0;
        if (sw == SW) {
#pragma unroll 4
            for (int r = 0; r < nr; ++r) {
                const typename Strip<T>::V v = Strip<T>::load(p + (int64_t)r * w);
                uint32_t k = 0;
#pragma unroll
                for (int i = 0; i < SW; ++i) {
                    const uint32_t b = Strip<T>::at(v, i) > thresh;
                    cnt[i] += b;
                    k += b;
                }
                row_part[(r0 + r) * RB + lane] = (uint8_t)k;
            }
        } else {
            for (int r = 0; r < nr; ++r) {
                uint32_t k = 0;
#pragma unroll
                for (int i = 0; i < SW; ++i)
                    if (i < sw) {
                        const uint32_t b = (uint32_t)gcp<T>(p + (int64_t)r * w)[i] > thresh;
                        cnt[i] += b;
                        k += b;
                    }
                row_part[(r0 + r) * RB + lane] = (uint8_t)k;
            }
        }
        __syncthreads();                                                 // row_part written, col_sum zeroed
#pragma unroll
        for (int i = 0; i < SW; ++i)
            if (cnt[i]) atomicAdd(&col_sum[lane * SW + i], cnt[i]);      // LDS: the four waves of a tile column
        if (threadIdx.x < TH && ty * TH + (int)threadIdx.x < h) {        // row t of the tile: its 64 lane counts, four to a word
            const uint32_t* q = (const uint32_t*)(row_part + threadIdx.x * RB);
            uint32_t s = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) s = __builtin_amdgcn_sad_u8(q[j], 0u, s);
            if (s) atomicAdd(rows + (int64_t)f * h + ty * TH + threadIdx.x, s);
        }
        __syncthreads();                                                 // col_sum complete
#pragma unroll
        for (int j = 0; j < TW / NT; ++j) {
            const int c = threadIdx.x + j * NT, x = tx * TW + c;
            const uint32_t s = col_sum[c];
            if (x < w && s) atomicAdd(cols + (int64_t)f * w + x, s);
        }
        __syncthreads();                                                 // before the next plane reuses the LDS
    }
}

}  // namespace

extern "C" int demfi_luma_line_counts(const uint8_t* base, const int64_t* offsets, int n, int h, int w, int sample_bytes, int64_t thresh,
                                      uint32_t* rows, uint32_t* cols, void* stream)
{
    const char* fn = "demfi_luma_line_counts";
    if (!base || !offsets || !rows || !cols || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (thresh < 0 || thresh > 65535)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: threshold %lld outside 0..65535", fn, (long long)thresh);
    if (int st = check_even(fn, sample_bytes, (uintptr_t)base)) return st;
    if (n == 0) return DEMFI_OK;
    DEMFI_HIP_CHECK(hipMemsetAsync(rows, 0, (size_t)n * h * sizeof(uint32_t), (hipStream_t)stream));
    DEMFI_HIP_CHECK(hipMemsetAsync(cols, 0, (size_t)n * w * sizeof(uint32_t), (hipStream_t)stream));
    const int tiles = ((w + TW - 1) / TW) * ((h + TH - 1) / TH);         // at most 32 * 128
    const dim3 grid((unsigned)tiles, (unsigned)min(n, 65535));
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(luma_line_counts_kernel<TAG_TYPE(t)>, grid, dim3(NT), 0, (hipStream_t)stream, base, offsets, n, h, w, (uint32_t)thresh,
                           rows, cols);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
