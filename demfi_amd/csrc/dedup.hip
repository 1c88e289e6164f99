// Repeated frames of the Y4M video path (demfi_amd/cadence.py, --dedup): per (frame, last kept frame) pair, how many 8x8 luma
// blocks differ a lot (hot) or noticeably (warm).  The definition is cadence.block_counts_np; this kernel gives the same two
// integers.
//
// The luma plane is the first h*w samples of a payload (bytes, or 16-bit samples above 8 bits).  It is cut into 8x8 blocks from
// the top-left corner; the blocks at the right and bottom edges are partial, of area a < 64.  With SAD the sum of absolute
// sample differences over a block, the block is hot when 64*SAD > hi_s*a and warm when 64*SAD > lo_s*a (hi_s, lo_s: the
// thresholds times 2^(depth-8)); integers throughout.
//
// One lane owns one block, consecutive lanes own consecutive blocks of a block row, so for each of the 8 rows a wave reads one
// contiguous run of 512 bytes (1 KiB of 16-bit samples) from each frame.  A row of a plane of arbitrary width starts at any
// alignment: the 8-byte (16-byte) loads are unaligned ones, which global memory serves (tile.hip's copy_piece and
// yuv420_sad_kernel read the same way).  Partial blocks go sample by sample.  A workgroup is ONE wave: the reduction is a ballot
// and a popcount, and lane 0 adds the wave's counts with one atomicAdd per counter (integer adds are exact in any order).
#include "payload_kit.h"

namespace {

constexpr int NT = 64;
constexpr int BS = 8;                   // block side
constexpr int64_t MAX_THRESHOLD = (int64_t)1 << 40;   // hi_s * 64 stays far inside 64 bits

// SAD of 8 consecutive samples at any sample address
template <typename T> __device__ __forceinline__ uint32_t row_sad(const T* a, const T* b, uint32_t acc)
{
    return Strip<T>::sad(Strip<T>::load(a), Strip<T>::load(b), acc);
}

// grid: x = waves over the blocks of a plane, y = pairs (strided).  T: the sample type; offsets count bytes.
template <typename T>
__global__ __launch_bounds__(NT) void luma_block_counts_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ a_offs,
                                                              const int64_t* __restrict__ b_offs, int n, int h, int w, uint64_t hi_s,
                                                              uint64_t lo_s, uint32_t* __restrict__ counts)
{
    const int nbx = (w + BS - 1) / BS, nby = (h + BS - 1) / BS;
    const int bi = blockIdx.x * NT + threadIdx.x;
    const bool live = bi < nbx * nby;
    const int by = live ? bi / nbx : 0, bx = live ? bi - by * nbx : 0;
    const int x0 = bx * BS, y0 = by * BS;
    const int bw = min(BS, w - x0), bh = min(BS, h - y0);
    const int64_t first = (int64_t)y0 * w + x0;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        uint32_t sad = 0;
        if (live) {
            const T* a = (const T*)(base + a_offs[f]) + first;
            const T* b = (const T*)(base + b_offs[f]) + first;
            if (bw == BS && bh == BS) {
#pragma unroll
                for (int y = 0; y < BS; ++y) sad = row_sad(a + (int64_t)y * w, b + (int64_t)y * w, sad);
            } else if (bw == BS) {
                for (int y = 0; y < bh; ++y) sad = row_sad(a + (int64_t)y * w, b + (int64_t)y * w, sad);
            } else {
                for (int y = 0; y < bh; ++y)
                    for (int x = 0; x < bw; ++x) {
                        const int p = (int)gcp<T>(a + (int64_t)y * w)[x], q = (int)gcp<T>(b + (int64_t)y * w)[x];
                        sad += (uint32_t)(p > q ? p - q : q - p);
                    }
            }
        }
        const uint64_t lhs = (uint64_t)64 * sad, area = (uint64_t)(bw * bh);
        const int hot = __popcll(__ballot(live && lhs > hi_s * area));
        const int warm = __popcll(__ballot(live && lhs > lo_s * area));
        if (threadIdx.x == 0) {
            if (hot) atomicAdd(counts + 2 * f, (uint32_t)hot);
            if (warm) atomicAdd(counts + 2 * f + 1, (uint32_t)warm);
        }
    }
}

}  // namespace

extern "C" int demfi_luma_block_counts(const uint8_t* base, const int64_t* a_offsets, const int64_t* b_offsets, int n, int h, int w,
                                       int sample_bytes, int64_t hi_s, int64_t lo_s, uint32_t* counts, void* stream)
{
    const char* fn = "demfi_luma_block_counts";
    if (!base || !a_offsets || !b_offsets || !counts || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (hi_s < 0 || lo_s < 0 || hi_s > MAX_THRESHOLD || lo_s > MAX_THRESHOLD)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: thresholds %lld, %lld outside 0..2^40", fn, (long long)hi_s, (long long)lo_s);
    if (int st = check_even(fn, sample_bytes, (uintptr_t)base)) return st;
    if (n == 0) return DEMFI_OK;
    DEMFI_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n * 2 * sizeof(uint32_t), (hipStream_t)stream));
    const int nblk = ((w + BS - 1) / BS) * ((h + BS - 1) / BS);
    const dim3 grid((unsigned)((nblk + NT - 1) / NT), (unsigned)min(n, 65535));
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(luma_block_counts_kernel<TAG_TYPE(t)>, grid, dim3(NT), 0, (hipStream_t)stream, base, a_offsets, b_offsets, n, h, w,
                           (uint64_t)hi_s, (uint64_t)lo_s, counts);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
