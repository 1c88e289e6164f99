// Tiles of large frames (demfi_amd/tiling.py): crop uint8 BGR frames into the equal-size tiles of a plan, and paste the kept
// rectangles of computed tiles back into full frames.  The definition is the numpy pair crop_np / stitch_np; these kernels
// move the same bytes.
//
// Both are row copies: a tile row is 3 * tw bytes at (row * tw) * 3 of its tile, a frame row segment starts at
// ((y * w) + x) * 3 of its frame, which has any alignment.  A lane owns one 16-byte piece of one row, cut at the 16-byte
// boundaries of the DESTINATION: piece 0 is the bytes before the first boundary (none when the row starts on one), piece c >= 1
// the c-th aligned 16 bytes, the last one short.  Whole pieces are one aligned 16-byte store fed by one 16-byte load of any
// alignment (global memory serves those; yuv420_sad_kernel reads the same way); the head and the tail go byte by byte.
// Consecutive lanes own consecutive pieces of a row, so a wave reads and writes 1 KiB runs.
//
// The rectangles come from device memory and the kernels cannot trust them: a tile whose rectangle leaves the frame (or whose
// kept rectangle leaves its tile) is skipped as a whole, so no launch reads or writes outside the buffers it was sized for.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;
constexpr int RECT = 6;               // int32 per tile: source y0, x0; kept y0, x0, y1, x1 (frame coordinates)

// piece c of the n-byte row src -> dst
__device__ __forceinline__ void copy_piece(uint8_t* dst, const uint8_t* src, int n, int c)
{
    const int head = min((int)((16 - ((uintptr_t)dst & 15)) & 15), n);
    const int lo = c == 0 ? 0 : head + 16 * (c - 1);
    const int cnt = c == 0 ? head : min(16, n - lo);
    if (cnt <= 0) return;
    if (cnt == 16) {
        *gp<u4_t>(dst + lo) = *(const DEMFI_GLOBAL u4_a1*)(src + lo);
        return;
    }
#pragma unroll
    for (int i = 0; i < 15; ++i)
        if (i < cnt) gp<uint8_t>(dst + lo)[i] = gcp<uint8_t>(src + lo)[i];
}

__host__ __device__ inline int pieces_of(int nbytes) { return (nbytes + 15) / 16 + 1; }

// grid: x = pieces of a tile, y = tile, z = frames (strided)
__global__ __launch_bounds__(NT) void tile_crop_kernel(const uint8_t* __restrict__ src, int64_t src_stride, uint8_t* __restrict__ dst,
                                                      int n, int h, int w, int th, int tw, int n_tiles,
                                                      const int32_t* __restrict__ rects)
{
    const int j = blockIdx.y;
    const int y0 = rects[RECT * j], x0 = rects[RECT * j + 1];
    if (y0 < 0 || x0 < 0 || y0 > h - th || x0 > w - tw) return;
    const int nb = 3 * tw, np = pieces_of(nb);
    const int id = blockIdx.x * NT + threadIdx.x;
    const int y = id / np, c = id - y * np;
    if (y >= th) return;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* s = src + (int64_t)f * src_stride + ((int64_t)(y0 + y) * w + x0) * 3;
        uint8_t* d = dst + (((int64_t)f * n_tiles + j) * th + y) * nb;
        copy_piece(d, s, nb, c);
    }
}

// frame f: tile j read at base + src_offsets[f * n_tiles + j], its kept rectangle written into the frame at dst + dst_offsets[f]
__global__ __launch_bounds__(NT) void tile_stitch_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ src_offsets,
                                                        uint8_t* __restrict__ dst, const int64_t* __restrict__ dst_offsets, int n, int h,
                                                        int w, int th, int tw, int n_tiles, const int32_t* __restrict__ rects)
{
    const int j = blockIdx.y;
    const int32_t* r = rects + RECT * j;
    const int y0 = r[0], x0 = r[1], ky0 = r[2], kx0 = r[3], ky1 = r[4], kx1 = r[5];
    if (y0 < 0 || x0 < 0 || y0 > h - th || x0 > w - tw) return;
    if (ky0 < y0 || kx0 < x0 || ky1 <= ky0 || kx1 <= kx0 || ky1 > y0 + th || kx1 > x0 + tw) return;
    const int nb = 3 * (kx1 - kx0), np = pieces_of(3 * tw);          // the grid is sized for a whole tile row
    const int id = blockIdx.x * NT + threadIdx.x;
    const int row = id / np, c = id - row * np;
    const int y = ky0 + row;
    if (y >= ky1) return;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* s = base + src_offsets[(int64_t)f * n_tiles + j] + ((int64_t)(y - y0) * tw + (kx0 - x0)) * 3;
        uint8_t* d = dst + dst_offsets[f] + ((int64_t)y * w + kx0) * 3;
        copy_piece(d, s, nb, c);
    }
}

// rects: the HOST copy of the plan's rectangles
int check_tiles(const char* fn, const void* a, const void* b, int n, int h, int w, int th, int tw, int n_tiles, const int32_t* rects,
                const void* rects_dev)
{
    if (!a || !b || !rects || !rects_dev || n < 0)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d", fn, n);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (th < 2 || tw < 2 || th > h || tw > w)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: tile size %dx%d outside 2..%dx%d", fn, th, tw, h, w);
    if (n_tiles < 1 || n_tiles > 65535)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d tiles outside 1..65535", fn, n_tiles);
    for (int j = 0; j < n_tiles; ++j) {
        const int32_t* r = rects + RECT * j;
        if (r[0] < 0 || r[1] < 0 || r[0] > h - th || r[1] > w - tw)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: tile %d at (%d, %d) of size %dx%d leaves the %dx%d frame", fn, j, r[0], r[1], th,
                                   tw, h, w);
        if (r[2] < r[0] || r[3] < r[1] || r[4] <= r[2] || r[5] <= r[3] || r[4] > r[0] + th || r[5] > r[1] + tw)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: tile %d keeps rows %d..%d, columns %d..%d outside its rectangle at (%d, %d)", fn, j,
                                   r[2], r[4], r[3], r[5], r[0], r[1]);
    }
    return DEMFI_OK;
}

dim3 grid_for(int n, int th, int tw, int n_tiles)
{
    const int64_t lanes = (int64_t)th * pieces_of(3 * tw);
    return dim3((unsigned)((lanes + NT - 1) / NT), (unsigned)n_tiles, (unsigned)min(n, 65535));
}

}  // namespace

extern "C" int demfi_u8_tile_crop(const uint8_t* src, int64_t src_stride, uint8_t* dst, int n, int h, int w, int th, int tw,
                                  int n_tiles, const int32_t* rects, const int32_t* rects_dev, void* stream)
{
    int st = check_tiles("demfi_u8_tile_crop", src, dst, n, h, w, th, tw, n_tiles, rects, rects_dev);
    if (st < 0) return st;
    if (n > 1 && src_stride < (int64_t)h * w * 3)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_u8_tile_crop: src_stride %lld below the frame size %lld", (long long)src_stride,
                               (long long)h * w * 3);
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(tile_crop_kernel, grid_for(n, th, tw, n_tiles), dim3(NT), 0, (hipStream_t)stream, src, src_stride, dst, n, h, w,
                       th, tw, n_tiles, rects_dev);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_u8_tile_stitch(const uint8_t* base, const int64_t* src_offsets, uint8_t* dst, const int64_t* dst_offsets, int n,
                                    int h, int w, int th, int tw, int n_tiles, const int32_t* rects, const int32_t* rects_dev,
                                    void* stream)
{
    int st = check_tiles("demfi_u8_tile_stitch", base, dst, n, h, w, th, tw, n_tiles, rects, rects_dev);
    if (st < 0) return st;
    if (!src_offsets || !dst_offsets)
        return demfi_set_error(DEMFI_ERR_ARG, "demfi_u8_tile_stitch: NULL offsets");
    if (n == 0) return DEMFI_OK;
    hipLaunchKernelGGL(tile_stitch_kernel, grid_for(n, th, tw, n_tiles), dim3(NT), 0, (hipStream_t)stream, base, src_offsets, dst,
                       dst_offsets, n, h, w, th, tw, n_tiles, rects_dev);
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
