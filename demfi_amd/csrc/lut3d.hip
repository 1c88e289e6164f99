// A user's 3D colour LUT at the egress of the Y4M edge (demfi_amd/video.py --lut): one stateless stage between the scaler and the encode.
//   demfi_rgb_lut3d   RGB payloads (uint16 [3, h, w], planes B, G, R: those of colour.hip) -> RGB payloads of 16-bit encoded values
// The definition is numpy code in demfi_amd/lut3d.py (lut_payload_np); the kernel matches it byte for byte.  Per pixel and channel
// code = inv_in[v], (idx, frac) = axt[code]; tetrahedral interpolation over the four lattice points the sorted fractions name, in
// uint32: the weights sum to 65535, the numerator stays below 65535^2 + 32768 < 2^32, and the division by 65535 is
// (n + (n >> 16) + 1) >> 16, the floor over that whole range (tests/test_lut3d.py).  A tie gives the disputed vertex the weight 0, so
// the three compare-swaps need not be stable.
//
// The lane layout is colour.hip's: a lane owns a strip of 8 pixels of one row, one 16-byte access per plane in and out; strips cut by
// the right edge or off the vector boundary (payloads are only sample-aligned) take the sample path of load_n / store_n.
//   inv_in: 128 KiB, read through L2 with 2-byte loads, as demfi_linear_to_yuv reads its table.
//   axt:    per code idx << 16 | frac, at most 16 KiB; a workgroup copies it into LDS once, so nothing is divided by N - 1 here.
//   cube:   [N^3][4] uint16 (R, G, B, 0): one lattice point is one 8-byte load, four a pixel, read through L2 (39 KB at N = 17, 287 KB
//           at 33, 2.2 MB at 65).  cube_in_lds = 1 (N <= 17): a workgroup copies the cube into LDS too and walks several chunks of
//           lanes to pay for the copy; profiles/lut3d.md has the comparison.
// Whatever the tables hold, no load leaves them: a code is clamped to the peak and an index to N - 2.  64-bit offsets, no atomics.
#include "yuv_common.h"

namespace {

constexpr int MAXF = 4096;            // payloads along the grid's y; a block walks the rest
constexpr int AXT_MAX = 4096;         // entries of axt at 12 bits
constexpr int LDS_N = 17;             // the largest cube kept in LDS: 17^3 * 8 = 39304 bytes beside the 16 KiB of axt
constexpr int LDS_BLOCKS = 512;       // chunks of the LDS form along the grid's x: two workgroups a CU

__device__ __forceinline__ void swap_desc(int& fa, int& sa, int& fb, int& sb)       // (fa, sa) keeps the larger fraction
{
    if (fa < fb) {
        const int f = fa, s = sa;
        fa = fb, sa = sb, fb = f, sb = s;
    }
}

// payload f read at src + offs[f] BYTES: row y x columns x0 .. x0+7 of its three planes -> the same strip of the written payload
template <bool LDS_CUBE>
__global__ __launch_bounds__(NT) void rgb_lut3d_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offs,
                                                      uint16_t* __restrict__ dst, int64_t dst_stride, int n, int h, int w, int peak, int N,
                                                      const uint16_t* __restrict__ inv_in, const uint32_t* __restrict__ axt,
                                                      const u2_t* __restrict__ cube, int chunks)
{
    __shared__ uint32_t ax[AXT_MAX];
    __shared__ u2_t lc[LDS_CUBE ? LDS_N * LDS_N * LDS_N : 1];
    for (int i = threadIdx.x; i <= peak; i += NT) ax[i] = gcp<uint32_t>(axt)[i];
    if (LDS_CUBE)
        for (int i = threadIdx.x; i < N * N * N; i += NT) lc[i] = gcp<u2_t>(cube)[i];
    __syncthreads();
    const int ns = (w + SX - 1) / SX, N2 = N * N, top = 1 + N + N2;
    const int64_t hw = (int64_t)h * w;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int id = chunk * NT + threadIdx.x;
        if (id >= h * ns) continue;
        const int y = id / ns, x0 = (id - y * ns) * SX;
        for (int f = blockIdx.y; f < n; f += gridDim.y) {
            const uint16_t* P = (const uint16_t*)(src + offs[f]);
            uint32_t a[3][8];                          // idx << 16 | frac of the strip's pixels, planes B, G, R
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                int t[8];
                load_n<uint16_t, 8>(P + ch * hw + (int64_t)y * w, x0, w, t);
#pragma unroll
                for (int px = 0; px < SX; ++px) a[ch][px] = ax[min((int)gcp<uint16_t>(inv_in)[t[px]], peak)];
            }
            int o[3][8];
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                const int ib = min((int)(a[0][px] >> 16), N - 2), ig = min((int)(a[1][px] >> 16), N - 2),
                          ir = min((int)(a[2][px] >> 16), N - 2);
                int f1 = (int)(a[2][px] & 0xffffu), s1 = 1, f2 = (int)(a[1][px] & 0xffffu), s2 = N, f3 = (int)(a[0][px] & 0xffffu), s3 = N2;
                swap_desc(f1, s1, f2, s2);
                swap_desc(f2, s2, f3, s3);
                swap_desc(f1, s1, f2, s2);
                const int v0 = (ib * N + ig) * N + ir;
                u2_t q[4];
                if (LDS_CUBE) {
                    q[0] = lc[v0], q[1] = lc[v0 + s1], q[2] = lc[v0 + s1 + s2], q[3] = lc[v0 + top];
                } else {
                    q[0] = gcp<u2_t>(cube)[v0], q[1] = gcp<u2_t>(cube)[v0 + s1], q[2] = gcp<u2_t>(cube)[v0 + s1 + s2],
                    q[3] = gcp<u2_t>(cube)[v0 + top];
                }
                const uint32_t wt[4] = {(uint32_t)(65535 - f1), (uint32_t)(f1 - f2), (uint32_t)(f2 - f3), (uint32_t)f3};
                uint32_t num[3] = {32767u, 32767u, 32767u};            // B, G, R
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    num[0] += (q[k][1] & 0xffffu) * wt[k];
                    num[1] += (q[k][0] >> 16) * wt[k];
                    num[2] += (q[k][0] & 0xffffu) * wt[k];
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) o[ch][px] = (int)((num[ch] + (num[ch] >> 16) + 1u) >> 16);
            }
            uint16_t* D = dst + (int64_t)f * dst_stride + (int64_t)y * w + x0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) store_n<uint16_t, 8>(D + ch * hw, o[ch], w - x0);
        }
    }
}

}  // namespace

extern "C" int demfi_rgb_lut3d(const uint8_t* src, const int64_t* offsets, const int64_t* offsets_dev, int n, int h, int w, int depth,
                               const uint16_t* inv_in, int cube_n, const uint16_t* cube, const uint32_t* axis_table, int cube_in_lds,
                               uint8_t* dst, int64_t dst_stride, void* stream)
{
    const char* fn = "demfi_rgb_lut3d";
    if (!src || !offsets || !offsets_dev || !inv_in || !cube || !axis_table || !dst) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (depth != 8 && depth != 10 && depth != 12)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: bit depth %d (8, 10 or 12: the table of the codes has at most 4096 entries)", fn, depth);
    if (cube_n < 2 || cube_n > 65) return demfi_set_error(DEMFI_ERR_ARG, "%s: cube size %d outside 2..65", fn, cube_n);
    if (int st = check_flag(fn, "cube_in_lds", cube_in_lds)) return st;
    if (cube_in_lds && cube_n > LDS_N)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: cube_in_lds with a cube size of %d (%d at most)", fn, cube_n, LDS_N);
    if (((uintptr_t)axis_table & 3) || ((uintptr_t)cube & 7))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: axis_table off a 4-byte or cube off an 8-byte boundary", fn);
    const int64_t payload = (int64_t)6 * h * w;
    if (int st = check_dst_stride(fn, dst_stride, payload)) return st;
    uintptr_t odd = (uintptr_t)src | (uintptr_t)inv_in | (uintptr_t)dst | (uintptr_t)dst_stride;
    if (int st = walk_offsets(fn, offsets, n, 1, 1, OFFS_ALL, 0, NO_LIMIT, 0, &odd)) return st;
    if (int st = check_even(fn, 2, odd)) return st;
    if (n == 0) return DEMFI_OK;
    if (dst_stride > (INT64_MAX - payload) / n) return demfi_set_error(DEMFI_ERR_ARG, "%s: dst_stride %lld leaves the address space", fn, (long long)dst_stride);
    int64_t lo = offsets[0], hi = offsets[0];
    for (int i = 1; i < n; ++i) lo = offsets[i] < lo ? offsets[i] : lo, hi = offsets[i] > hi ? offsets[i] : hi;
    if (hi > INT64_MAX - payload) return demfi_set_error(DEMFI_ERR_ARG, "%s: offset %lld leaves the address space", fn, (long long)hi);
    const uintptr_t s0 = (uintptr_t)src + (uintptr_t)lo, s1 = (uintptr_t)src + (uintptr_t)hi + (uintptr_t)payload;
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((n - 1) * dst_stride + payload);
    if (s0 < d1 && d0 < s1) return demfi_set_error(DEMFI_ERR_ARG, "%s: the source payloads and dst overlap", fn);
    const int64_t lanes = (int64_t)h * ((w + SX - 1) / SX);
    const int chunks = (int)((lanes + NT - 1) / NT);
    const dim3 grid((unsigned)(cube_in_lds ? min(chunks, LDS_BLOCKS) : chunks), (unsigned)min(n, cube_in_lds ? 1 : MAXF));
    hipStream_t s = (hipStream_t)stream;
    by_bool(cube_in_lds != 0, [&](auto lds) {
        hipLaunchKernelGGL(rgb_lut3d_kernel<TAG_VALUE(lds)>, grid, dim3(NT), 0, s, src, offsets_dev, (uint16_t*)dst, dst_stride / 2, n, h, w,
                           (1 << depth) - 1, cube_n, inv_in, axis_table, (const u2_t*)cube, chunks);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
