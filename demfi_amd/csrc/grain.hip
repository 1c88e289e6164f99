// Film grain at the egress of the Y4M video path (demfi_amd/grain.py, --grain): written payload r is the source payload at base +
// offsets[r] with synthetic grain added to every plane.  In exact integers, >> an arithmetic shift:
//   mix32(x):        x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (uint32)
//   white(X, Y)    = b0 + b1 + b2 + b3 - 510 over the bytes of mix32(key ^ mix32((Y << 16) | X))         (|white| <= 510)
//   F(x, y)        = sum_{i, j = -R..R} c[i] c[j] white(x + 2 + i, y + 2 + j),  c = [1] / [1,2,1] / [1,4,6,4,1]
//   out            = clip(v + ((F * G[min(L >> (d - 8), 255)] + 2^15) >> 16), min(lo, v), max(hi, v))
// key is the plane's of the payload (three per payload, computed on the host: the kernel does not know how they are derived), G the
// plane's 256-entry gain table (luma / chroma, built on the host: the kernel computes no curve and no square root), L the frame's own
// luma: v itself in the luma plane, for the chroma sample (x, y) the luma sample at (min(x sx, w - 1), min(y sy, h - 1)) of the same
// SOURCE payload.  The definition is grain.grain_payload_np; this kernel gives the same integers.
//
// Accumulator (grain.accumulator_bounds): |F| <= 510 * 256 and the host's cap S <= 8 keep |F * G| + 2^15 below 2^31 at every depth and
// size (the widest: R = 2 at 16 bits, about 1.69e9), so the product is a 32-bit one; the entry point refuses a table entry that could
// take it further.
//
// A workgroup of 256 threads owns a tile of TW = 64 columns x TH = 16 rows of one plane of one payload.
//   R > 0: all threads hash the white cells of the tile and its R-wide halo once into LDS (int16 [TH + 2R][80], two cells and one
//   32-bit store a step).  The horizontal taps: thread (row, segment) reads the 8 + 2R cells of its 8 columns as two 128-bit words and
//   writes its 8 sums (|.| <= 510 * 16: int16) as one into hz (int16 [TH + 2R][72]).  The vertical taps run in the last phase, straight
//   from 2R + 1 rows of hz with 128-bit reads.  LDS instructions, not bytes, are what such a filter pays for: one int16 a lane and
//   access cost the 5 x 5 filter a fifth more at 10 bits (profiles/grain.md).  Row strides of 160 and 144 bytes keep every 128-bit access
//   aligned; in the byte kernel's last phase the four rows of a ds_read_b128 lane group (0, 3, 5, 6 at bytes 144 row + 32 word) meet
//   pairwise on four 16-byte slots: 2-way, counted by hand, not measured.  R = 0 skips LDS for the noise: a thread hashes the cells of
//   its samples.
//   The last phase: thread (row = item / Q, word = item % Q) owns the 16 bytes = SPT samples (16 bytes, 8 uint16) at column word * SPT of
//   its row; 64 (128) threads have an item.
//   v is one 16-byte load and one 16-byte store where the item lies inside the plane and both addresses are 16-byte aligned, else
//   sample by sample (decided per item: ragged right edges and rows that start off 16 bytes).  The plane's gain table is in LDS.
// No atomics, plain vector stores; payload offsets and r * dst_stride are 64-bit; every LDS index is formed from the thread's own tile
// coordinates and every global one is checked against the plane, so no table or key content can take an access out of bounds.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int TW = 64, TH = 16;         // columns and rows of a tile
constexpr int MAXR = 2;
constexpr int WS = TW + 16;             // row stride of the white cells (int16): a row is 160 bytes, every 8-cell segment 16-byte aligned
constexpr int HS = TW + 8;              // row stride of the horizontal sums (int16): 144 bytes
constexpr int MAX_SIDE = 65531;

struct Planes {
    int n;
    int rows[MAXP], cols[MAXP];
    int tiles_x[MAXP], tiles[MAXP];
    int sx, sy;                         // chroma subsampling factors (1 or 2)
    int64_t start[MAXP];                // first sample of the plane in the payload
};

struct Rule {
    int shift;                          // d - 8
    int lo[2], hi[2];                   // nominal range: luma, chroma
};

// int16 number i of the 16 that two 16-byte LDS words hold, sign-extended
__device__ __forceinline__ int half_at(const u4_t& a, const u4_t& b, int i)
{
    const uint32_t w = i < 8 ? a[i >> 1] : b[(i - 8) >> 1];
    return (i & 1) ? (int)w >> 16 : (int)(short)(w & 0xffffu);
}
__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ int white_cell(uint32_t key, uint32_t X, uint32_t Y)
{
    const uint32_t u = mix32(key ^ mix32((Y << 16) | X));
    return (int)__builtin_amdgcn_sad_u8(u, 0u, 0u) - 510;                    // the sum of the four bytes: v_sad_u8 against zero
}

template <int R> __device__ __forceinline__ constexpr int tap(int i)
{
    return R == 0 ? 1 : R == 1 ? (i == 1 ? 2 : 1) : (i == 2 ? 6 : (i == 1 || i == 3) ? 4 : 1);
}

// grid: x = tiles of a plane (the most any plane has), y = (payload, plane) pairs (strided)
template <typename T, int R>
__global__ __launch_bounds__(NT) void payload_grain_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs,
                                                           const uint32_t* __restrict__ keys, int n, Planes pl, Rule rule,
                                                           const int* __restrict__ gains, uint8_t* __restrict__ dst, int64_t dst_stride)
{
    constexpr int es = (int)sizeof(T), SPT = 16 / es, Q = TW / SPT, ITEMS = TH * Q;
    __shared__ int gain[256];
    __shared__ __attribute__((aligned(16))) short cells[R ? TH + 2 * R : 1][WS];
    __shared__ __attribute__((aligned(16))) short hz[R ? TH + 2 * R : 1][HS];
    const int tid = threadIdx.x;
    for (int rp = blockIdx.y; rp < n * pl.n; rp += gridDim.y) {
        const int r = rp / pl.n, p = rp - r * pl.n;
        if ((int)blockIdx.x >= pl.tiles[p]) continue;                        // uniform over the workgroup
        const int chroma = p > 0;
        const int rows = pl.rows[p], cols = pl.cols[p];
        const int tyi = (int)blockIdx.x / pl.tiles_x[p], txi = (int)blockIdx.x - tyi * pl.tiles_x[p];
        const int x0 = txi * TW, y0 = tyi * TH;
        const uint32_t key = keys[3 * (int64_t)r + p];
        const uint8_t* pay = base + offs[r];
        __syncthreads();                                                     // the tile before has been read
        gain[tid] = gains[chroma * 256 + tid];
        if (R > 0) {
            constexpr int CW = TW + 2 * R, CH = TH + 2 * R;              // the tile and its halo
            for (int k = tid; k < CH * (CW / 2); k += NT) {                  // two cells a step, one 32-bit LDS store
                const int ly = k / (CW / 2), lx = 2 * (k - ly * (CW / 2));
                const uint32_t Y = (uint32_t)(y0 + ly + 2 - R), X = (uint32_t)(x0 + lx + 2 - R);
                *(uint32_t*)&cells[ly][lx] = pack16(white_cell(key, X, Y), white_cell(key, X + 1, Y));
            }
            __syncthreads();
            if (tid < CH * (TW / 8)) {                                       // the horizontal taps: 8 columns of a row a thread
                const int ly = tid >> 3, c0 = 8 * (tid & 7);
                const u4_t a = *(const u4_t*)&cells[ly][c0], b = *(const u4_t*)&cells[ly][c0 + 8];   // b: 2R cells of it count
                int t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    t[j] = 0;
#pragma unroll
                    for (int i = 0; i <= 2 * R; ++i) t[j] += tap<R>(i) * half_at(a, b, j + i);
                }
                *(u4_t*)&hz[ly][c0] = u4_t{pack16(t[0], t[1]), pack16(t[2], t[3]), pack16(t[4], t[5]), pack16(t[6], t[7])};
            }
        }
        __syncthreads();
        if (tid >= ITEMS) continue;                                          // no barrier below
        const int ry = tid / Q, xq = x0 + (tid - ry * Q) * SPT, y = y0 + ry;
        if (y >= rows || xq >= cols) continue;
        const int nv = min(SPT, cols - xq);
        const int64_t at = (pl.start[p] + (int64_t)y * cols + xq) * es;     // the item's first byte in the payload
        const uint8_t* sp = pay + at;
        uint8_t* dp = dst + (int64_t)r * dst_stride + at;
        const bool wide = nv == SPT && (((uintptr_t)sp | (uintptr_t)dp) & 15) == 0;
        const int lo = rule.lo[chroma], hi = rule.hi[chroma];
        const DEMFI_GLOBAL T* lrow = gcp<T>(pay) + (int64_t)min(y * pl.sy, pl.rows[0] - 1) * pl.cols[0];   // chroma: the luma row of this row
        // the item, WIDE: all SPT samples, one 16-byte load and store, no sample of it predicated; else the nv samples one by one
        auto item = [&](auto wide_c) {
            constexpr bool WIDE = decltype(wide_c)::value;
            uint32_t v[SPT], L[SPT];
            if (WIDE) {
                const u4_t w = *gcp<u4_t>(sp);
#pragma unroll
                for (int k = 0; k < SPT; ++k) v[k] = Samples<T>::at(w, k);
            } else {
#pragma unroll
                for (int k = 0; k < SPT; ++k) v[k] = k < nv ? (uint32_t)gcp<T>(sp)[k] : 0u;
            }
            if (chroma) {                                                    // uniform over the workgroup
#pragma unroll
                for (int k = 0; k < SPT; ++k) L[k] = WIDE || k < nv ? (uint32_t)lrow[min((xq + k) * pl.sx, pl.cols[0] - 1)] : 0u;
            } else {
#pragma unroll
                for (int k = 0; k < SPT; ++k) L[k] = v[k];
            }
            int f[SPT];
            if (R > 0) {                                                     // the vertical taps, straight from the rows of hz
#pragma unroll
                for (int k = 0; k < SPT; ++k) f[k] = 0;
#pragma unroll
                for (int j = 0; j <= 2 * R; ++j) {
                    const short* row = &hz[ry + j][xq - x0];
                    const u4_t a = *(const u4_t*)row, b = SPT > 8 ? *(const u4_t*)(row + 8) : a;
#pragma unroll
                    for (int k = 0; k < SPT; ++k) f[k] += tap<R>(j) * half_at(a, b, k);
                }
            } else {
#pragma unroll
                for (int k = 0; k < SPT; ++k) f[k] = white_cell(key, (uint32_t)(xq + k + 2), (uint32_t)(y + 2));
            }
            uint32_t o[SPT];
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int g = gain[min(L[k] >> rule.shift, 255u)];
                const int s = (int)v[k], d = (f[k] * g + (1 << 15)) >> 16;
                o[k] = (uint32_t)min(max(s + d, min(lo, s)), max(hi, s));
            }
            if (WIDE) {
                u4_t w = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < SPT; ++k) Samples<T>::put(w, k, o[k]);
                *gp<u4_t>(dp) = w;
            } else {
#pragma unroll
                for (int k = 0; k < SPT; ++k)
                    if (k < nv) gp<T>(dp)[k] = (T)o[k];
            }
        };
        if (wide) item(std::true_type{});
        else item(std::false_type{});
    }
}

}  // namespace

extern "C" int demfi_payload_grain(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, const uint32_t* keys,
                                   const uint32_t* keys_dev, int n, const int32_t* planes, int n_planes, int sample_bytes, int depth,
                                   int full_range, int size, const int32_t* gains, const int32_t* gains_dev, uint8_t* dst,
                                   int64_t dst_stride, void* stream)
{
    const char* fn = "demfi_payload_grain";
    if (!base || !offsets || !offsets_dev || !keys || !keys_dev || !planes || !gains || !gains_dev || !dst)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (!is_depth(depth) || sample_bytes != (depth > 8 ? 2 : 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: %d bits in %d bytes per sample (8 bits in 1; 10, 12, 14 or 16 in 2)", fn, depth, sample_bytes);
    if (int st = check_flag(fn, "full_range", full_range)) return st;
    if (size < 0 || size > MAXR) return demfi_set_error(DEMFI_ERR_ARG, "%s: size=%d (0..%d)", fn, size, MAXR);
    PlaneSet ps;
    if (int st = parse_planes(fn, planes, n_planes, MAX_SIDE, (int64_t)MAX_SIDE * MAX_SIDE, true, &ps)) return st;
    const int64_t P = ps.P;
    Planes pl = {};
    pl.n = n_planes, pl.sx = pl.sy = 1;
    int64_t most = 0;                                                        // tiles of the plane that has the most
    for (int p = 0; p < n_planes; ++p) {
        pl.rows[p] = ps.pl.rows[p], pl.cols[p] = ps.pl.cols[p], pl.start[p] = ps.pl.start[p];
        pl.tiles_x[p] = (pl.cols[p] + TW - 1) / TW;
        pl.tiles[p] = pl.tiles_x[p] * ((pl.rows[p] + TH - 1) / TH);
        most = max(most, (int64_t)pl.tiles[p]);
    }
    if (n_planes == MAXP) {                                                  // the chroma planes: one shape, the luma's or half of it, rounded up
        const int h = pl.rows[0], w = pl.cols[0], ch = pl.rows[1], cw = pl.cols[1];
        pl.sy = ch == h ? 1 : 2, pl.sx = cw == w ? 1 : 2;
        if (pl.rows[2] != ch || pl.cols[2] != cw || (ch != h && ch != (h + 1) / 2) || (cw != w && cw != (w + 1) / 2))
            return demfi_set_error(DEMFI_ERR_ARG, "%s: chroma planes of %d x %d and %d x %d beside a luma plane of %d x %d", fn, ch, cw,
                                   pl.rows[2], pl.cols[2], h, w);
    }
    if (P * sample_bytes >= ((int64_t)1 << 31))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: a payload of %lld bytes (below 2^31)", fn, (long long)(P * sample_bytes));
    if (int st = check_dst_stride(fn, dst_stride, P * sample_bytes)) return st;
    uintptr_t odd = (uintptr_t)base | (uintptr_t)dst | (uintptr_t)dst_stride;
    if (int st = walk_offsets(fn, offsets, n, 1, 1, OFFS_ALL, 0, NO_LIMIT, 0, &odd)) return st;
    if (int st = check_even(fn, sample_bytes, odd)) return st;
    if (((uintptr_t)gains_dev & 3) || ((uintptr_t)keys_dev & 3))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: gains_dev or keys_dev is not on a 4-byte boundary", fn);
    // |F| <= 510 * (sum of the taps)^2: the 32-bit product holds for gains up to this
    const int64_t fmax = 510LL << (4 * size), gmax = (((int64_t)1 << 31) - 1 - (1 << 15)) / fmax;
    for (int i = 0; i < 512; ++i)
        if (gains[i] < 0 || gains[i] > gmax)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: gain %d is %d (0..%lld at size %d)", fn, i, gains[i], (long long)gmax, size);
    if (n == 0) return DEMFI_OK;
    Rule rule = {};
    rule.shift = depth - 8;
    for (int c = 0; c < 2; ++c) {
        rule.lo[c] = full_range ? 0 : 16 << rule.shift;
        rule.hi[c] = full_range ? (1 << depth) - 1 : (c ? 240 : 235) << rule.shift;
    }
    const dim3 grid((unsigned)most, (unsigned)min((int64_t)n * n_planes, (int64_t)4096));
    by_sample(sample_bytes, [&](auto t) {
        by_int<0, MAXR>(size, [&](auto r) {
            hipLaunchKernelGGL((payload_grain_kernel<TAG_TYPE(t), TAG_VALUE(r)>), grid, dim3(NT), 0, (hipStream_t)stream, base, offsets_dev, keys_dev,
                               n, pl, rule, gains_dev, dst, dst_stride);
        });
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
