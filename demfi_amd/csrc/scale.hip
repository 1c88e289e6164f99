// Resized output of the Y4M video path (demfi_amd/scale.py, --scale): output payload r is source payload r with every plane resampled
// by a separable polyphase filter.  The kernel computes no weights: per plane and axis it reads the tables of scale.axis_table out of one
// device blob, first[n_out] (int32: the source index of tap 0, may lie outside the axis) and coef[n_out][T] (int16, Q14, every row sums
// to 1 << 14).  With F = 6 and >> an arithmetic shift, in exact integers:
//   horizontal:  t = (sum_j cx[xo][j] * src[y][clamp(fx[xo] + j)] + 2^(13-F)) >> (14 - F)               signed, not clamped
//   vertical:    v = clip((sum_j cy[yo][j] * t[clamp(fy[yo] + j)][xo] + 2^(13+F)) >> (14 + F), 0, peak)
// The definition is scale.scale_payload_np; this kernel gives the same integers.
//
// Accumulators (scale.accumulator_bounds): sum|c| of a row stays below 2 * 2^14, so the horizontal sum fits int32 at every depth
// (65535 * 1.55 * 2^14 < 2^31) and the vertical one at one byte per sample (< 2^29); at two bytes per sample the vertical sum reaches
// 2^36.8 and is kept in 64 bits (one v_mad_i64_i32 per tap).
//
// A workgroup of 256 threads owns a tile of TW = 64 output columns x up to TH = 16 output rows of one plane of one payload.
//   Phase 1, horizontal: the tile's output rows read the clamped source rows r_lo .. r_hi, at most MAXR = 96 of them (the entry point
//   gives a plane fewer output rows per tile when 16 would need more: only beyond a 4:1 shrink).  Thread (row group, column) computes t
//   for its column of every fourth of those rows (two rows a step, four taps a group: eight independent loads in flight) with the
//   column's T coefficients, staged once per tile in LDS as int32 [T][64] (so are the tile's rows of cy), and writes it to the LDS
//   array tile[row][64] (int32): consecutive lanes on consecutive columns, so neither array has a bank conflict.
//   Phase 2, vertical: thread (row = tid / 16, quad = tid % 16) owns 4 consecutive columns of one output row, reads the rows of its taps
//   from LDS with 128-bit reads (the 16 lanes of a row cover its 256 bytes: conflict-free) and accumulates; it stores its 4 samples as
//   one 4- or 8-byte word when the destination address allows, else (and at the plane's right edge) sample by sample.
// No atomics; every LDS and source index is clamped where it is formed, so no table content can take an access out of bounds.  Payload
// offsets and r * dst_stride are 64-bit; offsets inside a payload fit 32 bits (the entry point refuses payloads of 2^31 bytes).
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int TW = 64, TH = 16;         // output columns and rows of a tile
constexpr int MAXR = 96;                // source rows a tile holds in LDS
constexpr int MAXT = 32;                // taps at most
constexpr int FRAC = 6, QBITS = 14;

struct Plane {
    int rows_in, cols_in, rows_out, cols_out;
    int th;                             // output rows of a tile of this plane (1 .. TH)
    int tiles_x, tiles;                 // tiles along a row; in the plane
    int tx, ty;                         // taps
    int fx, cx, fy, cy;                 // byte offsets of the tables in the blob
    int64_t start_in, start_out;        // first sample of the plane in its payload
};
struct Planes {
    int n;
    Plane p[MAXP];
};

typedef int i4_t __attribute__((ext_vector_type(4)));

// the vertical sum with its rounding term -> the sample
template <typename A> __device__ __forceinline__ uint32_t clip_sample(A acc, int peak)
{
    const A v = acc >> (QBITS + FRAC);
    return (uint32_t)(v < 0 ? (A)0 : v > (A)peak ? (A)peak : v);
}

// grid: x = tiles of a plane (the most any plane has), y = (payload, plane) pairs (strided)
template <typename T>
__global__ __launch_bounds__(NT) void payload_scale_kernel(const uint8_t* __restrict__ base, const int64_t* __restrict__ offs, int n, Planes pl,
                                                           int peak, const uint8_t* __restrict__ tables, uint8_t* __restrict__ dst,
                                                           int64_t dst_stride)
{
    typedef typename Acc<T>::type acc_t;
    constexpr int es = (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) int tile[MAXR][TW];
    __shared__ int coefx[MAXT][TW];
    __shared__ int coefy[TH * MAXT];
    const int tid = threadIdx.x;
    for (int rp = blockIdx.y; rp < n * pl.n; rp += gridDim.y) {
        const int r = rp / pl.n, pi = rp - r * pl.n;
        const Plane& P = pl.p[pi];
        if ((int)blockIdx.x >= P.tiles) continue;                           // uniform over the workgroup
        const int tyi = (int)blockIdx.x / P.tiles_x, txi = (int)blockIdx.x - tyi * P.tiles_x;
        const int x0 = txi * TW, y0 = tyi * P.th;
        const int ny = min(P.th, P.rows_out - y0);                           // output rows of this tile
        const auto fx = gcp<int>(tables + P.fx);
        const auto fy = gcp<int>(tables + P.fy);
        const auto cx = gcp<int16_t>(tables + P.cx);
        const auto cy = gcp<int16_t>(tables + P.cy);
        const auto src = gcp<T>(base + offs[r] + P.start_in * es);
        // the source rows of the tile: first[] does not decrease along the axis
        const int r_lo = clampi(fy[y0], 0, P.rows_in - 1);
        const int r_hi = clampi(fy[y0 + ny - 1] + P.ty - 1, r_lo, P.rows_in - 1);
        const int nr = min(r_hi - r_lo + 1, MAXR);
        __syncthreads();                                                     // the tile before has been read
        // ---- phase 1 ----
        const int col = tid & (TW - 1), rg = tid >> 6;
        const int xo = x0 + col;
        const bool live = xo < P.cols_out;
        const int txp = (P.tx + 3) & ~3;                                     // taps in groups of four; the padding taps weigh 0
        for (int j = rg; j < txp; j += NT / TW) coefx[j][col] = live && j < P.tx ? (int)cx[(int64_t)xo * P.tx + j] : 0;
        for (int k = tid; k < ny * P.ty; k += NT) coefy[k] = cy[(int64_t)y0 * P.ty + k];      // the tile's rows of cy lie one behind the other
        __syncthreads();
        const int f0 = live ? fx[xo] : 0;
        // two source rows a step and four taps a group: eight independent loads in flight per lane
        for (int lr = rg; lr < nr; lr += 2 * (NT / TW)) {
            const int lr2 = lr + NT / TW;
            const bool two = lr2 < nr;                                       // uniform over the wave
            const auto row_a = src + (int64_t)(r_lo + lr) * P.cols_in;
            const auto row_b = src + (int64_t)(r_lo + (two ? lr2 : lr)) * P.cols_in;
            int acc_a = 1 << (QBITS - 1 - FRAC), acc_b = acc_a;
            for (int j = 0; j < txp; j += 4) {
                int sa[4], sb[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = clampi(f0 + j + k, 0, P.cols_in - 1);
                    sa[k] = row_a[x], sb[k] = row_b[x];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = coefx[j + k][col];
                    acc_a += c * sa[k], acc_b += c * sb[k];
                }
            }
            tile[lr][col] = acc_a >> (QBITS - FRAC);
            if (two) tile[lr2][col] = acc_b >> (QBITS - FRAC);
        }
        __syncthreads();
        // ---- phase 2 ----
        const int ry = tid >> 4, q = tid & 15;
        const int xq = x0 + 4 * q;
        if (ry < ny && xq < P.cols_out) {
            const int yo = y0 + ry;
            const int g0 = fy[yo];
            const int* crow = coefy + ry * P.ty;
            acc_t a0 = (acc_t)1 << (QBITS - 1 + FRAC), a1 = a0, a2 = a0, a3 = a0;
            for (int j = 0; j < P.ty; ++j) {
                const int lr = clampi(clampi(g0 + j, 0, P.rows_in - 1) - r_lo, 0, MAXR - 1);
                const int c = crow[j];
                const i4_t t = *(const i4_t*)&tile[lr][4 * q];
                a0 += (acc_t)c * t[0];
                a1 += (acc_t)c * t[1];
                a2 += (acc_t)c * t[2];
                a3 += (acc_t)c * t[3];
            }
            const uint32_t v0 = clip_sample(a0, peak), v1 = clip_sample(a1, peak), v2 = clip_sample(a2, peak), v3 = clip_sample(a3, peak);
            uint8_t* o = dst + (int64_t)r * dst_stride + (P.start_out + (int64_t)yo * P.cols_out + xq) * es;
            if (xq + 3 < P.cols_out && ((uintptr_t)o & (4 * es - 1)) == 0) {
                if (es == 1) *gp<uint32_t>(o) = v0 | v1 << 8 | v2 << 16 | v3 << 24;
                else *gp<u2_t>(o) = u2_t{v0 | v1 << 16, v2 | v3 << 16};
            } else {
                const auto os = gp<T>(o);
                os[0] = (T)v0;
                if (xq + 1 < P.cols_out) os[1] = (T)v1;
                if (xq + 2 < P.cols_out) os[2] = (T)v2;
                if (xq + 3 < P.cols_out) os[3] = (T)v3;
            }
        }
    }
}

}  // namespace

extern "C" int demfi_payload_scale(const uint8_t* base, const int64_t* offsets, const int64_t* offsets_dev, int n, const int32_t* planes_in,
                                   const int32_t* planes_out, int n_planes, int sample_bytes, int peak, const uint8_t* tables_dev,
                                   const int32_t* table_desc, uint8_t* dst, int64_t dst_stride, void* stream)
{
    const char* fn = "demfi_payload_scale";
    if (!base || !offsets || !offsets_dev || !planes_in || !planes_out || !tables_dev || !table_desc || !dst)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (int st = check_peak(fn, peak, sample_bytes)) return st;
    PlaneSet in, out;
    if (int st = parse_planes(fn, planes_in, n_planes, 32768, (int64_t)32768 * 32768, false, &in)) return st;
    if (int st = parse_planes(fn, planes_out, n_planes, 32768, (int64_t)32768 * 32768, false, &out)) return st;
    const int64_t Pin = in.P, Pout = out.P;
    Planes pl = {};
    pl.n = n_planes;
    const int64_t blob = table_desc[6 * n_planes];                          // bytes of tables_dev
    int64_t most = 0;                                                        // tiles of the plane that has the most
    for (int p = 0; p < n_planes; ++p) {
        Plane& P = pl.p[p];
        P.rows_in = in.pl.rows[p], P.cols_in = in.pl.cols[p], P.rows_out = out.pl.rows[p], P.cols_out = out.pl.cols[p];
        P.start_in = in.pl.start[p], P.start_out = out.pl.start[p];
        const int32_t* d = table_desc + 6 * p;
        P.fx = d[0], P.cx = d[1], P.tx = d[2], P.fy = d[3], P.cy = d[4], P.ty = d[5];
        if (P.tx < 1 || P.tx > MAXT || P.ty < 1 || P.ty > MAXT)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d has %d x %d taps (1..%d each)", fn, p, P.tx, P.ty, MAXT);
        if (P.fx < 0 || P.cx < 0 || P.fy < 0 || P.cy < 0 || ((P.fx | P.fy) & 3) || ((P.cx | P.cy) & 1))
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d: table offsets %d, %d, %d, %d (first: multiples of 4, coef: of 2, none negative)",
                                   fn, p, P.fx, P.cx, P.fy, P.cy);
        if (P.fx + 4 * (int64_t)P.cols_out > blob || P.cx + 2 * (int64_t)P.cols_out * P.tx > blob || P.fy + 4 * (int64_t)P.rows_out > blob ||
            P.cy + 2 * (int64_t)P.rows_out * P.ty > blob)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d: a table ends behind the %lld bytes of the blob", fn, p, (long long)blob);
        // output rows per tile: the most whose source rows fit MAXR.  first[o + k] - first[o] <= ceil(k rows_in / rows_out)
        int th = TH;
        while (th > 1 && ((int64_t)(th - 1) * P.rows_in + P.rows_out - 1) / P.rows_out + P.ty > MAXR) --th;
        P.th = th;
        P.tiles_x = (P.cols_out + TW - 1) / TW;
        P.tiles = P.tiles_x * ((P.rows_out + th - 1) / th);
        most = max(most, (int64_t)P.tiles);
    }
    if (Pin * sample_bytes >= ((int64_t)1 << 31) || Pout * sample_bytes >= ((int64_t)1 << 31))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: payloads of %lld -> %lld bytes (below 2^31 each)", fn, (long long)(Pin * sample_bytes),
                               (long long)(Pout * sample_bytes));
    if (int st = check_dst_stride(fn, dst_stride, Pout * sample_bytes)) return st;
    uintptr_t odd = (uintptr_t)base | (uintptr_t)dst | (uintptr_t)dst_stride;
    if (int st = walk_offsets(fn, offsets, n, 1, 1, OFFS_ALL, 0, NO_LIMIT, 0, &odd)) return st;
    if (int st = check_even(fn, sample_bytes, odd)) return st;
    if (((uintptr_t)tables_dev & 3)) return demfi_set_error(DEMFI_ERR_ARG, "%s: tables_dev is not on a 4-byte boundary", fn);
    if (n == 0) return DEMFI_OK;
    const dim3 grid((unsigned)most, (unsigned)min((int64_t)n * n_planes, (int64_t)4096));
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(payload_scale_kernel<TAG_TYPE(t)>, grid, dim3(NT), 0, (hipStream_t)stream, base, offsets_dev, n, pl, peak, tables_dev, dst,
                           dst_stride);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
