// Debanding of the Y4M video path in front of the network (demfi_amd/deband.py, --deband): a range-limited box mean in exact integers, on
// every plane of every payload as a plane in its own right, OUT OF PLACE (src -> dst: every tap reads the plane as it was).  For a sample c
// at (x, y) of a plane of rows x cols: rx = min(R, x, cols - 1 - x), ry = min(R, y, rows - 1 - y) (the window is clipped symmetrically about
// the sample and never leaves the plane), N = the samples v of the window with |v - c| < thr, out = (2 sum(N) + n) / (2 n) floored.  The
// definition is deband.deband_payload_np; this kernel gives the same integers.  The phase columns of the plane table are ignored.
//
// Tile: TX x TY = 64 x 32 samples of one plane of one payload, tile (i, j) at (64 i, 32 j).  The tile with a halo of 16 goes to LDS as
// 16-bit samples whatever the stored size: LR x LP = 64 rows x 104 samples = 13312 bytes (96 samples used; a pitch of 13 16-byte words, an
// odd number, so the 8 rows a wave reads start at different banks; the 128-bit reads of a wave are then at most 2-way conflicted, which
// costs nothing that shows: the kernel issues 5 of them per 8 x 33 taps).  Strips of 8 wholly inside the plane are one packed global
// load / store at any sample address (Strip of payload_kit.h), ragged ones go sample by sample.  Out-of-plane positions are never loaded;
// a tap there is excluded by rx / ry, so any stored bits of a 16-bit container are samples.
//
// A thread owns a strip of 8 consecutive samples of a row.  For each of the 2 ry + 1 window rows it reads the 8 + 2R samples its windows
// cover as aligned 128-bit LDS reads (3 words up to R = 8, 5 above), unpacks them into registers once, and slides over them with
// compile-time indices: the radius is a template argument (by_int over 1 .. 16), so no register array is indexed at run time and nothing
// spills.  Per tap: e = v - (c - thr + 1), one unsigned compare e < 2 thr - 1 (that is |v - c| < thr), a conditional add of e and a carry
// add into n: 32-bit VALU, five operations a tap.  Tiles within R of a plane border (or ragged) take the EDGE form, a workgroup-uniform
// branch: there the row loop runs to the thread's own ry and every tap also asks rx >= |i|.
// out = c - (thr - 1) + (2 sum(e) + n) / (2 n): the numerator is below 2^24 (deband.accumulator_bounds), so it is exact in a float; the
// quotient is a float multiply by 1 / (2 n) and one integer correction step either way.  int32 throughout; every offset into a payload is
// 64-bit; no atomics.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int TX = 64, TY = 32;         // a tile: samples x rows
constexpr int HX = 16, HY = 16;         // halo columns and rows in LDS: the greatest radius
constexpr int LP = TX + 2 * HX + 8;     // LDS row pitch in samples: 13 words of 16 bytes
constexpr int LR = TY + 2 * HY;         // LDS rows
constexpr int SX = TX / 8;              // strips of a tile row
constexpr int MAX_ENTRIES = 6;          // 3 planes x 2 fields
constexpr int MAX_SIDE = 16384;
constexpr int MAX_THR8 = 8, MAX_RADIUS = 16;
static_assert(TY * SX == NT, "one thread a strip");
static_assert(MAX_RADIUS <= HX && MAX_RADIUS <= HY && LP % 8 == 0, "the halo holds the widest window; rows start on a 16-byte word");

struct Plane {                          // one entry of the plane table (deblock.plane_table)
    int64_t first, pitch;               // first sample in the payload; samples from a row to the next
    int rows, cols;
};
struct Planes {
    int n;
    Plane p[MAX_ENTRIES];
};

__host__ __device__ inline int axis_tiles(int n, int T) { return (n + T - 1) / T; }

// The strip of 8 samples at row r, strip k of the tile (plane position (x, y)) -> res.  lds: the tile's image.  EDGE: the window of every
// sample is clipped to (rx, ry); strips may be ragged (samples outside the plane give values nobody stores).
template <int R, bool EDGE>
__device__ __forceinline__ void filter_strip(const uint16_t* lds, int r, int k, int x, int y, int rows, int cols, int thr, int (&res)[8])
{
    constexpr int W0 = (HX - R) / 8, W1 = (HX + 7 + R) / 8, NW = W1 - W0 + 1;      // the 16-byte words of a row the windows cover
    const uint16_t* base = lds + (HY + r) * LP + 8 * (k + W0);
    const u4_t cw = *(const u4_t*)(lds + (HY + r) * LP + HX + 8 * k);
    const unsigned span = 2u * (unsigned)thr - 1u;
    int cb[8], sum[8], cnt[8], rx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        cb[i] = (int)sample_at<uint16_t>(cw, i) - (thr - 1), sum[i] = 0, cnt[i] = 0;
        rx[i] = EDGE ? min(R, min(x + i, cols - 1 - (x + i))) : R;             // negative outside the plane: no tap
    }
    const int ry = EDGE ? max(0, min(R, min(y, rows - 1 - y))) : R;
#pragma unroll 1
    for (int j = -ry; j <= ry; ++j) {
        int v[8 * NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const u4_t word = *(const u4_t*)(base + j * LP + 8 * w);
#pragma unroll
            for (int s = 0; s < 8; ++s) v[8 * w + s] = (int)sample_at<uint16_t>(word, s);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int t = -R; t <= R; ++t) {
                const int e = v[HX - 8 * W0 + i + t] - cb[i];
                bool near = (unsigned)e < span;
                if (EDGE) near = near && rx[i] >= (t < 0 ? -t : t);
                sum[i] += near ? e : 0;
                cnt[i] += near ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = max(cnt[i], 1);                                        // 0 only for a sample outside the plane
        const int num = 2 * sum[i] + n, den = 2 * n;                         // num < 2^24, den <= 2178: both exact in a float
        int q = (int)((float)num * (1.0f / (float)den));                     // within one of the floor
        const int rem = num - q * den;
        q += (rem >= den ? 1 : 0) - (rem < 0 ? 1 : 0);
        res[i] = cb[i] + q;
    }
}

// grid: x = tiles of a plane (strided), y = (payload, table entry) pairs (strided).  T: the stored sample type; R: the radius.
template <typename T, int R>
__global__ __launch_bounds__(NT) void payload_deband_kernel(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int n,
                                                            Planes tab, int thr)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[LR * LP];
    typedef Strip<T> S;
    const int tid = threadIdx.x;
    const int64_t pairs = (int64_t)n * tab.n;
    for (int64_t pr = blockIdx.y; pr < pairs; pr += gridDim.y) {
        const Plane pl = tab.p[pr % tab.n];
        const T* in = (const T*)(src + (pr / tab.n) * src_stride) + pl.first;
        T* out = (T*)(dst + (pr / tab.n) * dst_stride) + pl.first;
        const int ntx = axis_tiles(pl.cols, TX), nty = axis_tiles(pl.rows, TY);
        for (int t = blockIdx.x; t < ntx * nty; t += gridDim.x) {
            const int x0 = (t % ntx) * TX, y0 = (t / ntx) * TY;             // LDS (r, c) is plane (y0 - HY + r, x0 - HX + c)
            // ---- the tile and a halo of R into LDS: strips of 8 ----
            for (int u = tid; u < LR * ((TX + 2 * HX) / 8); u += NT) {
                const int r = u / ((TX + 2 * HX) / 8), k = u % ((TX + 2 * HX) / 8);
                const int y = y0 - HY + r, x = x0 - HX + 8 * k;
                if (r < HY - R || r >= HY + TY + R || 8 * k + 8 <= HX - R || 8 * k >= HX + TX + R) continue;     // beyond the halo of R
                if (y < 0 || y >= pl.rows || x + 8 <= 0 || x >= pl.cols) continue;
                const T* g = in + (int64_t)y * pl.pitch + x;
                uint16_t* l = lds + r * LP + 8 * k;
                if (x >= 0 && x + 8 <= pl.cols) {
                    const typename S::V v = S::load(g);
                    u4_t w = u4_t(0u);
#pragma unroll
                    for (int i = 0; i < 8; ++i) sample_put<uint16_t>(w, i, S::at(v, i));
                    *(u4_t*)l = w;
                } else {
                    for (int i = max(0, -x); i < min(8, pl.cols - x); ++i) l[i] = gcp<T>(g)[i];
                }
            }
            __syncthreads();
            // ---- a strip of 8 samples of one row a thread ----
            {
                const int r = tid / SX, k = tid % SX;
                const int y = y0 + r, x = x0 + 8 * k;
                const bool inner = x0 >= R && x0 + TX + R <= pl.cols && y0 >= R && y0 + TY + R <= pl.rows;      // the same for the whole workgroup
                if (inner) {
                    int res[8];
                    filter_strip<R, false>(lds, r, k, x, y, pl.rows, pl.cols, thr, res);
                    typename S::V v = S::zero();
#pragma unroll
                    for (int i = 0; i < 8; ++i) S::put(v, i, (uint32_t)res[i]);
                    *(DEMFI_GLOBAL typename S::V_sample_aligned*)(out + (int64_t)y * pl.pitch + x) = v;
                } else if (y < pl.rows && x < pl.cols) {
                    int res[8];
                    filter_strip<R, true>(lds, r, k, x, y, pl.rows, pl.cols, thr, res);
                    T* g = out + (int64_t)y * pl.pitch + x;
                    if (x + 8 <= pl.cols) {
                        typename S::V v = S::zero();
#pragma unroll
                        for (int i = 0; i < 8; ++i) S::put(v, i, (uint32_t)res[i]);
                        *(DEMFI_GLOBAL typename S::V_sample_aligned*)g = v;
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (x + i < pl.cols) gp<T>(g)[i] = (T)res[i];
                    }
                }
            }
            __syncthreads();                                             // the next tile overwrites the LDS image
        }
    }
}

}  // namespace

extern "C" int demfi_payload_deband(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes, int n, const int64_t* planes,
                                    int n_planes, int sample_bytes, int depth, int thr8, int radius, void* stream)
{
    const char* fn = "demfi_payload_deband";
    if (!src || !dst || !planes) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (!is_depth(depth) || (depth > 8 && sample_bytes == 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: depth=%d with %d bytes per sample (8, 10, 12, 14 or 16; above 8 needs 2 bytes)", fn, depth,
                               sample_bytes);
    if (thr8 < 0 || thr8 > MAX_THR8 || radius < 1 || radius > MAX_RADIUS)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: window thr8=%d (0..%d), radius=%d (1..%d)", fn, thr8, MAX_THR8, radius, MAX_RADIUS);
    if (n_planes < 1 || n_planes > MAX_ENTRIES) return demfi_set_error(DEMFI_ERR_ARG, "%s: %d planes (1..%d)", fn, n_planes, MAX_ENTRIES);
    Planes tab{};
    tab.n = n_planes;
    int64_t extent = 0, most = 1, covered = 0;                           // samples of a payload the table reaches; tiles of its largest plane
    for (int p = 0; p < n_planes; ++p) {
        const int64_t* e = planes + 6 * p;                               // first sample, rows, cols, pitch, x phase, y phase
        if (e[0] < 0 || e[0] > ((int64_t)1 << 40)) return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d starts at sample %lld", fn, p, (long long)e[0]);
        if (e[1] < 1 || e[1] > MAX_SIDE || e[2] < 1 || e[2] > MAX_SIDE)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d is %lld x %lld (1..%d each)", fn, p, (long long)e[1], (long long)e[2], MAX_SIDE);
        if (e[3] < e[2] || e[3] > 4 * (int64_t)MAX_SIDE)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d has a pitch of %lld samples for %lld columns (cols..%d)", fn, p, (long long)e[3],
                                   (long long)e[2], 4 * MAX_SIDE);
        if (e[4] < 0 || e[4] > 7 || e[5] < 0 || e[5] > 7)                 // carried and ignored, but a table is a table
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d has the phases %lld, %lld (0..7)", fn, p, (long long)e[4], (long long)e[5]);
        tab.p[p] = Plane{e[0], e[3], (int)e[1], (int)e[2]};
        extent = max(extent, e[0] + (e[1] - 1) * e[3] + e[2]);
        covered += e[1] * e[2];
        most = max(most, (int64_t)axis_tiles((int)e[2], TX) * axis_tiles((int)e[1], TY));
    }
    if (int st = check_even(fn, sample_bytes, (uintptr_t)src | (uintptr_t)src_stride_bytes | (uintptr_t)dst | (uintptr_t)dst_stride_bytes)) return st;
    const int64_t bytes = extent * sample_bytes;
    if (src_stride_bytes < bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: src_stride=%lld below the %lld bytes of a payload", fn, (long long)src_stride_bytes, (long long)bytes);
    if (int st = check_dst_stride(fn, dst_stride_bytes, bytes)) return st;
    if (n > 0) {                                                         // the taps read what the stage has not written: src and dst apart
        const int64_t far = (INT64_MAX - bytes) / n;                     // n strides and a payload stay within int64
        if (src_stride_bytes > far || dst_stride_bytes > far)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: a stride of %lld / %lld bytes times n=%d leaves the address space", fn,
                                   (long long)src_stride_bytes, (long long)dst_stride_bytes, n);
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((n - 1) * src_stride_bytes + bytes);
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((n - 1) * dst_stride_bytes + bytes);
        if (s0 < d1 && d0 < s1) return demfi_set_error(DEMFI_ERR_ARG, "%s: src and dst overlap (the filter cannot work in place)", fn);
    }
    if (n == 0) return DEMFI_OK;
    // the identity, and samples of a payload that no entry names (none with the tables of deblock.plane_table): the payloads are copied
    if (thr8 == 0 || covered != extent)
        DEMFI_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dst_stride_bytes, src, (size_t)src_stride_bytes, (size_t)bytes, (size_t)n, hipMemcpyDeviceToDevice,
                                         (hipStream_t)stream));
    if (thr8 == 0) return DEMFI_OK;
    const int thr = thr8 << (depth - 8);
    const dim3 grid = rows_grid(most, 1, (int64_t)n * n_planes);
    by_sample(sample_bytes, [&](auto t) {
        by_int<1, MAX_RADIUS>(radius, [&](auto r) {
            hipLaunchKernelGGL((payload_deband_kernel<TAG_TYPE(t), TAG_VALUE(r)>), grid, dim3(NT), 0, (hipStream_t)stream, (const uint8_t*)src,
                               src_stride_bytes, (uint8_t*)dst, dst_stride_bytes, n, tab, thr);
        });
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
