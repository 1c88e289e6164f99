// Deringing of the Y4M video path in front of the network (demfi_amd/dering.py, --dering): AV1's constrained directional enhancement filter in
// exact integers, on every plane of every payload as a plane in its own right, OUT OF PLACE (src -> dst: every tap reads the plane as it was).
// A plane whose left Lp columns and top Tp rows were cropped away has a block starting at column x when (x + Lp) % 8 == 0, rows likewise; a
// block finds its direction (8 candidates, the cost of a direction = the weighted squares of its line sums), its variance scales the primary
// strength, and every sample takes 4 primary taps along the direction and 8 secondary taps across it, each through the constraint function,
// clamped to the extremes of what it read.  The definition is dering.dering_payload_np; this kernel gives the same integers.
//
// Tile: TX x TY = 64 x 32 samples = 8 x 4 whole blocks of one plane of one payload; in grid coordinates (gx = x + Lp, gy = y + Tp) tile j of
// an axis is [j T, (j + 1) T), so its borders lie on the block grid and the first and last tile of an axis end at the plane's edge.  The
// tile with a halo goes to LDS as 16-bit samples whatever the stored size: LR x LP = 36 x 80 samples = 5760 bytes (2 halo rows above and
// below; 8 halo columns left and right, of which the taps reach 2, so that every 8-sample strip of the grid is one aligned 16-byte LDS
// word), plus one dword a block (128 bytes): 5888 bytes of LDS.  Strips wholly inside the plane are one packed global load / store at any
// sample address (Strip of payload_kit.h), ragged ones go sample by sample.  Out-of-plane positions are never loaded; a tap there is known
// by its coordinates and skipped, so any stored bits of a 16-bit container are samples.
//
// Pass 1, directions: 8 lanes a block, lane i owns row i and column i of the block (positions clamped into the plane).  A direction's lines
// are i + m (rows) or j + m (columns) for a group index m that is a compile-time function of the position in the row / column, so lane i
// sums line i (and line i + 8) from the groups of lanes i - m through lane shuffles, and the 8 costs are summed over the 8 lanes: no
// register array is indexed by a run-time value.  Lane 0 writes dir, pri and the primary shift (31 - __clz, once a block) as one LDS dword.
// Pass 2, filter: a thread filters the 8 samples of one strip of one row; tap addresses are the centre's LDS address plus six run-time
// offsets (one LDS table lookup each).  int32 throughout (every cost <= 64 * 840 * 128^2 < 2^31); every offset into a payload is 64-bit;
// no atomics.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int TX = 64, TY = 32;         // a tile: samples x rows, whole blocks
constexpr int HX = 8, HY = 2;           // halo columns (2 used; 8 keeps strips aligned) and rows in LDS
constexpr int LP = TX + 2 * HX;         // LDS row pitch in samples
constexpr int LR = TY + 2 * HY;         // LDS rows
constexpr int BX = TX / 8, BY = TY / 8; // blocks of a tile
constexpr int MAX_ENTRIES = 6;          // 3 planes x 2 fields
constexpr int MAX_SIDE = 16384;
static_assert(BX * BY * 8 == NT && TY * BX == NT, "one lane group a block, one thread a strip");

struct Plane {                          // one entry of the plane table (deblock.plane_table)
    int64_t first, pitch;               // first sample in the payload; samples from a row to the next
    int rows, cols, xp, yp;             // size; the phases Lp % 8 and Tp % 8
};
struct Planes {
    int n;
    Plane p[MAX_ENTRIES];
};
struct Rule {                           // dering.strengths and what follows from them
    int P, sh, sec, sec_shift, damp;    // primary strength (8-bit steps), depth - 8, S << sh, max(0, damp - ilog2(sec)), D + sh
};

__host__ __device__ inline int axis_tiles(int n, int ph, int T) { return (ph + n + T - 1) / T; }

// 840 / n for a line of n samples; [0] = 0: no line
__constant__ int LINE_WEIGHT[9] = {0, 840, 420, 280, 210, 168, 140, 120, 105};
// dy and dx of direction k at distances 1 and 2 (dering.TAPS)
__constant__ int TAP_DY[8][2] = {{-1, -2}, {0, -1}, {0, 0}, {0, 1}, {1, 2}, {1, 2}, {1, 2}, {1, 2}};
__constant__ int TAP_DX[8][2] = {{1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}, {0, 1}, {0, 0}, {0, -1}};

// Lane i (of 8 consecutive lanes) holds the groups g[0 .. G) of GS samples each that belong to the lines i + m: the cost of the direction,
// summed over the 8 lanes' lines.  Lane i sums line i from the lanes i - m >= 0 and line i + 8 from the lanes i - m + 8.
template <int G, int GS> __device__ __forceinline__ int skew_cost(const int (&g)[G], int i, int lane)
{
    int a = g[0], b = 0;
#pragma unroll
    for (int m = 1; m < G; ++m) {
        const int v = __shfl(g[m], (lane & ~7) | ((i - m) & 7));
        a += i >= m ? v : 0;
        b += i >= m ? 0 : v;
    }
    const int na = min(i + 1, G), nb = max(G - 1 - i, 0);
    return LINE_WEIGHT[GS * na] * a * a + LINE_WEIGHT[GS * nb] * b * b;
}
__device__ __forceinline__ int sum8(int v)
{
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v + __shfl_xor(v, 4);
}

__device__ __forceinline__ int constrain(int diff, int thr, int shift)
{
    const int ad = abs(diff), m = min(ad, max(0, thr - (ad >> shift)));     // thr == 0 gives 0
    return diff < 0 ? -m : m;
}

// grid: x = tiles of a plane (strided), y = (payload, table entry) pairs (strided).  T: the stored sample type.
template <typename T>
__global__ __launch_bounds__(NT) void payload_dering_kernel(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int n,
                                                            Planes tab, Rule rule)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[LR * LP];
    __shared__ int blk[BX * BY];                                         // dir | primary shift << 3 | pri << 8
    typedef Strip<T> S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t pairs = (int64_t)n * tab.n;
    for (int64_t pr = blockIdx.y; pr < pairs; pr += gridDim.y) {
        const Plane pl = tab.p[pr % tab.n];
        const T* in = (const T*)(src + (pr / tab.n) * src_stride) + pl.first;
        T* out = (T*)(dst + (pr / tab.n) * dst_stride) + pl.first;
        const int ntx = axis_tiles(pl.cols, pl.xp, TX), nty = axis_tiles(pl.rows, pl.yp, TY);
        for (int t = blockIdx.x; t < ntx * nty; t += gridDim.x) {
            // the tile's corner in plane coordinates (may lie up to 7 in front of the plane); LDS (r, c) is plane (y0 - HY + r, x0 - HX + c)
            const int x0 = (t % ntx) * TX - pl.xp, y0 = (t / ntx) * TY - pl.yp;
            // ---- the tile and its halo into LDS: strips of 8 on the grid ----
            for (int u = tid; u < LR * (LP / 8); u += NT) {
                const int r = u / (LP / 8), k = u % (LP / 8);
                const int y = y0 - HY + r, x = x0 - HX + 8 * k;
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
            // ---- pass 1: direction and primary strength of every block; 8 lanes a block ----
            {
                const int b = tid >> 3, i = tid & 7;
                const int bx0 = x0 + 8 * (b % BX), by0 = y0 + 8 * (b / BX);     // the block's corner in plane coordinates
                const int yc = clampi(by0 + i, 0, pl.rows - 1) - (y0 - HY), xc = clampi(bx0 + i, 0, pl.cols - 1) - (x0 - HX);
                // a block slot behind the plane's end reads the tile's last in-plane samples: initialised LDS, a result nobody uses
                const int ylim = min(pl.rows - 1, y0 + TY - 1) - (y0 - HY), xlim = min(pl.cols - 1, x0 + TX - 1) - (x0 - HX);
                int row[8], col[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int xj = min(clampi(bx0 + j, 0, pl.cols - 1) - (x0 - HX), xlim), yj = min(clampi(by0 + j, 0, pl.rows - 1) - (y0 - HY), ylim);
                    row[j] = min((int)lds[min(yc, ylim) * LP + xj] >> rule.sh, 255) - 128;
                    col[j] = min((int)lds[yj * LP + min(xc, xlim)] >> rule.sh, 255) - 128;
                }
                int cost[8];
                {
                    int rev[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) rev[j] = row[7 - j];
                    cost[0] = skew_cost<8, 1>(row, i, lane);               // i + j
                    cost[4] = skew_cost<8, 1>(rev, i, lane);               // i + (7 - j)
                    const int rp[4] = {row[0] + row[1], row[2] + row[3], row[4] + row[5], row[6] + row[7]};
                    const int rq[4] = {rp[3], rp[2], rp[1], rp[0]};
                    cost[1] = skew_cost<4, 2>(rp, i, lane);                // i + j / 2
                    cost[3] = skew_cost<4, 2>(rq, i, lane);                // i + (3 - j / 2)
                    const int rs[1] = {rp[0] + rp[1] + rp[2] + rp[3]};
                    cost[2] = skew_cost<1, 8>(rs, i, lane);                // i
                    const int cp[4] = {col[0] + col[1], col[2] + col[3], col[4] + col[5], col[6] + col[7]};
                    const int cq[4] = {cp[3], cp[2], cp[1], cp[0]};
                    cost[7] = skew_cost<4, 2>(cp, i, lane);                // j + i / 2
                    cost[5] = skew_cost<4, 2>(cq, i, lane);                // j + (3 - i / 2)
                    const int cs[1] = {cp[0] + cp[1] + cp[2] + cp[3]};
                    cost[6] = skew_cost<1, 8>(cs, i, lane);                // j
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) cost[k] = sum8(cost[k]);
                int dir = 0, best = cost[0], opp = cost[4];
#pragma unroll
                for (int k = 1; k < 8; ++k) {
                    const bool more = cost[k] > best;                    // the first of the greatest
                    dir = more ? k : dir, opp = more ? cost[(k + 4) & 7] : opp, best = more ? cost[k] : best;
                }
                const int var = (best - opp) >> 10;
                const int e = var >> 6 ? min(31 - __clz(var >> 6), 12) : 0;
                const int pri = (var ? (rule.P * (4 + e) + 8) >> 4 : 0) << rule.sh;
                const int shift = pri ? max(0, rule.damp - (31 - __clz(pri))) : 0;
                if (i == 0) blk[b] = dir | shift << 3 | pri << 8;
            }
            __syncthreads();
            // ---- pass 2: a strip of 8 samples of one row a thread ----
            {
                const int r = tid / BX, k = tid % BX;                     // row and strip of the tile
                const int y = y0 + r, x = x0 + 8 * k;
                if (y >= 0 && y < pl.rows && x + 8 > 0 && x < pl.cols) {
                    const int info = blk[(r >> 3) * BX + k];
                    const int dir = info & 7, pshift = (info >> 3) & 31, pri = info >> 8;
                    const int d1 = (dir + 2) & 7, d2 = (dir + 6) & 7;
                    // the six offsets: primary, secondary one, secondary two, each at distances 1 and 2
                    const int dy0 = TAP_DY[dir][0], dx0 = TAP_DX[dir][0], dy1 = TAP_DY[dir][1], dx1 = TAP_DX[dir][1];
                    const int dy2 = TAP_DY[d1][0], dx2 = TAP_DX[d1][0], dy3 = TAP_DY[d1][1], dx3 = TAP_DX[d1][1];
                    const int dy4 = TAP_DY[d2][0], dx4 = TAP_DX[d2][0], dy5 = TAP_DY[d2][1], dx5 = TAP_DX[d2][1];
                    const uint16_t* centre = lds + (HY + r) * LP + HX + 8 * k;
                    const u4_t cw = *(const u4_t*)centre;
                    int res[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int c = (int)sample_at<uint16_t>(cw, i), xi = x + i;
                        int s = 0, lo = c, hi = c;
                        auto tap = [&](int dy, int dx, int w, int thr, int shift) {
                            const bool ok = (unsigned)(y + dy) < (unsigned)pl.rows && (unsigned)(xi + dx) < (unsigned)pl.cols;
                            const int v = ok ? (int)centre[i + dy * LP + dx] : c;     // the halo keeps the address inside the array
                            s += w * constrain(v - c, thr, shift);
                            lo = min(lo, v), hi = max(hi, v);
                        };
                        tap(dy0, dx0, 4, pri, pshift), tap(-dy0, -dx0, 4, pri, pshift);
                        tap(dy1, dx1, 2, pri, pshift), tap(-dy1, -dx1, 2, pri, pshift);
                        tap(dy2, dx2, 2, rule.sec, rule.sec_shift), tap(-dy2, -dx2, 2, rule.sec, rule.sec_shift);
                        tap(dy3, dx3, 1, rule.sec, rule.sec_shift), tap(-dy3, -dx3, 1, rule.sec, rule.sec_shift);
                        tap(dy4, dx4, 2, rule.sec, rule.sec_shift), tap(-dy4, -dx4, 2, rule.sec, rule.sec_shift);
                        tap(dy5, dx5, 1, rule.sec, rule.sec_shift), tap(-dy5, -dx5, 1, rule.sec, rule.sec_shift);
                        res[i] = clampi(c + ((8 + s - (s < 0)) >> 4), lo, hi);
                    }
                    T* g = out + (int64_t)y * pl.pitch + x;
                    if (x >= 0 && x + 8 <= pl.cols) {
                        typename S::V v = S::zero();
#pragma unroll
                        for (int i = 0; i < 8; ++i) S::put(v, i, (uint32_t)res[i]);
                        *(DEMFI_GLOBAL typename S::V_sample_aligned*)g = v;
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (x + i >= 0 && x + i < pl.cols) gp<T>(g)[i] = (T)res[i];
                    }
                }
            }
            __syncthreads();                                             // the next tile overwrites the LDS image
        }
    }
}

inline int ilog2_host(int v) { return 31 - __builtin_clz((unsigned)v); }

}  // namespace

extern "C" int demfi_payload_dering(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes, int n, const int64_t* planes,
                                    int n_planes, int sample_bytes, int depth, int pri, int sec, int damping, void* stream)
{
    const char* fn = "demfi_payload_dering";
    if (!src || !dst || !planes) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (!is_depth(depth) || (depth > 8 && sample_bytes == 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: depth=%d with %d bytes per sample (8, 10, 12, 14 or 16; above 8 needs 2 bytes)", fn, depth,
                               sample_bytes);
    if (pri < 0 || pri > 15 || sec < 0 || sec > 4 || damping < 3 || damping > 6)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: strengths pri=%d (0..15), sec=%d (0..4), damping=%d (3..6)", fn, pri, sec, damping);
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
        if (e[4] < 0 || e[4] > 7 || e[5] < 0 || e[5] > 7)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: plane %d has the phases %lld, %lld (0..7)", fn, p, (long long)e[4], (long long)e[5]);
        tab.p[p] = Plane{e[0], e[3], (int)e[1], (int)e[2], (int)e[4], (int)e[5]};
        extent = max(extent, e[0] + (e[1] - 1) * e[3] + e[2]);
        covered += e[1] * e[2];
        most = max(most, (int64_t)axis_tiles((int)e[2], (int)e[4], TX) * axis_tiles((int)e[1], (int)e[5], TY));
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
    // samples of a payload that no entry names (none with the tables of deblock.plane_table) are copied ahead of the launch
    if (covered != extent)
        DEMFI_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dst_stride_bytes, src, (size_t)src_stride_bytes, (size_t)bytes, (size_t)n, hipMemcpyDeviceToDevice,
                                         (hipStream_t)stream));
    const int sh = depth - 8, sec_s = sec << sh, damp = damping + sh;
    const Rule rule{pri, sh, sec_s, sec_s ? max(0, damp - ilog2_host(sec_s)) : 0, damp};
    const dim3 grid = rows_grid(most, 1, (int64_t)n * n_planes);
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL((payload_dering_kernel<TAG_TYPE(t)>), grid, dim3(NT), 0, (hipStream_t)stream, (const uint8_t*)src, src_stride_bytes,
                           (uint8_t*)dst, dst_stride_bytes, n, tab, rule);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
