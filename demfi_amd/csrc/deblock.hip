// Deblocking of the Y4M video path in front of the network (demfi_amd/deblock.py, --deblock): H.264's intra-edge (bS = 4) luma filter as a post
// filter on a fixed 8-sample grid, on every plane of every payload as a plane in its own right, IN PLACE.  A plane whose left Lp columns and
// top Tp rows were cropped away has a vertical edge at column x when (x + Lp) % 8 == 0 and 4 <= x <= cols - 4, rows likewise; one line
// p3 p2 p1 p0 | q0 q1 q2 q3 across an edge is filtered from its own values, all vertical edges first, then all horizontal edges on that
// result.  The definition is deblock.deblock_payload_np; this kernel gives the same integers.
//
// Edges are 8 apart, each reads +-4 and writes +-3: both passes of the cell [x-4, x+4) x [y-4, y+4) around a grid crossing touch only that cell
// (and the plane's remainders in line with it).  A workgroup owns a tile whose borders lie on cell borders only, x + Lp == 4 and y + Tp == 4
// (mod 8); the first tile of an axis starts at the plane's edge and the last one ends there.  So a tile needs no halo and reads and writes
// nothing another workgroup touches, which is what makes the work in place free of races without atomics or a second buffer.
//
// The tile goes to LDS as 16-bit samples whatever the stored size, shifted so that cell borders fall on multiples of 8 LDS columns and rows:
// a line across a vertical edge is then ONE aligned 16-byte LDS word (ds_read_b128 / ds_write_b128, consecutive lanes consecutive words),
// and the pass over the horizontal edges takes two columns a thread, eight dword reads down the rows and six dword writes (consecutive
// lanes consecutive dwords of a row: no bank is met twice).  Global rows are cut into 16-byte chunks at the LDS word boundaries: a whole
// chunk is one 16-byte load / store at whatever address the tile starts (the sample-aligned vector types of payload_kit.h), a chunk cut
// short by the tile's ragged ends goes sample by sample, and a tile stores only its own samples.  Every offset into a payload is 64-bit.
#include "payload_kit.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int TX = 128, TY = 32;        // a tile between its borders: samples x rows; the first tile of an axis has up to 7 more
constexpr int LP = TX + 16;             // LDS row pitch in samples: the shift (<= 7) + the first tile (<= TX + 7), a multiple of 16
constexpr int LR = TY + 8;              // LDS rows: the shift + the first tile's rows
constexpr int MAX_ENTRIES = 6;          // 3 planes x 2 fields
constexpr int MAX_SIDE = 16384;

struct Plane {                          // one entry of the plane table (deblock.plane_table)
    int64_t first, pitch;               // first sample in the payload; samples from a row to the next
    int rows, cols, xp, yp;             // size; the phases Lp % 8 and Tp % 8
};
struct Planes {
    int n;
    Plane p[MAX_ENTRIES];
};

// the first cell border of an axis of phase ph: the least x >= 0 with (x + ph) % 8 == 4
__host__ __device__ inline int first_border(int ph) { return (12 - ph) & 7; }
// tiles of an axis of n samples: tile 0 is [0, b0 + T), tile j >= 1 [b0 + j T, b0 + (j + 1) T), the last one ends at n
__host__ __device__ inline int axis_tiles(int n, int ph, int T)
{
    const int b0 = first_border(ph);
    return n <= b0 + T ? 1 : 1 + (n - b0 - 1) / T;
}
struct Span { int lo, hi, shift; };     // [lo, hi) of the axis; sample lo sits at LDS position shift, so cell borders sit at multiples of 8
__device__ __forceinline__ Span axis_span(int j, int nt, int n, int ph, int T)
{
    const int b0 = first_border(ph);
    return Span{j ? b0 + j * T : 0, j == nt - 1 ? n : b0 + (j + 1) * T, j ? 0 : (8 - b0) & 7};
}

// the rule on one line v = p3 p2 p1 p0 q0 q1 q2 q3; sums stay below 2^20
__device__ __forceinline__ void filter_line(int (&v)[8], int a, int b, int s)
{
    const int p3 = v[0], p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    const int d = abs(p0 - q0);
    const bool on = d < a && abs(p1 - p0) < b && abs(q1 - q0) < b;
    const bool ps = on && d < s && abs(p2 - p0) < b, qs = on && d < s && abs(q2 - q0) < b;
    v[3] = ps ? (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3 : on ? (2 * p1 + p0 + q1 + 2) >> 2 : p0;
    v[2] = ps ? (p2 + p1 + p0 + q0 + 2) >> 2 : p1;
    v[1] = ps ? (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3 : p2;
    v[4] = qs ? (q2 + 2 * q1 + 2 * q0 + 2 * p0 + p1 + 4) >> 3 : on ? (2 * q1 + q0 + p1 + 2) >> 2 : q0;
    v[5] = qs ? (q2 + q1 + q0 + p0 + 2) >> 2 : q1;
    v[6] = qs ? (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3 : q2;
}

template <typename T> struct Chunk {    // the 16 bytes of a global chunk <-> N = 16 / sizeof(T) 16-bit samples in LDS
    typedef typename std::conditional<sizeof(T) == 1, u4_a1, u4_a2>::type V;     // at any sample address
    static constexpr int N = Samples<T>::N;
    static __device__ __forceinline__ void to_lds(const T* g, uint16_t* l)
    {
        const u4_t v = *(const DEMFI_GLOBAL V*)g;
        if constexpr (sizeof(T) == 2) {
            *(u4_t*)l = v;
        } else {
            u4_t w[2] = {u4_t(0u), u4_t(0u)};
#pragma unroll
            for (int i = 0; i < 16; ++i) sample_put<uint16_t>(w[i / 8], i % 8, sample_at<uint8_t>(v, i));
            ((u4_t*)l)[0] = w[0], ((u4_t*)l)[1] = w[1];
        }
    }
    static __device__ __forceinline__ void to_global(const uint16_t* l, T* g)
    {
        u4_t v;
        if constexpr (sizeof(T) == 2) {
            v = *(const u4_t*)l;
        } else {
            const u4_t w[2] = {((const u4_t*)l)[0], ((const u4_t*)l)[1]};
            v = u4_t(0u);
#pragma unroll
            for (int i = 0; i < 16; ++i) sample_put<uint8_t>(v, i, sample_at<uint16_t>(w[i / 8], i % 8));
        }
        *(DEMFI_GLOBAL V*)g = v;
    }
};

// grid: x = tiles of a plane (strided), y = (payload, table entry) pairs (strided).  T: the stored sample type.
template <typename T>
__global__ __launch_bounds__(NT) void payload_deblock_kernel(uint8_t* base, int64_t stride, int n, Planes tab, int a, int b, int s)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[LR * LP];
    constexpr int N = Chunk<T>::N;
    const int64_t pairs = (int64_t)n * tab.n;
    for (int64_t pr = blockIdx.y; pr < pairs; pr += gridDim.y) {
        const Plane pl = tab.p[pr % tab.n];
        T* plane = (T*)(base + (pr / tab.n) * stride) + pl.first;
        const int ntx = axis_tiles(pl.cols, pl.xp, TX), nty = axis_tiles(pl.rows, pl.yp, TY);
        for (int t = blockIdx.x; t < ntx * nty; t += gridDim.x) {
            const Span X = axis_span(t % ntx, ntx, pl.cols, pl.xp, TX), Y = axis_span(t / ntx, nty, pl.rows, pl.yp, TY);
            const int tw = X.hi - X.lo, th = Y.hi - Y.lo;                // LDS columns [X.shift, X.shift + tw), rows [Y.shift, Y.shift + th)
            const int chunks = (X.shift + tw + N - 1) / N;
            T* corner = plane + (int64_t)Y.lo * pl.pitch + X.lo;
            // ---- the tile into LDS ----
            for (int u = threadIdx.x; u < th * chunks; u += NT) {
                const int r = u / chunks, k = u % chunks;
                const int lo = max(k * N, X.shift), hi = min(k * N + N, X.shift + tw);
                const T* g = corner + (int64_t)r * pl.pitch + (lo - X.shift);
                uint16_t* l = lds + (Y.shift + r) * LP + lo;
                if (hi - lo == N) {
                    Chunk<T>::to_lds(g, l);
                } else {
                    for (int i = 0; i < hi - lo; ++i) l[i] = gcp<T>(g)[i];
                }
            }
            __syncthreads();
            // ---- vertical edges: every whole line [8 m, 8 m + 8) of every row ----
            {
                const int m0 = (X.shift + 7) / 8, nl = (X.shift + tw) / 8 - m0;
                for (int u = threadIdx.x; u < th * nl; u += NT) {
                    u4_t* l = (u4_t*)(lds + (Y.shift + u / nl) * LP + 8 * (m0 + u % nl));
                    const u4_t w = *l;
                    int v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = (int)sample_at<uint16_t>(w, i);
                    filter_line(v, a, b, s);
                    u4_t o = u4_t(0u);
#pragma unroll
                    for (int i = 0; i < 8; ++i) sample_put<uint16_t>(o, i, (uint32_t)v[i]);
                    *l = o;
                }
            }
            __syncthreads();
            // ---- horizontal edges: every whole line of rows [8 m, 8 m + 8), two columns a thread ----
            {
                const int m0 = (Y.shift + 7) / 8, nl = (Y.shift + th) / 8 - m0;
                const int c0 = X.shift / 2, nc = (X.shift + tw + 1) / 2 - c0;
                for (int u = threadIdx.x; u < nl * nc; u += NT) {
                    uint32_t* l = (uint32_t*)(lds + 8 * (m0 + u / nc) * LP) + c0 + u % nc;
                    uint32_t w[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = l[i * (LP / 2)];
                    int lo[8], hi[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) lo[i] = (int)(w[i] & 0xffffu), hi[i] = (int)(w[i] >> 16);
                    filter_line(lo, a, b, s);
                    filter_line(hi, a, b, s);
#pragma unroll
                    for (int i = 1; i < 7; ++i) l[i * (LP / 2)] = (uint32_t)lo[i] | ((uint32_t)hi[i] << 16);
                }
            }
            __syncthreads();
            // ---- the tile's own samples back ----
            for (int u = threadIdx.x; u < th * chunks; u += NT) {
                const int r = u / chunks, k = u % chunks;
                const int lo = max(k * N, X.shift), hi = min(k * N + N, X.shift + tw);
                T* g = corner + (int64_t)r * pl.pitch + (lo - X.shift);
                const uint16_t* l = lds + (Y.shift + r) * LP + lo;
                if (hi - lo == N) {
                    Chunk<T>::to_global(l, g);
                } else {
                    for (int i = 0; i < hi - lo; ++i) gp<T>(g)[i] = (T)l[i];
                }
            }
            __syncthreads();                                             // the next tile overwrites the LDS image
        }
    }
}

}  // namespace

extern "C" int demfi_payload_deblock(void* payloads, int64_t stride_bytes, int n, const int64_t* planes, int n_planes, int sample_bytes, int thr_a,
                                     int thr_b, int thr_s, void* stream)
{
    const char* fn = "demfi_payload_deblock";
    if (!payloads || !planes) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer", fn);
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (n_planes < 1 || n_planes > MAX_ENTRIES) return demfi_set_error(DEMFI_ERR_ARG, "%s: %d planes (1..%d)", fn, n_planes, MAX_ENTRIES);
    const int peak = sample_bytes == 1 ? 255 : 65535;
    if (thr_b < 0 || thr_a < thr_b || thr_a > peak || thr_s < 0 || thr_s > peak)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: thresholds a=%d, b=%d, s=%d need 0 <= b <= a <= %d and 0 <= s <= %d", fn, thr_a, thr_b, thr_s, peak,
                               peak);
    Planes tab{};
    tab.n = n_planes;
    int64_t extent = 0, most = 1;                                        // samples of a payload the table reaches; tiles of its largest plane
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
        most = max(most, (int64_t)axis_tiles((int)e[2], (int)e[4], TX) * axis_tiles((int)e[1], (int)e[5], TY));
    }
    if (int st = check_even(fn, sample_bytes, (uintptr_t)payloads | (uintptr_t)stride_bytes)) return st;
    if (int st = check_dst_stride(fn, stride_bytes, extent * sample_bytes)) return st;
    if (n == 0) return DEMFI_OK;
    const dim3 grid = rows_grid(most, 1, (int64_t)n * n_planes);
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL((payload_deblock_kernel<TAG_TYPE(t)>), grid, dim3(NT), 0, (hipStream_t)stream, (uint8_t*)payloads, stride_bytes, n, tab,
                           thr_a, thr_b, thr_s);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
