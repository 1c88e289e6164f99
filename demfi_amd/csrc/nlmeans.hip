// Spatial denoising of the Y4M video path in front of the network (demfi_amd/nlmeans.py, --nlmeans): non-local means in exact integers, on
// every plane of every payload as a plane in its own right, OUT OF PLACE (src -> dst: every read is from the plane as it was).  With
// u(x, y) the sample at the clamped position, q(t) = min(|t| >> qshift, 4095) and, for every offset (i, j), |i|, |j| <= R, whose candidate
// (x + i, y + j) lies inside the plane: D = sum over the (2P + 1)^2 patch of q(u(p + a) - u(p + o + a))^2, w = T[min(D >> g, 1023)],
// out = (2 sum(w v) + W) / (2 W) floored, W = sum(w).  The definition is nlmeans.nlmeans_payload_np; this kernel gives the same integers.
// The table T and g come from the host (nlmeans.weight_table): no exponential here.  The phase columns of the plane table are ignored.
//
// Tile: TX x TY = 64 x 32 samples of one plane of one payload.  The tile with a halo of R + P <= 10 goes to LDS as 16-bit samples whatever
// the stored size, out-of-plane positions filled with the clamped sample, so a patch needs no branch: LR x LP = 52 rows x 85 samples =
// 8840 bytes.  The pitch is ODD: a thread's block starts 8 samples (4 dwords) from its neighbour's and 2 rows (85 dwords) from the one
// below, so the 32 lanes of a 16-bit LDS read fall into 32 different banks.  The table sits behind it (2 KiB); it is a kernel argument and
// each workgroup copies it once.
//
// A thread owns a block of 8 x 2 samples and keeps the (8 + 2P) x (2 + 2P) samples its own patches cover in registers.  Per offset (a
// run-time loop: the code is one body per sample type, P and "differences are shifted", all template arguments) it reads the same
// block displaced, forms each squared difference ONCE, slides the horizontal patch sums over a row in registers with compile-time
// indices (no register array is indexed at run time) and adds each row sum into the block rows it belongs to: the redundancy is
// (2 + 2P) / 2, not 2P + 1.  Per candidate sample: a shift and a min for the index, one 16-bit LDS read for the weight, a select for
// "inside the plane", an add into W and one multiply-add into sum(w v).  sum(w v) <= 225 * 256 * 65535 < 2^32 and W <= 57600
// (nlmeans.accumulator_bounds): both unsigned 32-bit at every depth, and the signed numerator of the definition, which does not fit 32
// bits at 16 under every table this entry point takes, is never formed.  The quotient is one unsigned 32-bit division and a comparison
// of the remainder (nlmeans.kernel_quotient).  Measured (profiles/nlmeans.md): 28.0 vector instructions a candidate sample at P = 2 on
// bytes (18.4 at P = 1, 38.4 at P = 3; 16-bit samples pay the clamp: 32.4), about half the vector pipes' issue rate.  Every offset into a
// payload is 64-bit; no atomics; no scratch.
#include "payload_kit.h"

namespace {

constexpr int NT = 128;                 // threads of a workgroup
constexpr int TX = 64, TY = 32;         // a tile: samples x rows
constexpr int BW = 8, BH = 2;           // a thread's block
constexpr int HM = 10;                  // halo columns and rows in LDS: the greatest R + P
constexpr int LW = TX + 2 * HM;         // samples of an LDS row in use
constexpr int LP = LW + 1;              // LDS row pitch in samples: odd
constexpr int LR = TY + 2 * HM;         // LDS rows
constexpr int SX = TX / BW;             // blocks of a tile row
constexpr int KT = 1024;                // entries of the weight table
constexpr int MAX_ENTRIES = 6;          // 3 planes x 2 fields
constexpr int MAX_SIDE = 16384;
constexpr int MAX_PATCH = 3, MAX_SEARCH = 7;
static_assert((TY / BH) * SX == NT, "one thread a block");
static_assert(MAX_PATCH + MAX_SEARCH <= HM && LP % 2 == 1, "the halo holds the widest window; the pitch is odd");

struct Plane {                          // one entry of the plane table (deblock.plane_table)
    int64_t first, pitch;               // first sample in the payload; samples from a row to the next
    int rows, cols;
};
struct Planes {
    int n;
    Plane p[MAX_ENTRIES];
};
struct Weights {                        // the weight table, by value
    uint16_t w[KT];
};

__host__ __device__ inline int axis_tiles(int n, int T) { return (n + T - 1) / T; }

// The block of BW x BH samples at block row rb, block column k of the tile (plane position (x, y)) -> res.  lds: the tile's image; lw: the
// weights.  Samples of the block outside the plane give values nobody stores.
template <typename T, int P, bool SHIFTED>
__device__ __forceinline__ void filter_block(const uint16_t* lds, const uint16_t* lw, int rb, int k, int x, int y, int rows, int cols, int R,
                                             int qshift, int g, uint32_t (&res)[BH][BW])
{
    constexpr int N = 2 * P + 1, AW = BW + 2 * P, AH = BH + 2 * P;
    const uint16_t* a0 = lds + (HM + rb * BH - P) * LP + HM + BW * k - P;          // the sample at (x - P, y - P)
    uint32_t A[AH][AW], W[BH][BW], SV[BH][BW];
#pragma unroll
    for (int rr = 0; rr < AH; ++rr)
#pragma unroll
        for (int cc = 0; cc < AW; ++cc) A[rr][cc] = a0[rr * LP + cc];
#pragma unroll
    for (int o = 0; o < BH; ++o)
#pragma unroll
        for (int kk = 0; kk < BW; ++kk) W[o][kk] = 0u, SV[o][kk] = 0u;
#pragma unroll 1
    for (int j = -R; j <= R; ++j) {
#pragma unroll 1
        for (int i = -R; i <= R; ++i) {
            const uint16_t* b0 = a0 + j * LP + i;                                   // |i|, |j| <= R: inside the halo of R + P
            uint32_t D[BH][BW], V[BH][BW];
#pragma unroll
            for (int o = 0; o < BH; ++o)
#pragma unroll
                for (int kk = 0; kk < BW; ++kk) D[o][kk] = 0u;
#pragma unroll
            for (int rr = 0; rr < AH; ++rr) {
                uint32_t sq[AW];
#pragma unroll
                for (int cc = 0; cc < AW; ++cc) {
                    const uint32_t b = b0[rr * LP + cc];
                    uint32_t q = __builtin_amdgcn_sad_u16(A[rr][cc], b, 0u);        // |a - b|: the high halves are zero
                    if (SHIFTED) q >>= qshift;                                      // depths 14 and 16 only
                    if (sizeof(T) == 2) q = min(q, 4095u);                          // bytes: |a - b| <= 255
                    sq[cc] = __umul24(q, q);
                    if (rr >= P && rr < P + BH && cc >= P && cc < P + BW) V[rr - P][cc - P] = b;       // the candidate itself
                }
                uint32_t h = 0u;
#pragma unroll
                for (int cc = 0; cc < N; ++cc) h += sq[cc];
#pragma unroll
                for (int kk = 0; kk < BW; ++kk) {
                    if (kk > 0) h = h + sq[kk + N - 1] - sq[kk - 1];
#pragma unroll
                    for (int o = 0; o < BH; ++o)
                        if (rr >= o && rr - o < N) D[o][kk] += h;                  // row rr of the block's image is row rr - o of o's patch
                }
            }
#pragma unroll
            for (int o = 0; o < BH; ++o) {
                const bool oky = (unsigned)(y + o + j) < (unsigned)rows;
#pragma unroll
                for (int kk = 0; kk < BW; ++kk) {
                    const bool ok = oky && (unsigned)(x + kk + i) < (unsigned)cols;          // the candidate lies inside the plane
                    const uint32_t w = ok ? (uint32_t)lw[min(D[o][kk] >> g, (uint32_t)(KT - 1))] : 0u;
                    W[o][kk] += w;
                    SV[o][kk] += __umul24(w, V[o][kk]);
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < BH; ++o)
#pragma unroll
        for (int kk = 0; kk < BW; ++kk) {
            const uint32_t den = max(W[o][kk], 1u);                                  // 0 only for a sample outside the plane
            const uint32_t qt = SV[o][kk] / den, rem = SV[o][kk] - qt * den;
            res[o][kk] = qt + (2u * rem >= den ? 1u : 0u);
        }
}

// grid: x = tiles of a plane (strided), y = (payload, table entry) pairs (strided).  T: the stored sample type; P: the patch radius;
// SHIFTED: differences lose low bits (qshift > 0).
template <typename T, int P, bool SHIFTED>
__global__ __launch_bounds__(NT) void payload_nlmeans_kernel(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int n,
                                                             Planes tab, Weights wt, int R, int qshift, int g)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[LR * LP];
    __shared__ __attribute__((aligned(16))) uint16_t lw[KT];
    typedef Strip<T> S;
    const int tid = threadIdx.x, H = R + P;
    for (int u = tid; u < KT; u += NT) lw[u] = wt.w[u];
    const int64_t pairs = (int64_t)n * tab.n;
    for (int64_t pr = blockIdx.y; pr < pairs; pr += gridDim.y) {
        const Plane pl = tab.p[pr % tab.n];
        const T* in = (const T*)(src + (pr / tab.n) * src_stride) + pl.first;
        T* out = (T*)(dst + (pr / tab.n) * dst_stride) + pl.first;
        const int ntx = axis_tiles(pl.cols, TX), nty = axis_tiles(pl.rows, TY);
        for (int t = blockIdx.x; t < ntx * nty; t += gridDim.x) {
            const int x0 = (t % ntx) * TX, y0 = (t / ntx) * TY;             // LDS (r, c) is plane (y0 - HM + r, x0 - HM + c), clamped
            // ---- the tile and a halo of R + P into LDS, the edge replicated ----
            for (int u = tid; u < LR * LW; u += NT) {
                const int r = u / LW, c = u % LW;
                if (r < HM - H || r >= HM + TY + H || c < HM - H || c >= HM + TX + H) continue;                 // beyond the halo of R + P
                const int yy = clamp_row(y0 - HM + r, pl.rows), xx = clamp_row(x0 - HM + c, pl.cols);
                lds[r * LP + c] = (uint16_t)gcp<T>(in)[(int64_t)yy * pl.pitch + xx];
            }
            __syncthreads();
            // ---- a block of 8 x 2 samples a thread ----
            {
                const int rb = tid / SX, k = tid % SX;
                const int y = y0 + BH * rb, x = x0 + BW * k;
                if (y < pl.rows && x < pl.cols) {
                    uint32_t res[BH][BW];
                    filter_block<T, P, SHIFTED>(lds, lw, rb, k, x, y, pl.rows, pl.cols, R, qshift, g, res);
#pragma unroll
                    for (int o = 0; o < BH; ++o) {
                        if (y + o >= pl.rows) continue;
                        T* gl = out + (int64_t)(y + o) * pl.pitch + x;
                        if (x + BW <= pl.cols) {
                            typename S::V v = S::zero();
#pragma unroll
                            for (int kk = 0; kk < BW; ++kk) S::put(v, kk, res[o][kk]);
                            *(DEMFI_GLOBAL typename S::V_sample_aligned*)gl = v;
                        } else {
#pragma unroll
                            for (int kk = 0; kk < BW; ++kk)
                                if (x + kk < pl.cols) gp<T>(gl)[kk] = (T)res[o][kk];
                        }
                    }
                }
            }
            __syncthreads();                                             // the next tile overwrites the LDS image
        }
    }
}

}  // namespace

extern "C" int demfi_payload_nlmeans(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes, int n, const int64_t* planes,
                                     int n_planes, int sample_bytes, int depth, int patch, int search, const uint16_t* table, int shift,
                                     void* stream)
{
    const char* fn = "demfi_payload_nlmeans";
    if (!src || !dst || !planes || !table) return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or table", fn);
    if (n < 0) return demfi_set_error(DEMFI_ERR_ARG, "%s: n=%d", fn, n);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (!is_depth(depth) || (depth > 8 && sample_bytes == 1))
        return demfi_set_error(DEMFI_ERR_ARG, "%s: depth=%d with %d bytes per sample (8, 10, 12, 14 or 16; above 8 needs 2 bytes)", fn, depth,
                               sample_bytes);
    if (patch < 1 || patch > MAX_PATCH || search < 1 || search > MAX_SEARCH || shift < 0 || shift > 31)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: window patch=%d (1..%d), search=%d (1..%d), shift=%d (0..31)", fn, patch, MAX_PATCH, search,
                               MAX_SEARCH, shift);
    Weights wt{};
    for (int k = 0; k < KT; ++k) {                                       // 256 at no distance, never above it, never increasing
        if (table[k] > 256 || (k == 0 ? table[0] != 256 : table[k] > table[k - 1]))
            return demfi_set_error(DEMFI_ERR_ARG, "%s: table[%d]=%d (table[0] = 256, no entry above 256 or above the one before)", fn, k,
                                   (int)table[k]);
        wt.w[k] = table[k];
    }
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
    if (n > 0) {                                                         // the patches read what the stage has not written: src and dst apart
        const int64_t far = (INT64_MAX - bytes) / n;                     // n strides and a payload stay within int64
        if (src_stride_bytes > far || dst_stride_bytes > far)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: a stride of %lld / %lld bytes times n=%d leaves the address space", fn,
                                   (long long)src_stride_bytes, (long long)dst_stride_bytes, n);
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((n - 1) * src_stride_bytes + bytes);
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((n - 1) * dst_stride_bytes + bytes);
        if (s0 < d1 && d0 < s1) return demfi_set_error(DEMFI_ERR_ARG, "%s: src and dst overlap (the filter cannot work in place)", fn);
    }
    if (n == 0) return DEMFI_OK;
    // samples of a payload that no entry names (none with the tables of deblock.plane_table): the payloads are copied first
    if (covered != extent)
        DEMFI_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dst_stride_bytes, src, (size_t)src_stride_bytes, (size_t)bytes, (size_t)n, hipMemcpyDeviceToDevice,
                                         (hipStream_t)stream));
    const int s = depth - 8, qshift = s - min(s, 4);                     // differences at 12 bits of precision at most
    const dim3 grid = rows_grid(most, 1, (int64_t)n * n_planes);
    by_sample(sample_bytes, [&](auto t) {
        by_int<1, MAX_PATCH>(patch, [&](auto p) {
            by_bool(qshift > 0, [&](auto sh) {
                hipLaunchKernelGGL((payload_nlmeans_kernel<TAG_TYPE(t), TAG_VALUE(p), TAG_VALUE(sh)>), grid, dim3(NT), 0, (hipStream_t)stream,
                                   (const uint8_t*)src, src_stride_bytes, (uint8_t*)dst, dst_stride_bytes, n, tab, wt, search, qshift, shift);
            });
        });
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
