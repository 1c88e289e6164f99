// Interlaced input of the Y4M video path (demfi_amd/deint.py, --deinterlace): the bob.  A payload of h rows holds two fields, the
// even rows and the odd rows of every plane; one field is kept and the rows of the other are rebuilt from it, so the payload
// becomes a progressive frame at that field's time instant.  The definition is deint.bob_plane_np; this kernel gives the same
// samples.
//
// A missing row y with both neighbours a = row y-1 and b = row y+1 inside the plane is the five-direction edge-directed line
// average: score(j) = sum over k = -1, 0, 1 of |a[x+k+j] - b[x+k-j]| and pred(j) = (a[x+j] + b[x-j] + 1) >> 1, column indices
// clamped to the plane; start from best = score(0) - 1, out = pred(0); j = -1 is taken when score(-1) < best and only then is
// j = -2 tried; then j = +1 against the running best and, if taken, j = +2.  A missing row with one neighbour copies it, a plane
// without a kept row (one row, odd rows kept) stays as it is.  Integers throughout.
//
// The work is done IN PLACE: a lane reads only kept rows and writes only missing rows, so no lane reads what another writes and
// there is nothing to order.  One lane owns a strip of SX = 8 samples of one missing row and needs samples x0-3 .. x0+10 of the
// rows above and below: its own strip and those of its two neighbours, three row reads through load_n each (8- or 16-byte
// words where the address allows it, sample by sample in rows of odd-width planes, which start at any alignment).  Consecutive
// lanes own consecutive strips of a row, so a wave reads and writes contiguous runs.  All planes of all payloads go in one
// launch: lanes run over the missing rows of Y, then Cb, then Cr, payloads along grid y.  Which rows are missing depends on the
// payload (bit i of odd_mask), so every plane gets lanes for ceil(rows / 2) rows and the lanes of a row that does not exist idle.
//
// The motion-adaptive mode (--deinterlace-mode adaptive, demfi_yuv_deint_adaptive; the definition is deint.adaptive_plane_np) keeps
// that layout, fields along grid y, and clamps the bob's value sp of a missing row y to [d - diff, d + diff] around the temporal
// average d of the fields before and after (yadif's rule with the spatial check, integers throughout).  Besides the two halo rows of
// its own field a lane reads ten rows without a halo, one load_n word each where the address allows it: rows y, y-2, y+2 of P1 =
// field f-1 and N1 = field f+1, rows y-1, y+1 of P2 = field f-2 and N2 = field f+2.  Field g is read out of the payload at
// offsets[5 i + 2 + (g - f)], the copy that belongs to field g.
// THE HAZARD RULE: a lane reads only rows that are KEPT rows of the payload it reads them from (rows of parity 1-q of the payloads
// of f-1 and f+1, rows of parity q of those of f-2, f and f+2), and it writes only MISSING rows of its own payload.  Kept rows are
// never written by any launch, so a neighbouring payload may already have been rebuilt, or be rebuilt by this very launch or a
// concurrent one: what a lane reads of it is the same either way.  In particular the other field of the same source payload is not
// read out of the payload being rewritten (its rows y-2 and y+2 are other lanes' output there) but out of that other field's own
// copy.  So the work stays in place and nothing needs ordering inside a launch or between the launches of neighbouring fields.
// A field absent at an end of the stream (offset -1) is replaced by its partner on the other side in time; with P1 and N1 both
// absent the lane stores the bob's value, with P2 and N2 both absent their two terms are dropped.
#include "yuv_common.h"

namespace {

constexpr int HALO = 3;                 // samples needed beside a strip: |k + j| <= 3 for k = -1 .. 1, j = -2 .. 2
constexpr int NA = SX + 2 * HALO;       // x0-3 .. x0+10

// v[t] = row[clamp(x0 - HALO + t, 0, w-1)], t = 0 .. NA-1
template <typename T> __device__ __forceinline__ void load_halo(const T* row, int x0, int w, int* v)
{
    int t[SX];
    load_n<T, SX>(row, x0, w, v + HALO);
    if (x0 >= SX) {
        load_n<T, SX>(row, x0 - SX, w, t);
#pragma unroll
        for (int i = 0; i < HALO; ++i) v[i] = t[SX - HALO + i];
    } else {                            // x0 == 0: the left edge repeats
        const int e = (int)gcp<T>(row)[0];
#pragma unroll
        for (int i = 0; i < HALO; ++i) v[i] = e;
    }
    if (x0 + SX < w) {
        load_n<T, SX>(row, x0 + SX, w, t);
#pragma unroll
        for (int i = 0; i < HALO; ++i) v[HALO + SX + i] = t[i];
    } else {                            // the right edge repeats
        const int e = (int)gcp<T>(row)[w - 1];
#pragma unroll
        for (int i = 0; i < HALO; ++i) v[HALO + SX + i] = e;
    }
}

__device__ __forceinline__ int absdiff(int a, int b) { return a > b ? a - b : b - a; }

// the SX samples of a missing row between a and b (load_halo of the rows above and below)
__device__ __forceinline__ void edge_average(const int* a, const int* b, int* out)
{
    // d[j+2][t] = |a[x+j] - b[x-j]| at x = x0 - 1 + t, t = 0 .. SX+1
    int d[5][SX + 2];
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int t = 0; t < SX + 2; ++t) d[j + 2][t] = absdiff(a[t + j + 2], b[t - j + 2]);
#pragma unroll
    for (int i = 0; i < SX; ++i) {
        int sc[5], pr[5];
#pragma unroll
        for (int j = -2; j <= 2; ++j) {
            sc[j + 2] = d[j + 2][i] + d[j + 2][i + 1] + d[j + 2][i + 2];
            pr[j + 2] = (a[i + j + HALO] + b[i - j + HALO] + 1) >> 1;
        }
        int best = sc[2] - 1, o = pr[2];
        const bool l1 = sc[1] < best;
        best = l1 ? sc[1] : best;
        o = l1 ? pr[1] : o;
        const bool l2 = l1 && sc[0] < best;
        best = l2 ? sc[0] : best;
        o = l2 ? pr[0] : o;
        const bool r1 = sc[3] < best;
        best = r1 ? sc[3] : best;
        o = r1 ? pr[3] : o;
        const bool r2 = r1 && sc[4] < best;
        o = r2 ? pr[4] : o;
        out[i] = o;
    }
}

// grid: x = lanes over (plane, missing row, strip), y = payloads.  base is read and written: no __restrict__.
template <typename T>
__global__ __launch_bounds__(NT) void bob_kernel(uint8_t* base, int64_t stride_bytes, int h, int w, int ch, int cw, uint64_t odd_mask)
{
    const int sy = (w + SX - 1) / SX, sc = (cw + SX - 1) / SX;           // strips of a luma / chroma row
    const int64_t ly = (int64_t)((h + 1) / 2) * sy, lc = (int64_t)((ch + 1) / 2) * sc;
    int64_t l = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (l >= ly + 2 * lc) return;
    int rows = h, cols = w, strips = sy;
    int64_t first = 0;                                                   // the plane's first sample in the payload
    if (l >= ly) {
        l -= ly;
        rows = ch, cols = cw, strips = sc;
        first = (int64_t)h * w;
        if (l >= lc) {
            l -= lc;
            first += (int64_t)ch * cw;
        }
    }
    const int q = (int)((odd_mask >> blockIdx.y) & 1);                   // parity of the rows kept
    const int y = 2 * (int)(l / strips) + 1 - q, x0 = (int)(l % strips) * SX;
    if (y >= rows) return;
    const bool up = y >= 1, dn = y + 1 < rows;
    if (!up && !dn) return;                                              // one row and it is not kept: the plane stays
    T* plane = (T*)(base + (int64_t)blockIdx.y * stride_bytes) + first;
    T* dst = plane + (int64_t)y * cols + x0;
    const int n = min(SX, cols - x0);
    int o[SX];
    if (up && dn) {
        int a[NA], b[NA];
        load_halo<T>(plane + (int64_t)(y - 1) * cols, x0, cols, a);
        load_halo<T>(plane + (int64_t)(y + 1) * cols, x0, cols, b);
        edge_average(a, b, o);
    } else {
        load_n<T, SX>(plane + (int64_t)(up ? y - 1 : y + 1) * cols, x0, cols, o);
    }
    store_n<T, SX>(dst, o, n);
}

// grid: x = lanes over (plane, missing row, strip), y = fields.  offs: five byte offsets per field from base, the payloads that hold
// fields f-2 .. f+2 (-1: absent).  base is read and written: no __restrict__.
template <typename T>
__global__ __launch_bounds__(NT) void adaptive_kernel(uint8_t* base, const int64_t* offs, int h, int w, int ch, int cw, uint64_t odd_mask)
{
    const int sy = (w + SX - 1) / SX, sc = (cw + SX - 1) / SX;
    const int64_t ly = (int64_t)((h + 1) / 2) * sy, lc = (int64_t)((ch + 1) / 2) * sc;
    int64_t l = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (l >= ly + 2 * lc) return;
    int rows = h, cols = w, strips = sy;
    int64_t first = 0;
    if (l >= ly) {
        l -= ly;
        rows = ch, cols = cw, strips = sc;
        first = (int64_t)h * w;
        if (l >= lc) {
            l -= lc;
            first += (int64_t)ch * cw;
        }
    }
    const int q = (int)((odd_mask >> blockIdx.y) & 1);
    const int y = 2 * (int)(l / strips) + 1 - q, x0 = (int)(l % strips) * SX;
    if (y >= rows) return;
    const bool up = y >= 1, dn = y + 1 < rows;
    if (!up && !dn) return;
    const int64_t* o = offs + 5 * (int64_t)blockIdx.y;
    const int64_t oc = o[2];
    if (oc < 0) return;                                                  // refused by the host check; never written
    T* plane = (T*)(base + oc) + first;
    T* dst = plane + (int64_t)y * cols + x0;
    const int n = min(SX, cols - x0);
    int sp[SX];
    if (!(up && dn)) {
        load_n<T, SX>(plane + (int64_t)(up ? y - 1 : y + 1) * cols, x0, cols, sp);
        store_n<T, SX>(dst, sp, n);
        return;
    }
    int c[SX], e[SX];
    {
        int a[NA], b[NA];
        load_halo<T>(plane + (int64_t)(y - 1) * cols, x0, cols, a);
        load_halo<T>(plane + (int64_t)(y + 1) * cols, x0, cols, b);
        edge_average(a, b, sp);
#pragma unroll
        for (int i = 0; i < SX; ++i) c[i] = a[HALO + i], e[i] = b[HALO + i];
    }
    const int64_t o1 = o[1] >= 0 ? o[1] : o[3], o3 = o[3] >= 0 ? o[3] : o[1];
    const int64_t o0 = o[0] >= 0 ? o[0] : o[4], o4 = o[4] >= 0 ? o[4] : o[0];
    if (o1 < 0) {                                                        // no field before or after: the bob's value
        store_n<T, SX>(dst, sp, n);
        return;
    }
    const T* p1 = (const T*)(base + o1) + first;
    const T* n1 = (const T*)(base + o3) + first;
    int d[SX], diff[SX], u[SX], v[SX];
    load_n<T, SX>(p1 + (int64_t)y * cols, x0, cols, u);
    load_n<T, SX>(n1 + (int64_t)y * cols, x0, cols, v);
#pragma unroll
    for (int i = 0; i < SX; ++i) d[i] = (u[i] + v[i]) >> 1, diff[i] = absdiff(u[i], v[i]) >> 1;
    if (o0 >= 0) {
        const T* t2[2] = {(const T*)(base + o0) + first, (const T*)(base + o4) + first};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            load_n<T, SX>(t2[k] + (int64_t)(y - 1) * cols, x0, cols, u);
            load_n<T, SX>(t2[k] + (int64_t)(y + 1) * cols, x0, cols, v);
#pragma unroll
            for (int i = 0; i < SX; ++i) diff[i] = max(diff[i], (absdiff(u[i], c[i]) + absdiff(v[i], e[i])) >> 1);
        }
    }
    if (y >= 2 && y + 2 < rows) {                                        // the spatial check
        int bb[SX], gg[SX];
        load_n<T, SX>(p1 + (int64_t)(y - 2) * cols, x0, cols, u);
        load_n<T, SX>(n1 + (int64_t)(y - 2) * cols, x0, cols, v);
#pragma unroll
        for (int i = 0; i < SX; ++i) bb[i] = (u[i] + v[i]) >> 1;
        load_n<T, SX>(p1 + (int64_t)(y + 2) * cols, x0, cols, u);
        load_n<T, SX>(n1 + (int64_t)(y + 2) * cols, x0, cols, v);
#pragma unroll
        for (int i = 0; i < SX; ++i) {
            gg[i] = (u[i] + v[i]) >> 1;
            const int de = d[i] - e[i], dc = d[i] - c[i], bc = bb[i] - c[i], ge = gg[i] - e[i];
            const int mx = max(max(de, dc), min(bc, ge)), mn = min(min(de, dc), max(bc, ge));
            diff[i] = max(diff[i], max(mn, -mx));
        }
    }
#pragma unroll
    for (int i = 0; i < SX; ++i) sp[i] = min(max(sp[i], d[i] - diff[i]), d[i] + diff[i]);
    store_n<T, SX>(dst, sp, n);
}

}  // namespace

extern "C" int demfi_yuv_deint_adaptive(void* base, int64_t size_bytes, const int64_t* offsets, const int64_t* offsets_dev, int n, int h,
                                        int w, int layout, int sample_bytes, uint64_t odd_mask, void* stream)
{
    const char* fn = "demfi_yuv_deint_adaptive";
    if (!base || !offsets || !offsets_dev || n < 0 || n > 64)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d outside 0..64", fn, n);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (layout != DEMFI_YUV_420 && layout != DEMFI_YUV_422 && layout != DEMFI_YUV_444 && layout != DEMFI_YUV_MONO)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: layout %d", fn, layout);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    const int64_t pb = payload_of(layout, h, w) * sample_bytes;
    // a field's five payloads: absent ones anywhere but its own, in the middle; a whole payload inside the buffer
    uintptr_t low = (uintptr_t)base;
    if (int st = walk_offsets(fn, offsets, n, 5, 5, OFFS_BUT_CENTRE, 2, size_bytes - pb, 0, &low)) return st;
    if (int st = check_even(fn, sample_bytes, low)) return st;
    for (int i = 0; i < n; ++i) {
        const int64_t* o = offsets + 5 * i;
        if (o[1] < 0 && o[3] < 0)
            return demfi_set_error(DEMFI_ERR_ARG, "%s: field %d has neither the field before it nor the one after it", fn, i);
        for (int j = 0; j < i; ++j)
            if (offsets[5 * j + 2] == o[2])
                return demfi_set_error(DEMFI_ERR_ARG, "%s: fields %d and %d rebuild the same payload", fn, j, i);
    }
    if (n == 0) return DEMFI_OK;
    const int ch = layout == DEMFI_YUV_420 ? (h + 1) / 2 : layout == DEMFI_YUV_MONO ? 0 : h;
    const int cw = layout == DEMFI_YUV_444 ? w : layout == DEMFI_YUV_MONO ? 0 : (w + 1) / 2;
    const int64_t lanes = (int64_t)((h + 1) / 2) * ((w + SX - 1) / SX) + 2 * (int64_t)((ch + 1) / 2) * ((cw + SX - 1) / SX);
    const dim3 grid((unsigned)((lanes + NT - 1) / NT), (unsigned)n);
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(adaptive_kernel<TAG_TYPE(t)>, grid, dim3(NT), 0, (hipStream_t)stream, (uint8_t*)base, offsets_dev, h, w, ch, cw, odd_mask);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}

extern "C" int demfi_yuv_bob(void* payloads, int64_t stride_bytes, int n, int h, int w, int layout, int sample_bytes, uint64_t odd_mask,
                             void* stream)
{
    const char* fn = "demfi_yuv_bob";
    if (!payloads || n < 0 || n > 64)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: NULL buffer or n=%d outside 0..64", fn, n);
    if (int st = check_frame_size(fn, h, w)) return st;
    if (layout != DEMFI_YUV_420 && layout != DEMFI_YUV_422 && layout != DEMFI_YUV_444 && layout != DEMFI_YUV_MONO)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: layout %d", fn, layout);
    if (int st = check_sample_bytes(fn, sample_bytes)) return st;
    if (int st = check_even(fn, sample_bytes, (uintptr_t)payloads | (uintptr_t)stride_bytes)) return st;
    if (stride_bytes < payload_of(layout, h, w) * sample_bytes)
        return demfi_set_error(DEMFI_ERR_ARG, "%s: stride of %lld bytes below the payload's %lld", fn, (long long)stride_bytes,
                               (long long)(payload_of(layout, h, w) * sample_bytes));
    if (n == 0) return DEMFI_OK;
    const int ch = layout == DEMFI_YUV_420 ? (h + 1) / 2 : layout == DEMFI_YUV_MONO ? 0 : h;
    const int cw = layout == DEMFI_YUV_444 ? w : layout == DEMFI_YUV_MONO ? 0 : (w + 1) / 2;
    const int64_t lanes = (int64_t)((h + 1) / 2) * ((w + SX - 1) / SX) + 2 * (int64_t)((ch + 1) / 2) * ((cw + SX - 1) / SX);
    const dim3 grid((unsigned)((lanes + NT - 1) / NT), (unsigned)n);
    by_sample(sample_bytes, [&](auto t) {
        hipLaunchKernelGGL(bob_kernel<TAG_TYPE(t)>, grid, dim3(NT), 0, (hipStream_t)stream, (uint8_t*)payloads, stride_bytes, h, w, ch, cw, odd_mask);
    });
    DEMFI_HIP_CHECK(hipGetLastError());
    return DEMFI_OK;
}
