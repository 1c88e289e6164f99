// Device toolkit shared by every MFMA kernel unit (the conv_*.hip units through conv_common.h; resblock.hip, gru.hip and wsconv.hip
// directly): the compile-time loop, the MFMA wrappers, the one-instruction fp16 residual add / subtract, the XCD work partition, and -- trace build only -- the
// phase trace.  No tile constants and no buffers of its own: a unit that wants a trace buffer declares it (DEMFI_TRACE_BUFFER).
// Everything here is __forceinline__ or a macro: moving a helper in or out of this file must not change one instruction of any kernel
// (build.sh --asm, profiles/kernel_toolkit_isa.md).
#pragma once
#include "common.h"
#include <type_traits>
#ifdef DEMFI_TRACE
#include <vector>
#endif

namespace {

// Compile-time loop: the accumulator arrays must only ever be indexed by constants (runtime-indexed
// ext_vector arrays go to scratch), and '#pragma unroll' is refused on the large epilogue body.
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

template <typename T> struct Mma;

template <> struct Mma<half_t> {
    static __device__ __forceinline__ void run(f16x_t& acc, const uint4& a, const uint4& b)
    {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8_t, a), __builtin_bit_cast(h8_t, b),
                                                     acc, 0, 0, 0);
    }
    // first MFMA of an accumulator with an explicit C operand (the bias rows: saves the epilogue's bias adds)
    static __device__ __forceinline__ void initc(f16x_t& acc, const uint4& a, const uint4& b, const f16x_t& c)
    {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8_t, a), __builtin_bit_cast(h8_t, b), c, 0, 0, 0);
    }
    // first MFMA of an accumulator: C = inline constant 0 instead of 16 v_mov per accumulator before the loop
    static __device__ __forceinline__ void init(f16x_t& acc, const uint4& a, const uint4& b)
    {
        const f16x_t z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8_t, a), __builtin_bit_cast(h8_t, b), z, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static __device__ __forceinline__ void run(f16x_t& acc, const uint4& a, const uint4& b)
    {
        f4_t fa = __builtin_bit_cast(f4_t, a), fb = __builtin_bit_cast(f4_t, b);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[0], fb[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[1], fb[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[2], fb[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[3], fb[3], acc, 0, 0, 0);
    }
};

// (fp16 half of a packed pair) * 1.0 + c in one VALU op: the residual add of the epilogues (bias + residual -> an accumulator's initial value)
__device__ __forceinline__ float res_mix_lo(unsigned a, float c)
{
    float d = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(a), "v"(c));
#endif
    return d;
}
__device__ __forceinline__ float res_mix_hi(unsigned a, float c)
{
    float d = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(a), "v"(c));
#endif
    return d;
}
// c - (fp16 half of a packed pair) in one VALU op (no v_cvt_f32_f16): the GRU update's tanh(.) - h
__device__ __forceinline__ float sub_mix_lo(float c, unsigned a)
{
    float d = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(a), "v"(c));
#endif
    return d;
}
__device__ __forceinline__ float sub_mix_hi(float c, unsigned a)
{
    float d = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(a), "v"(c));
#endif
    return d;
}

// ---- work partition of a persistent kernel over the 8 XCDs (workgroup b runs on XCD b % 8) -------------------------------------------------
// XCD x owns the contiguous band [lo, lo + n) of the 'total_' work items, so neighbours (which share halo data) meet in one L2; without
// whole XCD rows of workgroups, or with fewer items than workgroups, the plain split.  MACROS, not functions: as __forceinline__ functions
// they moved register allocation and scheduling of the kernels around them (profiles/kernel_toolkit_isa.md).
// XCD_ITEM_RUN: workgroup -> the contiguous run [it0_, it1_) of its band (kernels that carry state from one item to the next)
#define XCD_ITEM_RUN(total_, it0_, it1_)                                                                             \
    {                                                                                                                 \
        const int G = gridDim.x;                                                                                      \
        if ((G & 7) == 0 && (total_) >= G) {                                                                          \
            const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, nw = G >> 3;                                       \
            const int q = (total_) >> 3, r = (total_) & 7;                                                            \
            const int lo = xcd * q + min(xcd, r), n = q + (xcd < r ? 1 : 0);                                          \
            it0_ = lo + (int)(((int64_t)n * idx) / nw);                                                               \
            it1_ = lo + (int)(((int64_t)n * (idx + 1)) / nw);                                                         \
        } else {                                                                                                      \
            it0_ = (int)(((int64_t)(total_) * blockIdx.x) / G);                                                       \
            it1_ = (int)(((int64_t)(total_) * (blockIdx.x + 1)) / G);                                                 \
        }                                                                                                             \
    }
// XCD_TILE_STRIDE: workgroup -> tiles first_, first_ + step_, ... < end_ of its band (the workgroups of an XCD interleave)
#define XCD_TILE_STRIDE(total_, first_, end_, step_)                                                                 \
    {                                                                                                                 \
        const int G = gridDim.x;                                                                                      \
        if ((G & 7) == 0 && (total_) >= G) {                                                                          \
            const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;                                                    \
            const int q = (total_) >> 3, r = (total_) & 7;                                                            \
            const int lo = xcd * q + min(xcd, r);                                                                     \
            first_ = lo + idx;                                                                                        \
            end_ = lo + q + (xcd < r ? 1 : 0);                                                                        \
            step_ = G >> 3;                                                                                           \
        } else {                                                                                                      \
            first_ = blockIdx.x;                                                                                      \
            end_ = (total_);                                                                                          \
            step_ = G;                                                                                                \
        }                                                                                                             \
    }

// ---- in-kernel phase trace (libdemfi_hip_trace.so, build.sh --trace; never in the product) ----------------------------------------
// A unit declares ONE buffer, DEMFI_TRACE_BUFFER(workgroups, waves, steps, stamps), inside its anonymous namespace.  Lane 0 of a wave
// stamps s_memtime into [wg][wave][step][stamp] for the first 'steps' loop iterations of workgroups 0 .. workgroups-1:
// TRACE_STAMP(wave, step, stamp) or TRACE_STAMP(wave, step, stamp, flag), which also sets bit 63 where 'flag' holds.  What the stamp
// numbers mean is the unit's business.  TRACE_DRAIN(out, merge) is the host side: the buffer's TR_N entries go to out (OR-ed into it
// if 'merge') and the device copy is cleared; it yields 0 or a negative error code.
#ifdef DEMFI_TRACE
#define DEMFI_TRACE_BUFFER(wgs_, waves_, steps_, stamps_)                                                            \
    constexpr int TR_WGS = (wgs_), TR_WAVES = (waves_), TR_STEPS = (steps_), TR_STAMPS = (stamps_);                  \
    constexpr int64_t TR_N = (int64_t)TR_WGS * TR_WAVES * TR_STEPS * TR_STAMPS;                                      \
    __device__ unsigned long long g_trace[TR_N];
// the stamp itself; TRACE_STAMP appends the default flag, so flag_ is the caller's fourth argument or false.  The flag is read AFTER the
// counter, in the macro and not in a function: an argument evaluated before the counter moved the resblock's register allocation.
#define TRACE_STAMP_(wave_, k_, i_, flag_, ...)                                                                      \
    do {                                                                                                              \
        if (blockIdx.x < TR_WGS && (k_) < TR_STEPS && (threadIdx.x & 63) == 0)                                       \
            g_trace[((blockIdx.x * TR_WAVES + (wave_)) * TR_STEPS + (k_)) * TR_STAMPS + (i_)] =                      \
                __builtin_readcyclecounter() | ((unsigned long long)((flag_) ? 1 : 0) << 63);                        \
    } while (0)
#define TRACE_STAMP(...) TRACE_STAMP_(__VA_ARGS__, false, )
inline int trace_drain(const void* symbol, int64_t n, unsigned long long* out, bool merge)
{
    std::vector<unsigned long long> tmp(n);
    DEMFI_HIP_CHECK(hipMemcpyFromSymbol(tmp.data(), symbol, n * 8));
    for (int64_t i = 0; i < n; ++i) out[i] = merge ? (out[i] | tmp[i]) : tmp[i];
    tmp.assign(n, 0ull);
    DEMFI_HIP_CHECK(hipMemcpyToSymbol(symbol, tmp.data(), n * 8));
    return 0;
}
#define TRACE_DRAIN(out_, merge_) trace_drain(HIP_SYMBOL(g_trace), TR_N, (out_), (merge_))
#else
#define DEMFI_TRACE_BUFFER(wgs_, waves_, steps_, stamps_)
#define TRACE_STAMP(...) do { } while (0)
#define TRACE_DRAIN(out_, merge_) 0
#endif

}  // namespace
