// Device pieces the LDS-direct MFMA kernels share (gemm_nt.hip, gemm_lw.hip, gemm_k192.hip through gemm_common.h; wgrad256.hip,
// wgrad_lw.hip): the global -> LDS load, its buffer resource, the waits and the barrier that publish it, and the compile-time loop the
// unrolled rings are written with.  Where two kernels need two DIFFERENT instructions for the same job, both are here under two names.
#pragma once
#include "dgx_common.h"
#include <type_traits>

namespace {
// voffset beyond num_records: the lane touches no memory, its 16 bytes land in LDS as zeros
constexpr uint32_t BUF_OOB = 0x80000000u;

// 16 bytes per lane from a raw buffer straight into LDS (no staging registers): lane i of the wave lands at lds_wave_base + 16*i.
// Out-of-range lanes (voff >= num_records) do not touch memory.  The caller orders the data with s_waitcnt vmcnt + barrier; the
// compiler does not track these loads.  soff: scalar byte offset, part of the range check on gfx950 (tools/probes/soffset_probe.hip) --
// the row offset of a stage can travel there, no VALU add per load in a loop whose lone wave per SIMD pays for every instruction next
// to its MFMAs.
__device__ __forceinline__ void lds_load16(uint32_t voff, u32x4 rsrc, uint32_t lds_wave_base, uint32_t soff) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(voff), "s"(rsrc), "s"(lds_wave_base), "s"(soff)
                 : "memory");
}
// raw buffer resource over [base, base + bytes)
__device__ __forceinline__ u32x4 buf_rsrc(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)base;
    return u32x4{(uint32_t)a, (uint32_t)(a >> 32) & 0xffffu, bytes, 0x00020000u};
}
// ... with every word passed through readfirstlane: wgrad_lw.hip's form, whose loader waves rebuild their descriptors per item from a
// table entry found with a dynamic index (not the same instructions as buf_rsrc: each kernel keeps the one it was measured with)
__device__ __forceinline__ u32x4 buf_rsrc_uniform(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)base;
    return u32x4{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(a >> 32) & 0xffffu)),
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000u};
}
__device__ __forceinline__ uint32_t to_sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// counted wait for this wave's own LDS-direct loads (the compiler does not count them)
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// lgkmcnt(0) as inline assembly: a fence the compiler cannot move memory operations across
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// lgkmcnt(0) as the BUILTIN: the compiler's wait-count pass sees it, so the fragment reads issued behind the barrier are waited for
// with their own counts (behind an inline-asm wait it re-waits lgkmcnt(0) in front of the first MFMA of the phase)
__device__ __forceinline__ void wait_lgkm0_tracked() { __builtin_amdgcn_s_waitcnt(0xc07f); }
// raw s_barrier (LDS-direct loads stay in flight across it) + a scheduling fence
__device__ __forceinline__ void wg_barrier() {
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// f(ic<0>{}), ..., f(ic<N-1>{}): a loop whose index is a constant expression in the body (ring slots as immediates)
template <int N> using ic = std::integral_constant<int, N>;
template <int N, int I = 0, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(ic<I>{}); static_for<N, I + 1>(f); }
}

// eight bf16 ones: ones^T x fragment on the matrix pipe = column sums (the bias gradients)
__device__ __forceinline__ bf16x8 bf16_ones() {
    return bf16x8{(short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80};
}
}  // namespace
