// Phase clocks of the development build (DGX_DEV=1 python -m divergen_amd.csrc.build -> _obj/dev/libdgx_dev.so; the product
// build compiles every macro below to nothing).  A kernel marks a phase boundary with DGX_CLK(slot), slot 0..7: thread 0 of every
// workgroup below DGX_CLK_WGS writes the shader-clock counter to dgx_clk_buf[workgroup][slot] with a plain store (a later stamp of the
// same slot overwrites the earlier one: a persistent kernel leaves the stamps of its last item).  DGX_CLK_RT stamps the constant
// 100 MHz counter instead; the ratio of two intervals taken with both is the clock the CU ran at.  The buffer is per translation
// unit; DGX_CLK_READER(name) defines that unit's accessor `int name(unsigned long long out[DGX_CLK_WGS * 8])`, which copies the
// stamps of the launches since the last call to the host and clears them (tools/gemm_clock_probe.py).
#pragma once
#ifdef DGX_DEV
#include <hip/hip_runtime.h>
constexpr int DGX_CLK_WGS = 4096;
namespace { __device__ unsigned long long dgx_clk_buf[DGX_CLK_WGS * 8]; }
#define DGX_CLK_AT(i, t) do { if (threadIdx.x == 0 && blockIdx.x < DGX_CLK_WGS) dgx_clk_buf[blockIdx.x * 8 + (i)] = (t); } while (0)
#define DGX_CLK(i) DGX_CLK_AT(i, __builtin_readcyclecounter())
#define DGX_CLK_RT(i) DGX_CLK_AT(i, __builtin_amdgcn_s_memrealtime())
#define DGX_CLK_READER(name)                                                                                      \
    extern "C" int name(unsigned long long* out) {                                                                \
        void* buf = nullptr;                                                                                      \
        if (hipDeviceSynchronize() != hipSuccess || hipGetSymbolAddress(&buf, HIP_SYMBOL(dgx_clk_buf)) != hipSuccess ||  \
            hipMemcpy(out, buf, sizeof(dgx_clk_buf), hipMemcpyDeviceToHost) != hipSuccess ||                      \
            hipMemset(buf, 0, sizeof(dgx_clk_buf)) != hipSuccess)                                                 \
            return -1;                                                                                            \
        return 0;                                                                                                 \
    }
#else
#define DGX_CLK(i)
#define DGX_CLK_RT(i)
#define DGX_CLK_READER(name)
#endif
