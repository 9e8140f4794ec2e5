// Shared pieces of libdgx's forward / input-gradient GEMM kernels (gemm_nt.hip: 8 waves that load their own operands, two workgroups
// per CU for the short contractions; gemm_lw.hip: 8 MFMA waves + 4 loader waves, persistent; gemm_k192.hip: resident weight panel):
// problem descriptor, the operand addressing and split-K pieces the tiled kernels share, exact-GELU arithmetic
// and the fused tails of the read-out (bias | bias + GELU with both tensors | x GELU'(f1) |
// x ReLU'(act) | window-reverse + DropPath + residual).
#pragma once
#include "lds_direct.h"
#include "gemm_plan.h"
#include "winmap.h"
#include <type_traits>

constexpr int G_ORDERS = WM_IDENTITY | WM_CLASSIC | WM_COMPACT;      // the row orders of the residual epilogue (M rows, all of them tokens or classic rows)
constexpr int GBK = 64;                 // K-step (elements): 128-byte tile rows

namespace dgxgemm {
struct GemmP {
    const uint16_t* A;
    const uint16_t* B;
    int M, N, K, lda, ldb;
    int tiles_n, total, per_xcd;
    int splits, kt_per_split;  // split-K: workgroup (tile, s) contracts K-tiles [s * kt_per_split, ...) into ws[s] (fp32)
    float* ws;
    int mode;
    uint16_t* C;            // bf16 (M, ldc): modes 0, 1, 2 (pre-activation), 4
    int ldc;
    const uint16_t* bias;   // bf16 (N) or null
    uint16_t* C2;           // mode 2: GELU(C)
    const uint16_t* aux;    // mode 4: f1 (M, ldaux)
    int ldaux;
    const void* res;        // mode 3: residual stream (tokens, N) fp32 | bf16
    void* out;              //         out = res + scale[b] * y
    const float* scale;     //         per-sample DropPath factor or null
    int res_dtype;
    WmMap map;              //         the order of the GEMM rows (winmap.h)
    // implicit 3x3 convolution (pad 1, stride 1) over a zero-bordered NHWC image (dgx_conv3x3_*): K-tile kt of the A operand
    // is tap kt / conv_kc, channels 64 (kt % conv_kc) ..: the SAME rows shifted by (tap / 3) * conv_wp + tap % 3 pixels;
    // GEMM rows are the N*H*W OUTPUT pixels (cmap: n, h, w); row m reads the padded position of its pixel (per-lane offset), so
    // no border rows are computed and M tiles exactly when N*H*W does (P3 level, 2 x 128 x 128 = 256 tiles of 128 rows: one round
    // of the chip; over the padded grid it was 265 tiles = two rounds)
    int conv_kc, conv_wp;
    int cmap_n, cmap_h, cmap_w;
    int relu;
    // grouped implicit convolution (dgx_conv3x3_gemm_multi): ngrp > 0 images that share B / bias / N / K / the epilogue -- the FPN
    // levels under one tower layer -- in ONE launch: tile L belongs to group g = the last one with tile0 <= L; the kernel patches
    // A / C / M and the image geometry from the group's record and goes on as for a single image (no split-K in this form)
    int ngrp;
    struct Grp { const uint16_t* A; uint16_t* C; int M, cn, ch, cw, wp, tile0; } grp[6];
};
constexpr int GEMM_MAXG = 6;
}  // namespace dgxgemm
using dgxgemm::GemmP;

namespace {

// The tail compiled into an instantiation: MC >= 0 fixes the mode (3 / 6: mode 3 with a bf16 / fp32 residual stream), MC < 0 leaves it
// a run-time field.  With the mode a run-time field the tail's operand prefetch sat under mode branches, and the compiler's wait-count
// model, merging the path without a prefetch, waited for every outstanding load (vmcnt(0)) before the staging pass the prefetch was
// meant to overlap (round 5, tools/isa_wait_scan.py).
template <int MC> __device__ __forceinline__ void g_fix_mode(GemmP& P) {
    if constexpr (MC == 6) { P.mode = 3; P.res_dtype = DGX_F32; }
    else if constexpr (MC == 3) { P.mode = 3; P.res_dtype = DGX_BF16; }
    else if constexpr (MC >= 0) P.mode = MC;
}
// Host side of the same: calls f(std::integral_constant<int, mc>) for a tail mc = dgxplan::tail_mc (the mode, 6 for an fp32 residual
// stream; anything else arrives as 0).  Each launcher maps the values it has no instantiation for onto the one that serves them.
template <class F> int g_with_mc(int mc, F&& f) {
    switch (mc) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        default: return f(std::integral_constant<int, 0>{});
    }
}
inline int g_tail_mc(const GemmP& P) { return dgxplan::tail_mc(P.mode, P.res_dtype == DGX_BF16); }

// Grouped convolution: the record of the image that tile L belongs to (the last one with tile0 <= L); the caller patches A / C / M and
// the image geometry of its own copy of the descriptor from it and goes on with tile L - tile0 of that image.  L comes out of a division,
// which runs on the vector unit: pass it through readfirstlane first, which tells the compiler the value is uniform.  Constant indices
// only: a dynamic index into the by-value descriptor would go through private memory and lose uniformity.
__device__ __forceinline__ dgxgemm::GemmP::Grp g_group_of_tile(const GemmP& P, int L) {
    dgxgemm::GemmP::Grp q = P.grp[0];
#pragma unroll
    for (int k = 1; k < dgxgemm::GEMM_MAXG; ++k)
        if (k < P.ngrp && L >= P.grp[k].tile0) q = P.grp[k];
    return q;
}
__device__ __forceinline__ void g_enter_group(GemmP& P, const dgxgemm::GemmP::Grp& q) {
    P.A = q.A; P.C = q.C; P.M = q.M;
    P.cmap_n = q.cn; P.cmap_h = q.ch; P.cmap_w = q.cw; P.conv_wp = q.wp;
}
// Byte offset of this lane's 16-byte chunk (logical chunk lc) of GEMM row m of the A operand, BUF_OOB for a row beyond M.  Implicit
// convolution: row m is output pixel (n, y, x), which reads its position in the zero-bordered image.
__device__ __forceinline__ uint32_t g_a_voff(const GemmP& P, int m, int lc) {
    int64_t arow = m;
    if (P.conv_kc) {
        const int hw = P.cmap_h * P.cmap_w;
        const int n = m / hw, r = m - n * hw;
        const int y = r / P.cmap_w, x = r - y * P.cmap_w;
        arow = ((int64_t)n * (P.cmap_h + 2) + y + 1) * P.conv_wp + x + 1;
    }
    return m < P.M ? (uint32_t)((arow * P.lda + lc * 8) * 2) : BUF_OOB;
}
// soffset of K-tile kta of the A operand; implicit convolution: tap shift (rows) + channel block of the tap
__device__ __forceinline__ uint32_t g_a_soff(const GemmP& P, int kta) {
    uint32_t s = (uint32_t)kta * (GBK * 2);
    if (P.conv_kc) {
        const int tap = kta / P.conv_kc, kc = kta - tap * P.conv_kc;
        s = (uint32_t)((tap / 3) * P.conv_wp + tap % 3) * (uint32_t)(P.lda * 2) + (uint32_t)kc * (GBK * 2);
    }
    return s;
}
// bias entries of 4 consecutive columns (two packed bf16 pairs) as floats
__device__ __forceinline__ void g_bias4(const u32x2 raw, float (&bv)[4]) {
    bv[0] = __uint_as_float(raw[0] << 16); bv[1] = __uint_as_float(raw[0] & 0xffff0000u);
    bv[2] = __uint_as_float(raw[1] << 16); bv[3] = __uint_as_float(raw[1] & 0xffff0000u);
}

constexpr float kGInvSqrt2 = 0.70710678118654752440f;
constexpr float kGInvSqrt2Pi = 0.39894228040143267794f;
// Mode 3: (token << 32 | DropPath factor bits) of tile row `tid` (rows m0 ..) into the tile's LDS table, -1 for a padding row or one
// beyond M.  The factor is fetched HERE, once per tile row -- as a load inside the read-out's `locate` it sat in front of every chunk's
// store behind an s_waitcnt vmcnt(0) that also waited for the prefetched operands of the next slab and for the stores before it
// (round 5, tools/isa_wait_scan.py).
__device__ __forceinline__ void g_fill_rowtok(const GemmP& P, DGX_LDS int64_t* rowtok, int m0, int tid) {
    int b = 0;
    const int64_t orow = (int64_t)m0 + tid;
    const int64_t tok = orow < P.M ? wm_row_token<int64_t, G_ORDERS>(P.map, orow, b) : -1;
    const float scv = (tok >= 0 && P.scale) ? P.scale[b] : 1.0f;
    rowtok[tid] = tok < 0 ? -1 : ((tok << 32) | (int64_t)__float_as_uint(scv));
}

// Exact-GELU pieces  cdf(x) = (1 + erf(x / sqrt 2)) / 2  and  pdf(x) = exp(-x^2 / 2) / sqrt(2 pi)  from ONE exponential:
// erfc(z) = t (a1 + t (a2 + t (a3 + t (a4 + t a5)))) exp(-z^2), t = 1 / (1 + p z), z >= 0 (Abramowitz & Stegun 7.1.26,
// |error| <= 1.5e-7 absolute, i.e. ~2 ulp of an fp32 erf near 1 and 4 orders below the bf16 quantum of the results it
// feeds); the negative side uses erfc directly, so the tail keeps its relative accuracy.  ~16 VALU operations per
// element against ~37 for the two-branch erff of the device library -- the epilogue is VALU-bound on it.
__device__ __forceinline__ void g_gelu_terms(float x, float& cdf, float& pdf) {
    const float z = fabsf(x) * kGInvSqrt2;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    const float e = __expf(-z * z);
    float p = 1.061405429f;                        // explicit fma: the library is built with -ffp-contract=off
    p = fmaf(p, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float h = 0.5f * (p * t) * e;            // erfc(|z|) / 2
    cdf = x < 0.f ? h : 1.0f - h;
    pdf = e * kGInvSqrt2Pi;
}
// The same arithmetic on PAIRS of elements: every plain operation is a packed-fp32 instruction (v_pk_mul_f32 / v_pk_fma_f32 /
// v_pk_add_f32: two results per issue slot, the same IEEE roundings as the scalar forms, so results are bit-identical); only the
// reciprocal, the exponential and the sign select stay per element.  Halves the VALU slots of the GELU read-outs; measured
// in situ the read-out is bound by its loads and stores, not by these (fc1 forward 70.8 -> 69.6 us).
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ void g_gelu_terms2(f32x2 x, f32x2& cdf, f32x2& pdf) {
    const f32x2 ax = {fabsf(x[0]), fabsf(x[1])};
    const f32x2 z = ax * kGInvSqrt2;
    const f32x2 d = __builtin_elementwise_fma(f32x2{0.3275911f, 0.3275911f}, z, f32x2{1.0f, 1.0f});
    const f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    const f32x2 nz = -z;
    const f32x2 zz = nz * z;
    const f32x2 e = {__expf(zz[0]), __expf(zz[1])};
    f32x2 p = {1.061405429f, 1.061405429f};
    p = __builtin_elementwise_fma(p, t, f32x2{-1.453152027f, -1.453152027f});
    p = __builtin_elementwise_fma(p, t, f32x2{1.421413741f, 1.421413741f});
    p = __builtin_elementwise_fma(p, t, f32x2{-0.284496736f, -0.284496736f});
    p = __builtin_elementwise_fma(p, t, f32x2{0.254829592f, 0.254829592f});
    const f32x2 h = (p * t) * 0.5f * e;           // scalar form: 0.5f * (p * t) * e -- multiplication commutes exactly
    const f32x2 o = f32x2{1.0f, 1.0f} - h;
    cdf = f32x2{x[0] < 0.f ? h[0] : o[0], x[1] < 0.f ? h[1] : o[1]};
    pdf = e * kGInvSqrt2Pi;
}
__device__ __forceinline__ f32x2 g_gelu2(f32x2 x) {
    f32x2 cdf, pdf;
    g_gelu_terms2(x, cdf, pdf);
    return x * cdf;
}
__device__ __forceinline__ f32x2 g_gelu_grad2(f32x2 x) {
    f32x2 cdf, pdf;
    g_gelu_terms2(x, cdf, pdf);
    return cdf + x * pdf;                          // mul then add, as the scalar form (no contraction)
}
__device__ __forceinline__ float g_gelu(float x) {
    float cdf, pdf;
    g_gelu_terms(x, cdf, pdf);
    return x * cdf;
}
__device__ __forceinline__ float g_gelu_grad(float x) {
    float cdf, pdf;
    g_gelu_terms(x, cdf, pdf);
    return cdf + x * pdf;
}

// The fused tail of one 8-column chunk y = bf16(acc + bias) of output row gm (shared by the GEMM read-outs and the split-K
// fold), in two halves so that callers can put many chunks' extra operands (saved pre-activation of mode 4, residual of mode 3) in flight before consuming any:
// g_epi_prefetch issues the loads, g_epi_finish does the arithmetic and the stores.  tok / sc: mode 3 token index (>= 0)
// and DropPath factor of the row.
__device__ __forceinline__ void g_epi_prefetch(const GemmP& P, int gm, int gn, int64_t tok, u32x4& xa, u32x4& xb) {
    if (P.mode == 4 || P.mode == 5) {
        xa = *reinterpret_cast<const u32x4*>(P.aux + (int64_t)gm * P.ldaux + gn);
    } else if (P.mode == 3) {
        const int64_t o = tok * P.N + gn;
        if (P.res_dtype == DGX_BF16) {
            xa = *reinterpret_cast<const u32x4*>((const uint16_t*)P.res + o);
        } else {
            xa = reinterpret_cast<const u32x4*>((const float*)P.res + o)[0];
            xb = reinterpret_cast<const u32x4*>((const float*)P.res + o)[1];
        }
    }
}
__device__ __forceinline__ void g_epi_finish(const GemmP& P, int gm, int gn, const u32x4 y, int64_t tok, float sc, const u32x4 xa,
                                             const u32x4 xb) {
    if (P.mode <= 1) {
        u32x4 o = y;
        if (P.relu) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = ((o[k] & 0x8000u) ? 0u : (o[k] & 0xffffu)) | ((o[k] & 0x80000000u) ? 0u : (o[k] & 0xffff0000u));
        }
        *reinterpret_cast<u32x4*>(P.C + (int64_t)gm * P.ldc + gn) = o;
    } else if (P.mode == 2) {
        *reinterpret_cast<u32x4*>(P.C + (int64_t)gm * P.ldc + gn) = y;
        float v[8], o[8];
        unpack8(y, v);
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            const f32x2 r = g_gelu2(f32x2{v[k], v[k + 1]});
            o[k] = r[0]; o[k + 1] = r[1];
        }
        *reinterpret_cast<u32x4*>(P.C2 + (int64_t)gm * P.ldc + gn) = pack8(o);
    } else if (P.mode == 4) {
        float gq[8], v[8], d[8];
        unpack8(y, gq);
        unpack8(xa, v);
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            const f32x2 r = f32x2{gq[k], gq[k + 1]} * g_gelu_grad2(f32x2{v[k], v[k + 1]});
            d[k] = r[0]; d[k + 1] = r[1];
        }
        *reinterpret_cast<u32x4*>(P.C + (int64_t)gm * P.ldc + gn) = pack8(d);
    } else if (P.mode == 5) {                      // ReLU': pass y where the saved activation is positive
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = xa[k];
            const uint32_t lo = ((a & 0x8000u) || !(a & 0x7fffu)) ? 0u : 0xffffu;
            const uint32_t hi = ((a & 0x80000000u) || !(a & 0x7fff0000u)) ? 0u : 0xffff0000u;
            o[k] = y[k] & (lo | hi);
        }
        *reinterpret_cast<u32x4*>(P.C + (int64_t)gm * P.ldc + gn) = o;
    } else {                                       // mode 3
        float yv[8], xv[8];
        unpack8(y, yv);
        const int64_t o = tok * P.N + gn;
        if (P.res_dtype == DGX_BF16) {
            unpack8(xa, xv);
#pragma unroll
            for (int k = 0; k < 8; ++k) xv[k] += sc * yv[k];
            *reinterpret_cast<u32x4*>((uint16_t*)P.out + o) = pack8(xv);
        } else {
            f32x4 x0 = __builtin_bit_cast(f32x4, xa), x1 = __builtin_bit_cast(f32x4, xb);
#pragma unroll
            for (int k = 0; k < 4; ++k) { x0[k] += sc * yv[k]; x1[k] += sc * yv[4 + k]; }
            reinterpret_cast<f32x4*>((float*)P.out + o)[0] = x0;
            reinterpret_cast<f32x4*>((float*)P.out + o)[1] = x1;
        }
    }
}
__device__ __forceinline__ void g_epilogue_chunk(const GemmP& P, int gm, int gn, const u32x4 y, int64_t tok, float sc) {
    u32x4 xa = {0u, 0u, 0u, 0u}, xb = {0u, 0u, 0u, 0u};
    g_epi_prefetch(P, gm, gn, tok, xa, xb);
    g_epi_finish(P, gm, gn, y, tok, sc, xa, xb);
}
}  // namespace
