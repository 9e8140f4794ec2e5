// CLIP text transformer, forward only (the encoder is frozen), for gfx950: the pieces of CLIPTEXT.encode_text
// (DG/divergen/modeling/text/text_encoder.py:154-163) that no other kernel of this library covers.  The GEMMs run on dgx_gemm_bf16_nt, the
// per-layer LayerNorms on dgx_layernorm_fwd in token order; layers/text_ops.py strings them together.
//
//   dgx_text_embed            token_embedding[tok] + positional_embedding[l] -> the fp32 residual stream, and eot[b] = text.argmax(-1).
//   dgx_causal_attention_fwd  nn.MultiheadAttention with the causal mask of build_attention_mask, heads of 64: one workgroup per
//                             (sample, head), one wave per 16-query strip, MFMA 16x16x32 bf16 in the swapped orientation of
//                             window_attention.hip (S^T = K Q^T: a lane owns ONE query and 4 keys per tile), fp32 log2-domain softmax,
//                             K and V of the (sample, head) in LDS (<= 96 rows x 64: 27 KB), S never in HBM.  Key tiles above the
//                             diagonal are SKIPPED (strip w touches tiles 0..w), the diagonal tile is masked by a select (never an
//                             additive constant), so nothing a later token holds can reach an earlier row.
//   dgx_quick_gelu            x * sigmoid(1.702 x) over bf16, fp32 arithmetic.
//   dgx_text_eot_project      ln_final of the end-token row and text_projection, both fp32, one workgroup per sample.
//
// Rounding contract (tests/_text_ref64.py): bf16 q, k, v and output; logits, softmax statistics and accumulations fp32; P (the
// un-normalised exp2(s - max), normalised behind the MFMA) rounded to bf16 where it feeds the MFMA; one final bf16 rounding of the output.
#include "dgx_common.h"

namespace {
#define TE_LOG2E 1.4426950408889634f
constexpr int TE_NP = DGX_TEXT_MAX_L;      // rows of the K / V images: six 16-row strips
constexpr int TE_NT = TE_NP / 16;          // strips = waves of the largest workgroup
// row stride (elements) of the row-major K / V images: 72 = 36 banks.  The 16-byte fragment reads (8 consecutive rows per pass, 4 banks
// each: 0 36 8 44 16 52 24 60) and the transpose reads (4 consecutive rows x 8 banks: 0 36 8 44) are both conflict-free.
constexpr int TE_RR = 72;
static_assert(TE_NP % 32 == 0 && TE_NP >= 77, "the P V contraction walks the keys 32 at a time");

__device__ __forceinline__ bf16x8 te_ld_frag(const uint16_t* p, bool ok) {
    bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return ok ? *reinterpret_cast<const bf16x8*>(p) : z;
}

__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ tok_emb,
                                                         const float* __restrict__ pos_emb, int L, int W, int vocab, float* __restrict__ x,
                                                         int32_t* __restrict__ eot) {
    const int row = blockIdx.x, b = row / L, l = row - b * L, tid = threadIdx.x;
    const int64_t tok = tokens[row];
    const bool ok = tok >= 0 && tok < vocab;                 // the host refused such a row already: no read outside the table in any case
    const float* te = tok_emb + (ok ? tok : 0) * (int64_t)W;
    for (int c = tid; c < W; c += 256) x[(int64_t)row * W + c] = ok ? te[c] + pos_emb[(int64_t)l * W + c] : 0.0f;
    if (l == 0 && tid < 64) {                                // text.argmax(dim=-1): the FIRST index of the row's maximum, by wave 0
        int64_t bv = INT64_MIN;
        int best = L;
        for (int j = tid; j < L; j += 64) {                  // ascending j per lane: a strict > keeps the lane's first maximum
            const int64_t v = tokens[row + j];
            if (v > bv || best == L) { bv = v; best = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t ov = __shfl_xor(bv, o);
            const int ob = __shfl_xor(best, o);
            if (ov > bv || (ov == bv && ob < best)) { bv = ov; best = ob; }
        }
        if (tid == 0) eot[b] = best;
    }
}

__global__ __launch_bounds__(TE_NT * 64) void causal_attn_fwd_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, int L, int nH) {
    __shared__ __attribute__((aligned(16))) uint16_t Ks[TE_NP * TE_RR];
    __shared__ __attribute__((aligned(16))) uint16_t Vs[TE_NP * TE_RR];
    const int b = blockIdx.x / nH, h = blockIdx.x - b * nH;
    const int C = nH * 64;
    const int64_t rowst = 3 * (int64_t)C;
    const uint16_t* base = qkv + (int64_t)b * L * rowst + h * 64;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, g = l >> 4, c16 = l & 15;
    const int qi = 16 * w + c16;
    const bool qok = qi < L;
    const int nw = nthreads >> 6;                            // ceil(L / 16) strips
    const int nrows = ((nw + 1) & ~1) * 16;                  // rows the P V contraction can touch (<= TE_NP), zero past L

    const bf16x8 qf0 = te_ld_frag(base + (int64_t)qi * rowst + 8 * g, qok);
    const bf16x8 qf1 = te_ld_frag(base + (int64_t)qi * rowst + 32 + 8 * g, qok);
    for (int u = tid; u < nrows * 8; u += nthreads) {        // 16-byte chunks: row u >> 3, chunk u & 7
        const int r = u >> 3, c = u & 7;
        const uint16_t* src = base + (int64_t)r * rowst + 8 * c;
        const bf16x8 kv = te_ld_frag(src + C, r < L), vv = te_ld_frag(src + 2 * C, r < L);
        *reinterpret_cast<bf16x8*>(&Ks[r * TE_RR + 8 * c]) = kv;
        *reinterpret_cast<bf16x8*>(&Vs[r * TE_RR + 8 * c]) = vv;
    }
    __syncthreads();

    const float scale2 = 0.125f * TE_LOG2E;                  // head_dim^-0.5 (a power of two: where it is applied does not matter)
    float p[TE_NT][4];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < TE_NT; ++kt) {
        if (kt <= w) {                                       // (uniform) tiles above the diagonal are never computed
            const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(&Ks[(16 * kt + c16) * TE_RR + 8 * g]);
            const bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(&Ks[(16 * kt + c16) * TE_RR + 32 + 8 * g]);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = mfma16(kf0, qf0, acc);                     // acc[r] = S^T[key 16kt+4g+r][query c16]
            acc = mfma16(kf1, qf1, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = (16 * kt + 4 * g + r <= qi) ? acc[r] * scale2 : -INFINITY;
                p[kt][r] = s;
                mx = fmaxf(mx, s);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) p[kt][r] = -INFINITY;
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));                      // key 0 is visible to every query: mx is finite
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < TE_NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(p[kt][r] - mx);
            p[kt][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;

    f32x4 o[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    DGX_LDS const uint16_t* v_l4 = tr_lane_ptr(Vs, TE_RR, 4 * g, 0, c16);
#pragma unroll
    for (int t = 0; t < TE_NT / 2; ++t) {
        if (2 * t <= w) {                                    // (uniform)
            const u32x4 pk = {pack_bf2(p[2 * t][0], p[2 * t][1]), pack_bf2(p[2 * t][2], p[2 * t][3]),
                              pack_bf2(p[2 * t + 1][0], p[2 * t + 1][1]), pack_bf2(p[2 * t + 1][2], p[2 * t + 1][3])};
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pk);   // slots (g, j): keys 32t+4g+j, 32t+16+4g+(j-4) of query c16
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)                   // o[dt][r] = O[query c16][d 16dt+4g+r]
                o[dt] = mfma16(tr_frag(v_l4, 32 * t * TE_RR + 16 * dt, (32 * t + 16) * TE_RR + 16 * dt), pf, o[dt]);
        }
    }
    if (qok) {
        uint16_t* orow = out + ((int64_t)b * L + qi) * C + h * 64 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<u32x2*>(orow + 16 * dt) = u32x2{pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv)};
    }
}

__global__ __launch_bounds__(256) void quick_gelu_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int64_t n) {
    const int64_t n8 = n >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        float v[8];
        ld8(x + 8 * i, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] * (1.0f / (1.0f + expf(-1.702f * v[j])));
        st8(y + 8 * i, v);
    }
    if (blockIdx.x == 0) {
        const int64_t i = 8 * n8 + threadIdx.x;              // the tail of a length that is no multiple of 8
        if (i < n) {
            const float v = bf2f(x[i]);
            y[i] = f2bf(v * (1.0f / (1.0f + expf(-1.702f * v))));
        }
    }
}

// sum of one float per thread over a workgroup of 256, in every thread (wave butterfly, then the four wave sums in a fixed order)
__device__ __forceinline__ float block_sum256(float v, float* red /* 4 */) {
    v = wave_sum(v);
    __syncthreads();                                         // (red may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void text_eot_project_kernel(const float* __restrict__ x, const int32_t* __restrict__ eot,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ proj, int L, int W, int E, float eps,
                                                               float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float row_s[];   // W: the normalised row
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int e0 = eot[b];
    e0 = e0 < 0 ? 0 : (e0 >= L ? L - 1 : e0);
    const float* row = x + ((int64_t)b * L + e0) * W;
    float s = 0.f;
    for (int c = tid; c < W; c += 256) s += row[c];
    const float mean = block_sum256(s, red) / (float)W;
    float ss = 0.f;
    for (int c = tid; c < W; c += 256) {
        const float d = row[c] - mean;
        ss += d * d;
    }
    const float rstd = 1.0f / sqrtf(block_sum256(ss, red) / (float)W + eps);
    for (int c = tid; c < W; c += 256) row_s[c] = (row[c] - mean) * rstd * gamma[c] + beta[c];
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
        float acc = 0.f;
        for (int c = 0; c < W; ++c) acc += row_s[c] * proj[(int64_t)c * E + e];      // ascending c, one addition at a time
        out[(int64_t)b * E + e] = acc;
    }
}

}  // namespace

extern "C" int dgx_text_embed(const int64_t* tokens_host, const int64_t* tokens, const float* token_embedding, const float* positional_embedding,
                              int B, int L, int W, int vocab, float* x, int32_t* eot, void* stream) {
    if (!tokens_host || !tokens || !token_embedding || !positional_embedding || !x || !eot || B <= 0 || L <= 0 || W <= 0 || vocab <= 0)
        return DGX_ERR_BAD_ARG;
    for (int64_t i = 0; i < (int64_t)B * L; ++i)
        if (tokens_host[i] < 0 || tokens_host[i] >= vocab) return DGX_ERR_BAD_ARG;
    hipLaunchKernelGGL(text_embed_kernel, dim3(B * L), dim3(256), 0, (hipStream_t)stream, tokens, token_embedding, positional_embedding, L, W,
                       vocab, x, eot);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_causal_attention_fwd(const void* qkv, void* out, int B, int L, int nH, void* stream) {
    if (!qkv || !out || B <= 0 || nH <= 0 || L < 1 || L > DGX_TEXT_MAX_L) return DGX_ERR_BAD_ARG;
    const int nw = (L + 15) / 16;
    hipLaunchKernelGGL(causal_attn_fwd_kernel, dim3(B * nH), dim3(nw * 64), 0, (hipStream_t)stream, (const uint16_t*)qkv, (uint16_t*)out, L, nH);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_quick_gelu(const void* x, void* y, int64_t n, void* stream) {
    if (n <= 0) return DGX_OK;
    if (!x || !y) return DGX_ERR_BAD_ARG;
    const int64_t blocks = ((n >> 3) + 255) / 256;
    const int grid = (int)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
    hipLaunchKernelGGL(quick_gelu_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (uint16_t*)y, n);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_text_eot_project(const float* x, const int32_t* eot, const float* ln_weight, const float* ln_bias, const float* projection,
                                    int B, int L, int W, int E, float eps, float* out, void* stream) {
    if (!x || !eot || !ln_weight || !ln_bias || !projection || !out || B <= 0 || L <= 0 || W <= 0 || E <= 0) return DGX_ERR_BAD_ARG;
    if ((size_t)W * 4 > 48 * 1024) return DGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(text_eot_project_kernel, dim3(B), dim3(256), (size_t)W * 4, (hipStream_t)stream, x, eot, ln_weight, ln_bias, projection,
                       L, W, E, eps, out);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
