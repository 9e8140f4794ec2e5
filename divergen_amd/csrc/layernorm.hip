// Fused LayerNorm for the Swin blocks (gfx950).  HBM-bound: one wave per token row, 16-byte lanes.
//   forward : x fp32 (T,C) -> y bf16, optionally written straight in WINDOW order (zero rows for the
//             padding tokens): LayerNorm + bf16 cast + pad + roll + window_partition in one pass
//             (reads 4 B, writes 2 B per element) instead of LN (4+4) + cast (4+2) + gather (2+2).
//   backward: dy bf16 (window order when gathered) + x + (mean, rstd) -> dx fp32, and per-block partial
//             sums of dgamma / dbeta (a second tiny pass adds them into the gradient arena).
// Reference semantics: nn.LayerNorm at swintransformer.py:213,255 followed by :216-233.
#include "dgx_common.h"
#include "winmap.h"
#include <type_traits>

// behind `m.ws ? .. : row`: classic or compact window order; a compact y / emit buffer of the forward keeps its padding rows
constexpr int LN_ORDERS = WM_CLASSIC | WM_COMPACT_TAIL;

// One row in three passes over its source (sum, centred sum of squares, normalise): the form for rows too wide for the registers.
// col(i): float4 column i of the row.
template <typename YT, class F>
__device__ __forceinline__ void ln_row_3pass(F col, const float4* __restrict__ g4, const float4* __restrict__ b4, YT* __restrict__ yo,
                                             float* __restrict__ mean, float* __restrict__ rstd, int C, float eps, int lane) {
    float s = 0.f;
    for (int i = lane; i < C / 4; i += 64) { const float4 v = col(i); s += (v.x + v.y) + (v.z + v.w); }
    const float mu = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int i = lane; i < C / 4; i += 64) {
        const float4 v = col(i);
        const float a = v.x - mu, b = v.y - mu, c = v.z - mu, d = v.w - mu;
        q += (a * a + b * b) + (c * c + d * d);
    }
    const float rs = rsqrtf(wave_sum(q) / (float)C + eps);
    if (lane == 0) { *mean = mu; *rstd = rs; }
    for (int i = lane; i < C / 4; i += 64) {
        const float4 v = col(i), g = g4[i], b = b4[i];
        st4(yo, i, make_float4((v.x - mu) * rs * g.x + b.x, (v.y - mu) * rs * g.y + b.y,
                               (v.z - mu) * rs * g.z + b.z, (v.w - mu) * rs * g.w + b.w));
    }
}

// NJ = ceil(C/256) float4 columns per lane: the row is read ONCE into registers (mean, centred variance and the output all
// come from them); NJ == 0 is the generic three-pass form for rows wider than 1536.
template <typename XT, typename YT = uint16_t, int NJ = 0>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const XT* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, YT* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int64_t T_out,
                                                     int C, float eps, WmMap m) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
    if constexpr (NJ > 0) {
        // Two rows per trip, EVERY load of the trip in flight before anything is consumed: the rows as raw bits (no conversion, no
        // select next to the load: round 5 found each `i < C/4 ? ld4(...) : 0` compiled to load + s_waitcnt vmcnt(0) in its own
        // predicated block -- six memory latencies in series per trip on a kernel that should be ONE latency long), gamma and beta
        // with them; out-of-row lanes read the row's last quad (clamped index) and are masked where the value is used.
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const int wave32 = (int)blockIdx.x * 4 + wv, nwaves32 = (int)gridDim.x * 4, T32 = (int)T_out, nq = C / 4;
        constexpr int NJ1 = NJ > 0 ? NJ : 1;
        float4 gv[NJ1], bv[NJ1];
        bool in[NJ1];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = lane + 64 * j;
            in[j] = i < nq;
            gv[j] = g4[in[j] ? i : nq - 1];
            bv[j] = b4[in[j] ? i : nq - 1];
        }
        for (int orow0 = wave32; orow0 < T32; orow0 += 2 * nwaves32) {
            typename Raw4<XT>::type raw[2][NJ1];
            int toks[2];
            const int orows[2] = {orow0, orow0 + nwaves32};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                toks[u] = orows[u] < T32 ? (m.ws ? wm_row_token<int, LN_ORDERS>(m, orows[u]) : orows[u]) : -2;      // -1: padding row, -2: no row
                toks[u] = __builtin_amdgcn_readfirstlane(toks[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) raw[u][j] = Raw4<XT>::zero();
                if (toks[u] >= 0) {
                    const XT* xr = x + (int64_t)toks[u] * C;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) raw[u][j] = Raw4<XT>::ld(xr, in[j] ? lane + 64 * j : nq - 1);
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // the loads stay together, in front of every use
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (toks[u] == -2) continue;
                YT* yo = y + (int64_t)orows[u] * C;
                if (toks[u] < 0) {
                    for (int i = lane; i < nq; i += 64) st4(yo, i, make_float4(0.f, 0.f, 0.f, 0.f));
                    continue;
                }
                float4 v[NJ1];
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    v[j] = Raw4<XT>::f(raw[u][j]);
                    if (!in[j]) v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
                }
                const float mu = wave_sum(s) / (float)C;
                float q = 0.f;
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (in[j]) {
                        const float a = v[j].x - mu, b = v[j].y - mu, c = v[j].z - mu, d = v[j].w - mu;
                        q += (a * a + b * b) + (c * c + d * d);
                    }
                const float rs = rsqrtf(wave_sum(q) / (float)C + eps);
                if (lane == 0) { mean[toks[u]] = mu; rstd[toks[u]] = rs; }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int i = lane + 64 * j;
                    if (in[j]) {
                        const float4 g = gv[j], b = bv[j];
                        st4(yo, i, make_float4((v[j].x - mu) * rs * g.x + b.x, (v[j].y - mu) * rs * g.y + b.y,
                                                   (v[j].z - mu) * rs * g.z + b.z, (v[j].w - mu) * rs * g.w + b.w));
                    }
                }
            }
        }
        return;
    }
    for (int64_t orow = wave; orow < T_out; orow += nwaves) {
        const int64_t tok = m.ws ? wm_row_token<int64_t, LN_ORDERS>(m, orow) : orow;
        YT* yo = y + orow * C;
        if (tok < 0) {
            for (int i = lane; i < C / 4; i += 64) st4(yo, i, make_float4(0.f, 0.f, 0.f, 0.f));
            continue;
        }
        const XT* xr = x + tok * C;
        ln_row_3pass([&](int i) { return ld4<XT>(xr, i); }, g4, b4, yo, mean + tok, rstd + tok, C, eps, lane);
    }
}

constexpr int LNB_WAVES = 8;          // waves per backward workgroup: one partial row of (dgamma | dbeta) per workgroup
// Block partials: the waves fold their (dgamma | dbeta) registers into one LDS row in turn -> one row of `part` per block: [block][2][C]
// (tried: every wave into its own LDS row + one barrier -- 49 KB of LDS per workgroup cost more occupancy than the seven barriers:
// 16.1 -> 22.3 us)
template <int NJ, int WAVES>
__device__ __forceinline__ void ln_fold_part(const float (&dg)[NJ][4], const float (&db)[NJ][4], float* __restrict__ part, int C, int lane, int w) {
    __shared__ float red[2][NJ * 256];
    for (int turn = 0; turn < WAVES; ++turn) {
        if (w == turn) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = (lane + 64 * j) * 4 + k;
                    red[0][c] = turn ? red[0][c] + dg[j][k] : dg[j][k];
                    red[1][c] = turn ? red[1][c] + db[j][k] : db[j][k];
                }
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < C; c += 64 * WAVES) {
        part[((int64_t)blockIdx.x * 2 + 0) * C + c] = red[0][c];
        part[((int64_t)blockIdx.x * 2 + 1) * C + c] = red[1][c];
    }
}

// NJ = ceil(C/256): float4 columns per lane
// EMIT (dgx_layernorm_bwd_emit): the kernel also writes  emit[row(tok)] = bf16(escale[b] * dx[tok])  -- the operand of the NEXT
// GEMM of the backward pass -- in token order (em.ws == 0) or in window order (zero rows for the padding tokens), i.e. what a
// separate dgx_residual_bwd pass over dx produced before (one read of dx and one launch less per use).  The value is formed from
// dx AS STORED (rounded to its dtype first), so the two-kernel path gives the same bits.
template <int NJ, typename XT, typename DT = uint16_t, bool EMIT = false>
__global__ __launch_bounds__(64 * LNB_WAVES, ((NJ <= 2 || (NJ == 3 && sizeof(XT) == 2)) ? 4 : 2)) void ln_bwd_kernel(const DT* __restrict__ dy, const XT* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const XT* dres, XT* dx,
                                                     float* __restrict__ part, int64_t T, int C, WmMap m,
                                                     uint16_t* __restrict__ emit = nullptr, const float* __restrict__ escale = nullptr,
                                                     WmMap em = WmMap{0, 0, 0, 0, 0, 0, 0, 0}) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t wave = (int64_t)blockIdx.x * LNB_WAVES + w;
    const int64_t nwaves = (int64_t)gridDim.x * LNB_WAVES;
    float dg[NJ][4], db[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) dg[j][k] = db[j][k] = 0.f;
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    // two rows per trip: both rows' loads are in flight before the first row's reductions (T / waves = 2 rows per wave at
    // Swin-L stage 2: one memory latency per launch instead of two on a 16 us kernel)
    // Row / token indices are wave-uniform and far below 2^31: 32-bit scalar arithmetic (the 64-bit divisions of the window map were
    // ~150 VALU instructions per row and map).
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wave32 = (int)blockIdx.x * LNB_WAVES + wv, nwaves32 = (int)gridDim.x * LNB_WAVES, T32 = (int)T, nq = C / 4;
    bool in[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) in[j] = lane + 64 * j < nq;
    for (int tok0 = wave32; tok0 < T32; tok0 += 2 * nwaves32) {
        // The two rows stay in registers AS LOADED (packed: 6 registers per bf16 quad for x, dy and the residual-branch gradient).
        // EVERY load of the trip -- both rows' statistics, their 3 x NJ quads each, gamma -- is issued before anything is consumed
        // (round 5: the compiler had waited for row 0 before requesting row 1 and re-requested gamma in front of each use: ~8 exposed
        // L2 / HBM latencies per trip on a kernel that is one trip long).  x_hat and dy * gamma are formed twice, for the sums and for
        // the result, by the same operations.
        typename Raw4<XT>::type xr_[2][NJ], rr_[2][NJ];
        typename Raw4<DT>::type dr_[2][NJ];
        float4 gq[NJ];
        float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f}, rsv[2] = {0.f, 0.f}, muv[2] = {0.f, 0.f};
        const int toks[2] = {tok0, tok0 + nwaves32};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) { xr_[u][j] = Raw4<XT>::zero(); dr_[u][j] = Raw4<DT>::zero(); rr_[u][j] = Raw4<XT>::zero(); }
            const int tok = toks[u];
            if (tok >= T32) continue;
            const int drow = __builtin_amdgcn_readfirstlane(m.ws ? wm_token_row<int, LN_ORDERS>(m, tok) : tok);
            const DT* dyr = dy + (int64_t)drow * C;
            const XT* xr = x + (int64_t)tok * C;
            const XT* drr0 = dres ? dres + (int64_t)tok * C : nullptr;
            muv[u] = mean[tok];
            rsv[u] = rstd[tok];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = in[j] ? lane + 64 * j : nq - 1;        // out-of-row lanes re-read the last quad and are masked at the uses
                xr_[u][j] = Raw4<XT>::ld(xr, i);
                dr_[u][j] = Raw4<DT>::ld(dyr, i);
                if (drr0) rr_[u][j] = Raw4<XT>::ld(drr0, i);
            }
        }
        __builtin_amdgcn_sched_barrier(0);      // (gamma behind the rows: an L2 hit, it lands first anyway)
#pragma unroll
        for (int j = 0; j < NJ; ++j) gq[j] = g4[in[j] ? lane + 64 * j : nq - 1];
        __builtin_amdgcn_sched_barrier(0);      // the loads stay together, in front of every use
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (toks[u] >= T32) continue;
            const float mu = muv[u], rs = rsv[u];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (in[j]) {
                    const float4 v = Raw4<XT>::f(xr_[u][j]), g = gq[j], d4 = Raw4<DT>::f(dr_[u][j]);
                    const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
                    const float xv[4] = {v.x, v.y, v.z, v.w}, gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float xh = (xv[k] - mu) * rs, gv = dv[k] * gg[k];
                        s1[u] += gv;
                        s2[u] += gv * xh;
                        dg[j][k] += dv[k] * xh;
                        db[j][k] += dv[k];
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tok = toks[u];
            if (tok >= T32) continue;
            const float a1 = wave_sum(s1[u]) / (float)C, a2 = wave_sum(s2[u]) / (float)C, rs = rsv[u], mu = muv[u];
            XT* dxr = dx + (int64_t)tok * C;
            uint16_t* er = nullptr;
            float es = 1.0f;
            if (EMIT) {
                er = emit + (int64_t)__builtin_amdgcn_readfirstlane(em.ws ? wm_token_row<int, LN_ORDERS>(em, tok) : tok) * C;
                if (escale) es = escale[tok / (em.H * em.W)];
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = lane + 64 * j;
                if (in[j]) {
                    const float4 v = Raw4<XT>::f(xr_[u][j]), g = gq[j], d4 = Raw4<DT>::f(dr_[u][j]);
                    const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
                    const float xv[4] = {v.x, v.y, v.z, v.w}, gg[4] = {g.x, g.y, g.z, g.w};
                    float ov[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float xh = (xv[k] - mu) * rs, gv = dv[k] * gg[k];
                        ov[k] = rs * (gv - a1 - xh * a2);
                    }
                    float4 o = make_float4(ov[0], ov[1], ov[2], ov[3]);
                    if (dres) {                // gradient arriving on the residual branch (may alias dx: read above, before this store)
                        const float4 a = Raw4<XT>::f(rr_[u][j]);
                        o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
                    }
                    st4(dxr, i, o);
                    if (EMIT) {
                        const float4 r = rnd4<XT>(o);     // dx as stored
                        st4(er, i, make_float4(es * r.x, es * r.y, es * r.z, es * r.w));
                    }
                }
            }
        }
    }
    if (EMIT && em.ws && !em.compact) {        // classic window order: the rows of the padding tokens are zero (the compact emit buffer has none)
        const int64_t rows = wm_classic_rows(em);
        if (rows != T)
            for (int64_t orow = wave; orow < rows; orow += nwaves)
                if (wm_row_token<int64_t, LN_ORDERS>(em, orow) < 0)
                    for (int i = lane; i < C / 4; i += 64) st4(emit + orow * C, i, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    ln_fold_part<NJ, LNB_WAVES>(dg, db, part, C, lane, w);
}

// Second stage: dgamma += sum_blocks part[b][0], dbeta += sum_blocks part[b][1], for up to 16 norms of the same T and C in ONE launch
// (blockIdx.y: the norm -- the two norms of up to eight consecutive Swin blocks of a stage).
// block = LNR_QB float4 column-quads x LNR_RG row groups (1024 threads): 256 B contiguous per row read.  Round 2 used 64 quads x 16
// row groups: 6 workgroups for a C = 768 norm -- the whole second stage ran on 6 (12 for two norms) of the 256 CUs, 10.7 us for
// 6 MB; 16 quads x 64 row groups are 24 (48) workgroups.  Summation order (per norm, whatever the number of norms in the launch, so
// every form of the second stage is bit-identical): row group rg takes rows rg, rg + 64, ...; eight threads fold eight groups each,
// the first folds those eight.
constexpr int LNR_QB = 16, LNR_RG = 64, LNR_MAXN = 16;
struct LnRedN { const float* part[LNR_MAXN]; float* dgamma[LNR_MAXN]; float* dbeta[LNR_MAXN]; };
__global__ __launch_bounds__(1024) void ln_param_reduce_kernel(LnRedN R, int nblk, int C) {
    __shared__ float4 red[LNR_RG][LNR_QB];
    const float* part = R.part[0];
    float* dgamma = R.dgamma[0];
    float* dbeta = R.dbeta[0];
#pragma unroll
    for (int k = 1; k < LNR_MAXN; ++k)       // constant indices into the by-value table: a dynamic one would go through private memory
        if ((int)blockIdx.y == k) { part = R.part[k]; dgamma = R.dgamma[k]; dbeta = R.dbeta[k]; }
    const int lane = threadIdx.x % LNR_QB, rg = threadIdx.x / LNR_QB;
    const int q = blockIdx.x * LNR_QB + lane;          // float4 index inside the 2*C-wide partial row
    const int nq = 2 * C / 4;
    float4 s = {0.f, 0.f, 0.f, 0.f};
    if (q < nq) {
        const float4* p4 = reinterpret_cast<const float4*>(part);
#pragma unroll 4
        for (int b = rg; b < nblk; b += LNR_RG) {
            const float4 v = p4[(int64_t)b * nq + q];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[rg][lane] = s;
    __syncthreads();
    if (rg < 8) {
        float4 a = red[8 * rg][lane];
#pragma unroll
        for (int r = 1; r < 8; ++r) { const float4 v = red[8 * rg + r][lane]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
        s = a;
    }
    __syncthreads();
    if (rg < 8) red[rg][lane] = s;
    __syncthreads();
    if (rg == 0 && q < nq) {
        float4 a = red[0][lane];
#pragma unroll
        for (int r = 1; r < 8; ++r) { const float4 v = red[r][lane]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
        // the partial row is [dgamma(C) | dbeta(C)]; C % 4 == 0 so a quad never straddles the two
        float* dst = (4 * q < C) ? dgamma + 4 * q : dbeta + (4 * q - C);
        dst[0] += a.x; dst[1] += a.y; dst[2] += a.z; dst[3] += a.w;
    }
}
// n <= LNR_MAXN norms, nblk partial rows each; the unused entries of the table repeat norm 0 (never selected)
static void ln_param_reduce(const float* const* parts, float* const* dgammas, float* const* dbetas, int n, int nblk, int C, hipStream_t st) {
    LnRedN R;
    for (int k = 0; k < LNR_MAXN; ++k) {
        const int j = k < n ? k : 0;
        R.part[k] = parts[j]; R.dgamma[k] = dgammas[j]; R.dbeta[k] = dbetas[j];
    }
    hipLaunchKernelGGL(ln_param_reduce_kernel, dim3((2 * C / 4 + LNR_QB - 1) / LNR_QB, n), dim3(1024), 0, st, R, nblk, C);
}

// Host dispatch, in the style of g_with_mc (gemm_common.h): calls f(integral_constant<int, NJ>, XT()) with the first NJ of the
// ladder NJS that holds nj columns per lane (the last one takes whatever is left: the widest form, or 0 for the generic one) and XT
// the storage type of x_dtype.  Each entry point names the ladder it has kernels for.
template <int N0, int... NJS, class F> int ln_with_nj(int nj, int x_dtype, F&& f) {
    if constexpr (sizeof...(NJS) > 0)
        if (nj > N0) return ln_with_nj<NJS...>(nj, x_dtype, f);
    return x_dtype == DGX_BF16 ? f(std::integral_constant<int, N0>{}, uint16_t()) : f(std::integral_constant<int, N0>{}, float());
}

// y in YT; T_out rows (window order: the padding tokens' rows included, all zero)
template <typename YT>
static int ln_fwd_launch(const void* x, const float* gamma, const float* beta, YT* y, float* mean, float* rstd, int64_t T_out, int C, float eps,
                         const WmMap& m, int x_dtype, int grid, void* stream) {
    return ln_with_nj<1, 2, 3, 6, 0>((C + 255) / 256, x_dtype, [&](auto NJ, auto xt) {
        using XT = decltype(xt);
        hipLaunchKernelGGL((ln_fwd_kernel<XT, YT, decltype(NJ)::value>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const XT*)x, gamma, beta, y, mean, rstd,
                           T_out, C, eps, m);
        return DGX_OK;
    });
}

extern "C" int dgx_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                 float* rstd, int64_t T, int C, float eps, int B, int H, int W, int ws, int shift,
                                 int x_dtype, void* stream) {
    if (T <= 0) return DGX_OK;
    if (!x || !gamma || !beta || !y_bf16 || !mean || !rstd || (C & 3) || !(ws == 0 || wm_map_ok(B, H, W, ws, shift, WM_CLASSIC | WM_COMPACT, T)))
        return DGX_ERR_BAD_ARG;
    const WmMap m = wm_map(B, H, W, ws, shift);
    // (compact as well: the output keeps the padding rows, all zero, behind the real ones -- the qkv weight gradient's operand)
    const int64_t T_out = m.ws > 0 ? wm_classic_rows(m) : T;
    if (T_out + 16384 >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;      // 32-bit row arithmetic in the kernels
    const int nj = (C + 255) / 256;
    const int64_t per_wg = nj <= 6 ? 8 : 4;       // rows per workgroup and trip: 4 waves x 2 rows (register-resident rows)
    const int grid = (int)((T_out + per_wg - 1) / per_wg < 8192 ? (T_out + per_wg - 1) / per_wg : 8192);
    ln_fwd_launch(x, gamma, beta, (uint16_t*)y_bf16, mean, rstd, T_out, C, eps, m, x_dtype, grid, stream);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_layernorm_bwd_blocks(int64_t T) {
    int64_t b = (T + LNB_WAVES - 1) / LNB_WAVES;
    return (int)(b < 512 ? (b < 1 ? 1 : b) : 512);
}

// the identity map: ws == 0, the geometry unused
static const WmMap LN_NO_MAP = {0, 0, 0, 0, 0, 0, 0, 0};

static int ln_bwd_launch(const void* dy_bf16, const void* x, const float* mean, const float* rstd, const float* gamma, const void* dres,
                         void* dx, float* dgamma, float* dbeta, float* part, int64_t T, int C, int B, int H, int W, int ws, int shift,
                         int x_dtype, void* emit, const float* escale, int eB, int eH, int eW, int ews, int eshift, void* stream) {
    if (T <= 0) return DGX_OK;
    if (!dy_bf16 || !x || !mean || !rstd || !gamma || !dx || ((dgamma == nullptr) != (dbeta == nullptr)) || !part || (C & 3) || C > 1536 ||
        !(ws == 0 || wm_map_ok(B, H, W, ws, shift, WM_CLASSIC | WM_COMPACT, T)))
        return DGX_ERR_BAD_ARG;
    // (the emit geometry carries the tokens even in token order: escale is per image)
    if (emit && ((int64_t)eB * eH * eW != T || !(ews == 0 || wm_map_ok(eB, eH, eW, ews, eshift, WM_CLASSIC | WM_COMPACT, T)))) return DGX_ERR_BAD_ARG;
    if (T + 16384 >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;          // 32-bit row / token arithmetic in the kernels
    const WmMap m = wm_map(B, H, W, ws, shift);
    const WmMap em = emit ? wm_map(eB, eH, eW, ews, eshift) : LN_NO_MAP;
    const int grid = dgx_layernorm_bwd_blocks(T);
    hipStream_t st = (hipStream_t)stream;
    auto go = [&](auto NJ, auto xt, auto E) {
        using XT = decltype(xt);
        hipLaunchKernelGGL((ln_bwd_kernel<decltype(NJ)::value, XT, uint16_t, decltype(E)::value>), dim3(grid), dim3(64 * LNB_WAVES), 0, st, (const uint16_t*)dy_bf16, (const XT*)x,
                           mean, rstd, gamma, (const XT*)dres, (XT*)dx, part, T, C, m, (uint16_t*)emit, escale, em);
        return DGX_OK;
    };
    ln_with_nj<1, 2, 3, 6>((C + 255) / 256, x_dtype,
                           [&](auto NJ, auto xt) { return emit ? go(NJ, xt, std::true_type{}) : go(NJ, xt, std::false_type{}); });
    // dgamma == dbeta == NULL: the per-block partial rows stay in `part` for dgx_layernorm_param_reduce2 / _n (several norms, one launch)
    if (dgamma) ln_param_reduce(&part, &dgamma, &dbeta, 1, grid, C, st);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_layernorm_bwd(const void* dy_bf16, const void* x, const float* mean, const float* rstd,
                                 const float* gamma, const void* dres, void* dx, float* dgamma, float* dbeta, float* part,
                                 int64_t T, int C, int B, int H, int W, int ws, int shift, int x_dtype, void* stream) {
    return ln_bwd_launch(dy_bf16, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, part, T, C, B, H, W, ws, shift, x_dtype, nullptr, nullptr,
                         0, 0, 0, 0, 0, stream);
}

extern "C" int dgx_layernorm_bwd_emit(const void* dy_bf16, const void* x, const float* mean, const float* rstd, const float* gamma,
                                      const void* dres, void* dx, float* dgamma, float* dbeta, float* part, int64_t T, int C, int B,
                                      int H, int W, int ws, int shift, int x_dtype, void* emit_bf16, const float* emit_scale, int eB,
                                      int eH, int eW, int ews, int eshift, void* stream) {
    if (!emit_bf16) return DGX_ERR_BAD_ARG;
    return ln_bwd_launch(dy_bf16, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, part, T, C, B, H, W, ws, shift, x_dtype, emit_bf16,
                         emit_scale, eB, eH, eW, ews, eshift, stream);
}

// The second stage of TWO dgx_layernorm_bwd calls made with dgamma = dbeta = NULL (same T, hence the same number of partial
// rows, and the same C): dgamma_x += sum of part_x's rows, in the fixed order of the single-norm form (bit-identical).
extern "C" int dgx_layernorm_param_reduce2(const float* part_a, float* dgamma_a, float* dbeta_a, const float* part_b, float* dgamma_b,
                                           float* dbeta_b, int64_t T, int C, void* stream) {
    if (T <= 0) return DGX_OK;
    if (!part_a || !dgamma_a || !dbeta_a || !part_b || !dgamma_b || !dbeta_b || (C & 3) || C > 1536) return DGX_ERR_BAD_ARG;
    const float* parts[2] = {part_a, part_b};
    float* dgammas[2] = {dgamma_a, dgamma_b};
    float* dbetas[2] = {dbeta_a, dbeta_b};
    ln_param_reduce(parts, dgammas, dbetas, 2, dgx_layernorm_bwd_blocks(T), C, (hipStream_t)stream);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

// The second stage of up to 16 norms in ONE launch; entries: part / dgamma / dbeta pointer triples.
extern "C" int dgx_layernorm_param_reduce_n(const float* const* parts, float* const* dgammas, float* const* dbetas, int n, int64_t T, int C,
                                            void* stream) {
    if (T <= 0 || n <= 0) return DGX_OK;
    if (!parts || !dgammas || !dbetas || n > LNR_MAXN || (C & 3) || C > 1536) return DGX_ERR_BAD_ARG;
    for (int k = 0; k < n; ++k)
        if (!parts[k] || !dgammas[k] || !dbetas[k]) return DGX_ERR_BAD_ARG;
    ln_param_reduce(parts, dgammas, dbetas, n, dgx_layernorm_bwd_blocks(T), C, (hipStream_t)stream);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

// ------------------------------------------------------------------------------------------------
// PatchMerging front half (swintransformer.py:272-298): zero-pad to even H/W, gather the 2x2 neighbourhood
// [x(2i,2j) | x(2i+1,2j) | x(2i,2j+1) | x(2i+1,2j+1)] into one 4*C0-wide row and LayerNorm it -- in ONE pass over x,
// bf16 out (the operand of the reduction GEMM).  The reference materialises four strided slices, their concatenation and
// an fp32 LayerNorm; its backward zero-fills and adds four full-size tensors.  Here every element of x is read once in
// the forward and every element of dx written once in the backward.
struct MergeMap { int B, H, W, H2, W2, C0; };

// float4 column i (of 4*C0/4) of merged row (b, i2, j2) -> source float4 pointer index, or -1 in the zero padding
__device__ __forceinline__ int64_t merge_src4(const MergeMap& m, int b, int i2, int j2, int i, int q0) {
    const int seg = i / q0, wi = i - seg * q0;
    const int y = 2 * i2 + (seg & 1), x = 2 * j2 + (seg >> 1);
    if (y >= m.H || x >= m.W) return -1;
    return (((int64_t)b * m.H + y) * m.W + x) * q0 + wi;
}
template <typename T> __device__ __forceinline__ float4 ld4q(const T* base, int64_t q) {
    if (q < 0) return make_float4(0.f, 0.f, 0.f, 0.f);
    return ld4<T>(base + q * 4, 0);
}

template <typename XT>
__global__ __launch_bounds__(256) void pm_ln_fwd_kernel(const XT* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, uint16_t* __restrict__ y,
                                                        float* __restrict__ mean, float* __restrict__ rstd, float eps,
                                                        MergeMap m) {
    const int lane = threadIdx.x & 63;
    const int C = 4 * m.C0, q0 = m.C0 / 4;
    const int64_t T2 = (int64_t)m.B * m.H2 * m.W2;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave; row < T2; row += nwaves) {
        const int j2 = (int)(row % m.W2), i2 = (int)((row / m.W2) % m.H2), b = (int)(row / ((int64_t)m.W2 * m.H2));
        ln_row_3pass([&](int i) { return ld4q<XT>(x, merge_src4(m, b, i2, j2, i, q0)); }, reinterpret_cast<const float4*>(gamma),
                     reinterpret_cast<const float4*>(beta), y + row * C, mean + row, rstd + row, C, eps, lane);
    }
}

// NJ = ceil(4*C0/256) float4 columns per lane; same reduction layout as ln_bwd_kernel (part: [block][2][C])
// WAVES: waves per workgroup (4 for the 3072-wide case, whose 200 live registers do not fit an 8-wave workgroup)
template <int NJ, typename XT, int WAVES = LNB_WAVES>
__global__ __launch_bounds__(64 * WAVES) void pm_ln_bwd_kernel(const uint16_t* __restrict__ dy, const XT* __restrict__ x,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, XT* __restrict__ dx,
                                                        float* __restrict__ part, MergeMap m) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int C = 4 * m.C0, q0 = m.C0 / 4;
    const int64_t T2 = (int64_t)m.B * m.H2 * m.W2;
    const int64_t wave = (int64_t)blockIdx.x * WAVES + w, nwaves = (int64_t)gridDim.x * WAVES;
    float dg[NJ][4], db[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) dg[j][k] = db[j][k] = 0.f;
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    for (int64_t row = wave; row < T2; row += nwaves) {
        const int j2 = (int)(row % m.W2), i2 = (int)((row / m.W2) % m.H2), b = (int)(row / ((int64_t)m.W2 * m.H2));
        const uint16_t* dyr = dy + row * C;
        const float mu = mean[row], rs = rstd[row];
        float xh[NJ][4], gv[NJ][4];
        int64_t src[NJ];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = lane + 64 * j;
            src[j] = -1;
            if (i < C / 4) {
                src[j] = merge_src4(m, b, i2, j2, i, q0);
                const float4 v = ld4q<XT>(x, src[j]), g = g4[i], d4 = ld4<uint16_t>(dyr, i);
                const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
                const float xv[4] = {v.x, v.y, v.z, v.w}, gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    xh[j][k] = (xv[k] - mu) * rs;
                    gv[j][k] = dv[k] * gg[k];
                    s1 += gv[j][k];
                    s2 += gv[j][k] * xh[j][k];
                    dg[j][k] += dv[k] * xh[j][k];
                    db[j][k] += dv[k];
                }
            }
        }
        s1 = wave_sum(s1) / (float)C;
        s2 = wave_sum(s2) / (float)C;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (src[j] >= 0)
                st4(dx + src[j] * 4, 0,
                    make_float4(rs * (gv[j][0] - s1 - xh[j][0] * s2), rs * (gv[j][1] - s1 - xh[j][1] * s2),
                                rs * (gv[j][2] - s1 - xh[j][2] * s2), rs * (gv[j][3] - s1 - xh[j][3] * s2)));
    }
    ln_fold_part<NJ, WAVES>(dg, db, part, C, lane, w);
}

static bool merge_args_ok(int B, int H, int W, int C0) { return B > 0 && H > 0 && W > 0 && C0 > 0 && (C0 & 3) == 0 && 4 * C0 <= 3072; }

extern "C" int dgx_patch_merge_ln_fwd(const void* x, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                      float* rstd, int B, int H, int W, int C0, float eps, int x_dtype, void* stream) {
    if (!x || !gamma || !beta || !y_bf16 || !mean || !rstd || !merge_args_ok(B, H, W, C0)) return DGX_ERR_BAD_ARG;
    const MergeMap m = {B, H, W, (H + 1) / 2, (W + 1) / 2, C0};
    const int64_t T2 = (int64_t)B * m.H2 * m.W2;
    const int grid = (int)((T2 + 3) / 4 < 8192 ? (T2 + 3) / 4 : 8192);
    ln_with_nj<0>(0, x_dtype, [&](auto, auto xt) {
        using XT = decltype(xt);
        hipLaunchKernelGGL(pm_ln_fwd_kernel<XT>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const XT*)x, gamma, beta, (uint16_t*)y_bf16,
                           mean, rstd, eps, m);
        return DGX_OK;
    });
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_patch_merge_ln_bwd(const void* dy_bf16, const void* x, const float* mean, const float* rstd,
                                      const float* gamma, void* dx, float* dgamma, float* dbeta, float* part, int B, int H,
                                      int W, int C0, int x_dtype, void* stream) {
    if (!dy_bf16 || !x || !mean || !rstd || !gamma || !dx || !dgamma || !dbeta || !part || !merge_args_ok(B, H, W, C0))
        return DGX_ERR_BAD_ARG;
    const MergeMap m = {B, H, W, (H + 1) / 2, (W + 1) / 2, C0};
    const int64_t T2 = (int64_t)B * m.H2 * m.W2;
    const int C = 4 * C0, grid = dgx_layernorm_bwd_blocks(T2);
    hipStream_t st = (hipStream_t)stream;
    ln_with_nj<2, 3, 6, 12>((C + 255) / 256, x_dtype, [&](auto NJ, auto xt) {
        using XT = decltype(xt);
        constexpr int WAVES = decltype(NJ)::value == 12 ? 4 : LNB_WAVES;
        hipLaunchKernelGGL((pm_ln_bwd_kernel<decltype(NJ)::value, XT, WAVES>), dim3(grid), dim3(64 * WAVES), 0, st, (const uint16_t*)dy_bf16,
                           (const XT*)x, mean, rstd, gamma, (XT*)dx, part, m);
        return DGX_OK;
    });
    ln_param_reduce(&part, &dgamma, &dbeta, 1, grid, C, st);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}


// LayerNorm with an fp32 result (PatchEmbed.norm, swintransformer.py:440-442: under autocast the reference's LayerNorm
// returns fp32 and that tensor IS the stage-0 residual stream).  x f32|bf16 (T,C) -> y f32; backward takes dy f32.
extern "C" int dgx_layernorm_f32out_fwd(const void* x, const float* gamma, const float* beta, float* y, float* mean,
                                        float* rstd, int64_t T, int C, float eps, int x_dtype, void* stream) {
    if (T <= 0) return DGX_OK;
    if (!x || !gamma || !beta || !y || !mean || !rstd || (C & 3)) return DGX_ERR_BAD_ARG;
    const int grid = (int)((T + 3) / 4 < 8192 ? (T + 3) / 4 : 8192);
    ln_fwd_launch(x, gamma, beta, y, mean, rstd, T, C, eps, LN_NO_MAP, x_dtype, grid, stream);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_layernorm_f32out_bwd(const float* dy, const void* x, const float* mean, const float* rstd,
                                        const float* gamma, void* dx, float* dgamma, float* dbeta, float* part, int64_t T,
                                        int C, int x_dtype, void* stream) {
    if (T <= 0) return DGX_OK;
    if (!dy || !x || !mean || !rstd || !gamma || !dx || !dgamma || !dbeta || !part || (C & 3) || C > 768) return DGX_ERR_BAD_ARG;
    const int grid = dgx_layernorm_bwd_blocks(T);
    hipStream_t st = (hipStream_t)stream;
    ln_with_nj<1, 2, 3>((C + 255) / 256, x_dtype, [&](auto NJ, auto xt) {
        using XT = decltype(xt);
        hipLaunchKernelGGL((ln_bwd_kernel<decltype(NJ)::value, XT, float>), dim3(grid), dim3(64 * LNB_WAVES), 0, st, dy, (const XT*)x, mean, rstd,
                           gamma, (const XT*)nullptr, (XT*)dx, part, T, C, LN_NO_MAP);
        return DGX_OK;
    });
    ln_param_reduce(&part, &dgamma, &dbeta, 1, grid, C, st);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
