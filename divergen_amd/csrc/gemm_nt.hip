// bf16 GEMM with fused epilogues for gfx950:  C[M][N] = epi( sum_k A[m][k] * B[n][k] ),  A (M,K), B (N,K) row-major
// (both operands K-contiguous: y = x W^T of nn.Linear as stored; the input gradient dx = dy W runs on the transposed
// weight image the optimizer step refreshes, so it is the same kernel).  Replaces the hipBLASLt calls behind
// torch.addmm / torch.mm at the Linear sites of the reference: swintransformer.py:133,155 (qkv / proj), :40-46 (Mlp),
// :296 (PatchMerging.reduction), fpn.py:126-154 (1x1 laterals), box_head.py:26-98 (FCs).
//
// Structure (one workgroup = one BM x BN output tile, 8 waves = 2 (M) x 4 (N), K-step 64):
//   * both operand tiles go global -> LDS with LDS-direct loads (`buffer_load_dwordx4 ... lds`, no staging registers):
//     one wave-instruction = 8 tile rows x 128 B = 8 whole cache lines; rows are 128 B in LDS, the 16-byte chunk index
//     is XOR-swizzled with (row >> 1) & 7 (applied to the per-lane SOURCE address, the LDS image of an instruction is
//     lane-linear), which makes every ds_read_b128 of an MFMA fragment (16 rows x one chunk column) bank-conflict free;
//   * two LDS stages; the 8 waves form two groups (waves 0-3 / 4-7 = one wave of each group per SIMD) that run the
//     same per-K-tile program {read all fragments of the tile into registers | 2*WMF*WNF MFMAs} one phase apart: while
//     one wave of a SIMD issues MFMAs back to back, its partner reads LDS and issues the loads of the tile after next.
//     A stage is re-filled as soon as both groups have read it and has ~two phases to land (counted only by vmcnt(0)
//     at the end of the phase before its first read; raw s_barrier, so LDS-direct loads stay in flight across barriers);
//   * MFMA operands are swapped (D = W-fragment x X-fragment) so that a lane holds 4 CONSECUTIVE output columns of one
//     row: the epilogue packs them to bf16, stages the whole tile in LDS (stage buffers are idle by then) and streams
//     it out as whole rows, 16 B per lane, with the fused tail (bias | bias + exact GELU with both tensors written |
//     bias + window_reverse/roll/crop + DropPath + residual add | multiply by GELU'(f1)) applied on the way out;
//   * XCD-aware tile order: workgroups of one XCD (blockIdx % 8) take consecutive tiles = the same A row-panel.
#include "gemm_common.h"
#include "dev_clock.h"
#include <stdio.h>
#include <string.h>

namespace {
template <int BM, int BN, int NS_> struct GemmCfg {
    static constexpr int NS = NS_;                 // LDS stages (K-tiles resident or in flight)
    static constexpr int WMF = BM / 32;            // 16-row MFMA fragments per wave along M (2 waves)
    static constexpr int WNF = BN / 64;            // 16-column fragments per wave along N (4 waves)
    static constexpr int NA = BM / 64;             // LDS-direct loads per wave per K-tile, A rows
    static constexpr int NB = BN / 64;             //                                      B rows
    static constexpr int SB = (BM + BN) * 128;     // bytes per stage
    static constexpr int SROW = BN * 2 + 16;       // epilogue staging row stride (bytes)
    static constexpr int EPI = BM * SROW + BM * 8; // staged tile + row -> (token, sample) table
    static constexpr int LDS = (NS * SB > EPI ? NS * SB : EPI);
};
}  // namespace

// MC >= 0: the fused tail is a compile-time constant (2: bias + GELU, 3 / 6: bf16 / fp32 residual, 4: x GELU'(f1)), as in gemm_lw --
// the two-workgroup instantiation that runs the K <= 768 fused-tail GEMMs (why: g_fix_mode).  MC = -1: run-time mode.
template <int BM, int BN, int NS, int MINW, int MC = -1>
__global__ __launch_bounds__(512, MINW) void gemm_nt_kernel(GemmP P) {
    g_fix_mode<MC>(P);
    using Cfg = GemmCfg<BM, BN, NS>;
    constexpr int NL = Cfg::NA + Cfg::NB;          // LDS-direct loads per wave per K-tile
    constexpr int WMF = Cfg::WMF, WNF = Cfg::WNF, NA = Cfg::NA, NB = Cfg::NB, SB = Cfg::SB, SROW = Cfg::SROW;
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds_raw[];
    const int L0 = (blockIdx.x & 7) * P.per_xcd + (blockIdx.x >> 3);
    if (L0 >= P.total * P.splits) return;
    int L = L0 / P.splits;
    const int split = L0 - L * P.splits;           // the splits of a tile are neighbours on one XCD
    if (P.ngrp > 0) {                              // grouped convolution: this tile's image (P is this kernel's own copy of the descriptor)
        // g_group_of_tile / g_enter_group of gemm_common.h written out: through the helpers the two-workgroup instantiations, which never
        // run a grouped launch, come out with another register allocation (120 instead of 122 VGPRs)
        L = __builtin_amdgcn_readfirstlane(L);
        dgxgemm::GemmP::Grp q = P.grp[0];
#pragma unroll
        for (int k = 1; k < dgxgemm::GEMM_MAXG; ++k)
            if (k < P.ngrp && L >= P.grp[k].tile0) q = P.grp[k];
        P.A = q.A; P.C = q.C; P.M = q.M;
        P.cmap_n = q.cn; P.cmap_h = q.ch; P.cmap_w = q.cw; P.conv_wp = q.wp;
        L -= q.tile0;
    }
    DGX_CLK(0);
    DGX_CLK_RT(5);                                    // constant 100 MHz counter next to the shader-clock one: the ratio is the clock
    const int tm = L / P.tiles_n, tn = L - tm * P.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = w >> 2, wc = w & 3;            // group = M half of the tile (waves 0-3: rows 0 .. BM/2)
    const int c = l & 15, g = l >> 4;
    const int NTK = (P.K + GBK - 1) / GBK;         // K-tiles of the problem
    const int ktail = P.K - (NTK - 1) * GBK;       // elements of the last one (64 when K % 64 == 0)
    const int kt0 = split * P.kt_per_split;        // this workgroup's K-tiles: kt0 .. kt0 + NT
    const int NT = min(P.kt_per_split, NTK - kt0);

    // ---- loader role: instruction q = w + 8 s of a tile covers tile rows 8q .. 8q+7 (A rows first, then B rows);
    // lane -> row 8q + (l >> 3), physical chunk l & 7 = logical chunk ^ ((row >> 1) & 7), (q & 1) == (w & 1)
    const int rsub = l >> 3;
    const int lc = (l & 7) ^ (((w & 1) << 2) | (rsub >> 1));
    uint32_t voffA[NA], voffB[NB];
#pragma unroll
    for (int s = 0; s < NA; ++s) voffA[s] = g_a_voff(P, m0 + 8 * (w + 8 * s) + rsub, lc);
#pragma unroll
    for (int s = 0; s < NB; ++s) {
        const int n = n0 + 8 * (w + 8 * s) + rsub;
        voffB[s] = n < P.N ? (uint32_t)(((int64_t)n * P.ldb + lc * 8) * 2) : BUF_OOB;
    }
    const bool kt_ok = lc * 8 < ktail;             // this lane's chunk exists in the last K-tile
    const u32x4 rA = buf_rsrc(P.A, (uint32_t)((P.conv_kc ? (int64_t)P.cmap_n * (P.cmap_h + 2) * P.conv_wp + 2 * P.conv_wp + 2 : (int64_t)P.M) * P.lda * 2));
    const u32x4 rB = buf_rsrc(P.B, (uint32_t)((int64_t)P.N * P.ldb * 2));
    const uint32_t lds0 = (uint32_t)(uintptr_t)(DGX_LDS unsigned char*)lds_raw;
    const uint32_t ldsw = __builtin_amdgcn_readfirstlane(lds0 + 1024u * w);
    // one of the NL loads of a tile: k < NA -> A rows, else B rows
    auto issue_one = [&](int k, int t, int stage) {
        const int kta = kt0 + t;
        const uint32_t soff = (uint32_t)kta * (GBK * 2), soffA = g_a_soff(P, kta);
        const uint32_t dst = ldsw + (uint32_t)stage * SB;
        const bool tail = (kta == NTK - 1) && (ktail != GBK) && !kt_ok;
        if (k < NA) lds_load16(tail ? BUF_OOB : voffA[k], rA, dst + 8192u * k, soffA);
        else lds_load16(tail ? BUF_OOB : voffB[k - NA], rB, dst + BM * 128 + 8192u * (k - NA), soff);
    };

    // ---- MFMA role: wave tile = rows grp*BM/2 .. (+16 i + c), columns wc*BN/4 .. (+16 j + c); a fragment (16 rows, k-half kh)
    // is one ds_read_b128 per lane: row c, logical chunk g + 4 kh -> physical (g ^ swz) ^ 4 kh, swz = (c >> 1) & 7
    const int swz = (c >> 1) & 7;
    const uint32_t la = (uint32_t)((grp * (BM / 2) + c) * 128 + ((g ^ swz) << 4));
    const uint32_t lb = (uint32_t)((BM + wc * (BN / 4) + c) * 128 + ((g ^ swz) << 4));
    f32x4 acc[WMF][WNF];
#pragma unroll
    for (int i = 0; i < WMF; ++i)
#pragma unroll
        for (int j = 0; j < WNF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 af[WMF][2], bfr[WNF][2];
    // LOAD phase of group 0: this wave's NL loads of tile `ti` (if >= 0) into stage `istage`, then the 2 (WMF + WNF) fragment
    // reads of the tile in `stage`.  Measured (profiles/r04_gemm_nt_phases.txt): an LDS-direct load costs its wave ~60 cycles of
    // issue next to MFMAs or plain code and ~80-180 when it sits between ds_reads, so the loads are kept together.
    auto load_phase = [&](int stage, int ti, int istage) {
        if (ti >= 0) {
#pragma unroll
            for (int k = 0; k < NL; ++k) issue_one(k, ti, istage);
        }
        DGX_LDS const unsigned char* sa = lds_opaque((const unsigned char*)lds_raw + stage * SB + la);
        DGX_LDS const unsigned char* sa1 = lds_opaque((const unsigned char*)lds_raw + stage * SB + (la ^ 64u));
        DGX_LDS const unsigned char* sb = lds_opaque((const unsigned char*)lds_raw + stage * SB + lb);
        DGX_LDS const unsigned char* sb1 = lds_opaque((const unsigned char*)lds_raw + stage * SB + (lb ^ 64u));
#pragma unroll
        for (int j = 0; j < WNF; ++j) {
            bfr[j][0] = *reinterpret_cast<DGX_LDS const bf16x8*>(sb + 2048 * j);
            bfr[j][1] = *reinterpret_cast<DGX_LDS const bf16x8*>(sb1 + 2048 * j);
        }
#pragma unroll
        for (int i = 0; i < WMF; ++i) {
            af[i][0] = *reinterpret_cast<DGX_LDS const bf16x8*>(sa + 2048 * i);
            af[i][1] = *reinterpret_cast<DGX_LDS const bf16x8*>(sa1 + 2048 * i);
        }
    };
    auto mfmas = [&]() {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int i = 0; i < WMF; ++i)
#pragma unroll
                for (int j = 0; j < WNF; ++j) acc[i][j] = mfma16(bfr[j][kh], af[i][kh], acc[i][j]);   // D[n][m]: lane = 4 columns of a row
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- main loop.  Intervals between barriers I_0, I_1, ...: group 0 reads tile t in I_{2t+1} and multiplies in I_{2t+2};
    // group 1 reads in I_{2t+2} and multiplies in I_{2t+3}.  Tile tau lives in stage tau % NS: it replaces tile tau - NS, whose
    // last read (group 1) ends with the barrier that opens I_{2(tau-NS)+3}; both groups issue it in that interval (group 0 in
    // its read phase of tile tau-NS+1, group 1 in its MFMA phase of tile tau-NS) and every wave has waited for its share
    // before the barrier that opens I_{2 tau + 1}: 2 (NS - 1) intervals of flight.
    // wait for this wave's share of tile `tau` with the later tiles it has already issued still in flight
    auto wait_tile = [&](int tau) {
        int later = NT - 1 - tau;
        if (later > NS - 2) later = NS - 2;
        if (NS >= 4 && later >= 2) wait_vmcnt<2 * NL>();
        else if (NS >= 3 && later >= 1) wait_vmcnt<NL>();
        else wait_vmcnt<0>();
    };
#pragma unroll
    for (int t = 0; t < NS; ++t)
        if (t < NT) {
#pragma unroll
            for (int k = 0; k < NL; ++k) issue_one(k, t, t);
        }
    {
        int later = NT - 1;
        if (later > NS - 1) later = NS - 1;
        if (NS >= 4 && later >= 3) wait_vmcnt<3 * NL>();
        else if (NS >= 3 && later >= 2) wait_vmcnt<2 * NL>();
        else if (later >= 1) wait_vmcnt<NL>();
        else wait_vmcnt<0>();
    }
    wg_barrier();                                       // #0: tile 0 visible to everyone
    DGX_CLK(1);
    int rs = 0;                                    // stage of the tile being read
    // Group 0 issues in its LOAD phase, group 1 right AFTER its MFMAs (both in I_{2t+3} for tile t + 2 when NS = 2).
    // Measured per K-tile of a 256x192 tile: loads of group 1 in front of its MFMAs 2525 cycles (their issue time delays the
    // whole interval), behind them 2106; both groups issuing in their LOAD phases (possible from 3 stages on) is no better.
    if (grp == 0) {
        int is = NS - 1;                           // stage of the next tile to issue (tile t + NS - 1 at t >= 1)
        for (int t = 0; t < NT; ++t) {
            int ti = -1;
            if (t >= 1) {
                is = is + 1 == NS ? 0 : is + 1;
                if (t + NS - 1 < NT) ti = t + NS - 1;
            }
            load_phase(rs, ti, is);
            rs = rs + 1 == NS ? 0 : rs + 1;
            wait_lgkm0();
            wg_barrier();                               // #(2t+1)
            mfmas();
            if (t + 1 < NT) wait_tile(t + 1);
            wg_barrier();                               // #(2t+2)
        }
        wg_barrier();                                   // group 1's last phase
    } else {
        int is = 0;                                // tile t + NS goes where tile t was
        wg_barrier();                                   // #1: one phase behind group 0
        for (int t = 0; t < NT; ++t) {
            load_phase(rs, -1, 0);
            rs = rs + 1 == NS ? 0 : rs + 1;
            wait_lgkm0();
            if (t + 1 < NT) wait_tile(t + 1);
            wg_barrier();                               // #(2t+2)
            mfmas();
            if (t + NS < NT) {
#pragma unroll
                for (int k = 0; k < NL; ++k) issue_one(k, t + NS, is);
            }
            is = is + 1 == NS ? 0 : is + 1;
            wg_barrier();                               // #(2t+3)
        }
    }
    wait_vmcnt<0>();
    DGX_CLK(2);

    // ---- split-K: the raw fp32 accumulators go to this split's slab; dgx's fold kernel finishes the job
    if (P.splits > 1) {
        float* slab = P.ws + (int64_t)split * P.M * P.N;
        const int colw = n0 + wc * (BN / 4) + 4 * g;
#pragma unroll
        for (int i = 0; i < WMF; ++i) {
            const int gm = m0 + grp * (BM / 2) + 16 * i + c;
#pragma unroll
            for (int j = 0; j < WNF; ++j) {
                const int gn = colw + 16 * j;
                if (gm < P.M && gn < P.N) *reinterpret_cast<f32x4*>(slab + (int64_t)gm * P.N + gn) = acc[i][j];
            }
        }
        return;
    }
    // ---- epilogue: stage the tile as bf16 (bias added) in LDS, then stream whole rows out with the fused tail.  The extra
    // operands of the tail (mode 4 / 5: the saved pre-activation tile; mode 3: the residual rows -- cold in HBM) are requested
    // for the WHOLE tile before the accumulators are staged (ITERS 16-byte loads per lane in flight, hidden behind the staging
    // pass and its barrier); round 2 fetched them in batches of four behind the barrier and the read-out waited on each batch.
    DGX_LDS unsigned char* stg = (DGX_LDS unsigned char*)lds_raw;
    DGX_LDS int64_t* rowtok = reinterpret_cast<DGX_LDS int64_t*>(stg + BM * SROW);   // mode 3: (token << 32 | DropPath factor bits) per tile row
    constexpr int CPR = BN / 8;                    // 16-byte chunks per tile row
    constexpr int ITERS = (BM * CPR + 511) / 512;
    if (P.mode == 3) {
        if (tid < BM) g_fill_rowtok(P, rowtok, m0, tid);
        __syncthreads();
    }
    // PFN chunks of the tail operands per lane are requested at a time: the whole tile for the one-workgroup-per-CU instantiations,
    // half of it where two workgroups share a CU (128 registers per lane; the partner workgroup covers the second half's latency)
    constexpr int PFN = MINW >= 4 ? ITERS / 2 : ITERS;
    static_assert(PFN > 0 && ITERS % PFN == 0 && ITERS / PFN <= 2, "one or two whole chunks");
    u32x4 xa[PFN], xb[PFN];
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));               // opaque: keeps the chunk addresses of the tail from being formed above the main loop
    // chunk `it` of this lane: tile row / 16-byte column, global row / column, token and DropPath factor (mode 3)
    auto locate = [&](int it, int& row, int& ch, int& gm, int& gn, int64_t& tok, float& sc) -> bool {
        const int idx = tid_e + it * 512;
        row = idx / CPR;
        ch = idx - row * CPR;
        gm = m0 + row;
        gn = n0 + 8 * ch;
        tok = 0;
        sc = 1.0f;
        bool ok = idx < BM * CPR && gm < P.M && gn < P.N;
        if (P.mode == 3 && ok) {
            const int64_t rt = rowtok[row];
            ok = rt >= 0;
            tok = rt >> 32;
            sc = __uint_as_float((uint32_t)rt);
        }
        return ok;
    };
    // branch-free per lane (a chunk outside the problem reads element 0 of the operand and is dropped in the finish loop): with
    // the loads under per-lane conditions the compiler carries both arrays through every join and spills them
    static_assert((BM * CPR) % 512 == 0, "every lane owns exactly ITERS chunks");
    // ONE straight-line set of loads for every tail that reads an operand: the address is chosen per mode, the load is common.  With a
    // load per mode branch (round 4) the values met in different registers at the join and the compiler copied them there -- behind an
    // s_waitcnt vmcnt(0) at the end of each branch, i.e. the prefetch was waited for before the staging pass it was meant to overlap.
#define DGX_EPI_PREFETCH_N(IT0, SLOT0, CNT)                                                                                       \
    if (P.mode >= 3) {                                                                                                            \
        const bool m3_ = P.mode == 3, f32_ = m3_ && P.res_dtype != DGX_BF16;                                                      \
        const char* base_ = m3_ ? (const char*)P.res : (const char*)P.aux;                                                        \
        _Pragma("unroll") for (int pi_ = 0; pi_ < (CNT); ++pi_) {                                                                    \
            const int idx = tid_e + ((IT0) + pi_) * 512, row = idx / CPR, gm = m0 + row, gn = n0 + 8 * (idx - row * CPR);          \
            const bool in_ = gm < P.M && gn < P.N;                                                                                \
            int64_t off = 0;                                                                                                      \
            if (m3_) { const int64_t rt = rowtok[row]; if (in_ && rt >= 0) off = (rt >> 32) * P.N + gn; }                         \
            else if (in_) off = (int64_t)gm * P.ldaux + gn;                                                                       \
            const char* p_ = base_ + off * (f32_ ? 4 : 2);                                                                        \
            xa[(SLOT0) + pi_] = *reinterpret_cast<const u32x4*>(p_);                                                               \
            if (f32_) xb[(SLOT0) + pi_] = *reinterpret_cast<const u32x4*>(p_ + 16);                                                \
        }                                                                                                                         \
    }
#define DGX_EPI_PREFETCH(IT0) DGX_EPI_PREFETCH_N(IT0, 0, PFN)
    {
        const int colw = wc * (BN / 4) + 4 * g;    // + 16 j: this lane's 4 consecutive columns
        // the bias row is requested IN FRONT of the tail's operands: vmcnt retires in order, so waiting for a bias load that was issued
        // behind the prefetch meant waiting for the whole prefetch before the staging pass it was to hide under (round 5)
        u32x2 braw[WNF];
#pragma unroll
        for (int j = 0; j < WNF; ++j) {
            const int n = n0 + colw + 16 * j;
            braw[j] = u32x2{0u, 0u};
            if (P.bias && n < P.N) braw[j] = *reinterpret_cast<const u32x2*>(P.bias + n);
        }
        __builtin_amdgcn_sched_barrier(0);
        DGX_EPI_PREFETCH(0)
        __builtin_amdgcn_sched_barrier(0);
        float bv[WNF][4];
#pragma unroll
        for (int j = 0; j < WNF; ++j) g_bias4(braw[j], bv[j]);
#pragma unroll
        for (int i = 0; i < WMF; ++i) {
            const int row = grp * (BM / 2) + 16 * i + c;
#pragma unroll
            for (int j = 0; j < WNF; ++j) {
                const f32x4 a = acc[i][j];
                const u32x2 pk = {pack_bf2(a[0] + bv[j][0], a[1] + bv[j][1]), pack_bf2(a[2] + bv[j][2], a[3] + bv[j][3])};
                *reinterpret_cast<DGX_LDS u32x2*>(stg + row * SROW + (colw + 16 * j) * 2) = pk;
            }
        }
    }
    __syncthreads();
    DGX_CLK(3);
#pragma unroll
    for (int it = 0; it < PFN; ++it) {
        int row, ch, gm, gn;
        int64_t tok;
        float sc;
        if (locate(it, row, ch, gm, gn, tok, sc))
            g_epi_finish(P, gm, gn, *reinterpret_cast<DGX_LDS const u32x4*>(stg + row * SROW + ch * 16), tok, sc, xa[it], xb[it]);
        // second half (two workgroups per CU: half the tile's operands fit the registers): chunk PFN + it is requested into the
        // registers chunk `it` has just released, so it flies while the rest of the first half is finished
        if constexpr (PFN < ITERS) { DGX_EPI_PREFETCH_N(PFN + it, it, 1) }
    }
    if constexpr (PFN < ITERS) {
#pragma unroll
        for (int it = 0; it < PFN; ++it) {
            int row, ch, gm, gn;
            int64_t tok;
            float sc;
            if (locate(PFN + it, row, ch, gm, gn, tok, sc))
                g_epi_finish(P, gm, gn, *reinterpret_cast<DGX_LDS const u32x4*>(stg + row * SROW + ch * 16), tok, sc, xa[it], xb[it]);
        }
    }
#undef DGX_EPI_PREFETCH
#undef DGX_EPI_PREFETCH_N
    DGX_CLK(4);
    DGX_CLK_RT(6);
}

// split-K fold: y = bf16(sum_s slab[s] + bias), then the same fused tail; one lane per 8-column chunk
__global__ __launch_bounds__(256) void gemm_splitk_fold_kernel(GemmP P) {
    const int cpr = P.N >> 3;
    const int64_t total = (int64_t)P.M * cpr, slab = (int64_t)P.M * P.N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int gm = (int)(i / cpr), gn = (int)(i - (int64_t)gm * cpr) * 8;
        const float* p = P.ws + (int64_t)gm * P.N + gn;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < P.splits; ++s) {
            const float4 a = reinterpret_cast<const float4*>(p + s * slab)[0], b = reinterpret_cast<const float4*>(p + s * slab)[1];
            v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
        }
        if (P.bias) {
            float bv[8];
            unpack8(*reinterpret_cast<const u32x4*>(P.bias + gn), bv);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] += bv[k];
        }
        int64_t tok = 0;
        float sc = 1.0f;
        if (P.mode == 3) {
            int b = 0;
            tok = wm_row_token<int64_t, G_ORDERS>(P.map, (int64_t)gm, b);
            if (tok < 0) continue;
            if (P.scale) sc = P.scale[b];
        }
        g_epilogue_chunk(P, gm, gn, pack8(v), tok, sc);
    }
}

using dgxplan::GemmPlan;
static_assert(dgxplan::BK == GBK && dgxplan::MAXG == dgxgemm::GEMM_MAXG, "gemm_plan.h restates these");

namespace {
dgxplan::DevKnobs g_dev;               // dgx_dev_set
struct LastForm { int form = -1, bm = 0, bn = 0, splits = 0; } g_last;     // what the most recent dispatch launched (dgx_gemm_last_form)
FILE* g_gemm_log = nullptr;            // one line per launch (dgx_dev_gemm_log), joined with a kernel trace by tools/gemm_insitu.py

template <int BM, int BN, int NS, int MINW, int MC>
int nt_launch_e(GemmP& P, hipStream_t st) {
    using Cfg = GemmCfg<BM, BN, NS>;
    static bool once = false;
    if (!once) {
        if (hipFuncSetAttribute((const void*)gemm_nt_kernel<BM, BN, NS, MINW, MC>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS) != hipSuccess)
            return DGX_ERR_UNSUPPORTED;
        once = true;
    }
    hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, NS, MINW, MC>), dim3(8 * P.per_xcd), dim3(512), Cfg::LDS, st, P);
    return DGX_OK;
}
// The gemm_nt instantiation of a plan: tile, stages and workgroups per CU (dgxplan::nt_stages), compiled-in tail.  Returns
// DGX_ERR_UNSUPPORTED for one that is not instantiated.
int gemm_nt_launch(GemmP& P, const GemmPlan& pl, hipStream_t st) {
    const int bm = pl.bm, bn = pl.bn, ns = pl.stages;
    if (pl.wg_per_cu == 2 && bm == 128 && bn == 192 && ns == 2)
        return g_with_mc(pl.mc, [&](auto mc) {
            constexpr int v = decltype(mc)::value;
            return nt_launch_e<128, 192, 2, 4, (v == 2 || v == 3 || v == 4 || v == 6) ? v : -1>(P, st);
        });
    if (pl.wg_per_cu != 1) return DGX_ERR_UNSUPPORTED;
    if (bm == 256 && bn == 192 && ns == 2) return nt_launch_e<256, 192, 2, 2, -1>(P, st);
    if (bm == 192 && bn == 192 && ns == 3) return nt_launch_e<192, 192, 3, 2, -1>(P, st);
    if (bm == 128 && bn == 192 && ns == 4) return nt_launch_e<128, 192, 4, 2, -1>(P, st);
    if (bm == 192 && bn == 256 && ns == 2) return nt_launch_e<192, 256, 2, 2, -1>(P, st);
    if (bm == 128 && bn == 256 && ns == 3) return nt_launch_e<128, 256, 3, 2, -1>(P, st);
    if (bm == 256 && bn == 128 && ns == 3) return nt_launch_e<256, 128, 3, 2, -1>(P, st);
    if (bm == 128 && bn == 128 && ns == 4) return nt_launch_e<128, 128, 4, 2, -1>(P, st);
    return DGX_ERR_UNSUPPORTED;
}
}  // namespace

int gemm_lw_launch(GemmP& P, int bm, int bn, hipStream_t st);     // gemm_lw.hip: the loader-wave form
bool dgx_gemm_k192_takes(const GemmP& P);                          // gemm_k192.hip: the HBM-bound K = 192 problems of Swin stage 0
int dgx_gemm_k192_launch(const GemmP& P, hipStream_t st);

// The plan of a filled descriptor (gemm_plan.h decides; nothing here does) and its line in the launch log
static GemmPlan plan_and_log(const GemmP& P, int64_t ws_bytes) {
    dgxplan::GemmProblem q;
    q.M = P.M; q.N = P.N; q.K = P.K;
    q.mode = P.mode; q.res_bf16 = P.res_dtype == DGX_BF16;
    q.conv = P.conv_kc != 0; q.relu = P.relu != 0;
    q.ngrp = P.ngrp;
    int rows = P.ngrp ? 0 : P.M;                   // log: M = all images' rows
    for (int i = 0; i < P.ngrp; ++i) { q.Ms[i] = P.grp[i].M; rows += P.grp[i].M; }
    q.ws_bytes = P.ws ? ws_bytes : 0;
    q.k192_operands = dgx_gemm_k192_takes(P);
    const GemmPlan pl = dgxplan::plan_gemm(q, g_dev, dgx_get_reserved_cus() / 8);
    if (g_gemm_log) { fprintf(g_gemm_log, "%d %d %d %d %d %d\n", rows, P.N, P.K, P.conv_kc ? 9 : P.mode, pl.bm, pl.bn); fflush(g_gemm_log); }
    return pl;
}
// Launch a planned problem: the plan's tiling into the descriptor, the form's kernel, the split-K fold behind it
static int launch(GemmP& P, const GemmPlan& pl, hipStream_t st) {
    P.tiles_n = pl.tiles_n; P.total = pl.total; P.per_xcd = pl.per_xcd;
    P.splits = pl.splits; P.kt_per_split = pl.kt_per_split;
    for (int i = 0; i < P.ngrp; ++i) P.grp[i].tile0 = pl.tile0[i];
    const bool k192 = pl.form == dgxplan::FORM_K192;
    const int rc = k192 ? dgx_gemm_k192_launch(P, st) : pl.form == dgxplan::FORM_LW ? gemm_lw_launch(P, pl.bm, pl.bn, st) : gemm_nt_launch(P, pl, st);
    if (rc != DGX_OK) return rc;
    if (k192) g_last = {pl.form, 32, 192, 1};
    else g_last = {pl.form, pl.bm, pl.bn, pl.splits};
    if (!k192 && pl.splits > 1) {
        const int64_t chunks = (int64_t)P.M * (P.N >> 3);
        const int grid = (int)((chunks + 255) / 256 < 4096 ? (chunks + 255) / 256 : 4096);
        hipLaunchKernelGGL(gemm_splitk_fold_kernel, dim3(grid), dim3(256), 0, st, P);
    }
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

DGX_CLK_READER(dgx_dev_gemm_nt_clocks)
extern "C" int dgx_dev_gemm_log(const char* path) {
    if (g_gemm_log) { fclose(g_gemm_log); g_gemm_log = nullptr; }
    if (path && *path && !(g_gemm_log = fopen(path, "w"))) return DGX_ERR_BAD_ARG;
    return DGX_OK;
}
const dgxplan::DevKnobs& dgx_dev_knobs() { return g_dev; }      // wgrad256.hip reads wgrad_lw here
extern "C" int dgx_dev_set(const char* key, int value) {          // tests and A/B tools only; the values: dgxplan::DevKnobs
    if (!key) return DGX_ERR_BAD_ARG;
    if (!strcmp(key, "gemm_lw")) g_dev.lw = value;
    else if (!strcmp(key, "gemm_2wg")) g_dev.two_wg = value;
    else if (!strcmp(key, "gemm_tile")) { g_dev.tile_bm = value / 1000; g_dev.tile_bn = value % 1000; }
    else if (!strcmp(key, "gemm_splitk")) g_dev.splitk = value;
    else if (!strcmp(key, "gemm_k192")) g_dev.k192 = value;
    else if (!strcmp(key, "wgrad_lw")) g_dev.wgrad_lw = value;
    else if (!strcmp(key, "reset")) g_dev = dgxplan::DevKnobs();
    else return DGX_ERR_BAD_ARG;
    return DGX_OK;
}
extern "C" int dgx_gemm_last_form(int* bm, int* bn, int* splits) {
    if (bm) *bm = g_last.bm;
    if (bn) *bn = g_last.bn;
    if (splits) *splits = g_last.splits;
    return g_last.form;
}

extern "C" int dgx_gemm_bf16_nt(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb,
                                const dgx_gemm_epilogue* ep, void* stream) {
    if (M <= 0 || N <= 0) return DGX_OK;
    if (!A || !B || !ep || K <= 0 || (K & 7) || (N & 7) || (lda & 7) || (ldb & 7) || lda < K || ldb < K) return DGX_ERR_BAD_ARG;
    if ((int64_t)M * lda * 2 >= (1ll << 31) || (int64_t)N * ldb * 2 >= (1ll << 31)) return DGX_ERR_UNSUPPORTED;
    GemmP P;
    memset((void*)&P, 0, sizeof(P));
    P.A = (const uint16_t*)A; P.B = (const uint16_t*)B;
    P.M = M; P.N = N; P.K = K; P.lda = (int)lda; P.ldb = (int)ldb;
    P.mode = ep->mode;
    P.C = (uint16_t*)ep->c; P.ldc = (int)ep->ldc;
    P.bias = (const uint16_t*)ep->bias;
    P.C2 = (uint16_t*)ep->c2;
    P.aux = (const uint16_t*)ep->aux; P.ldaux = (int)ep->ldaux;
    P.res = ep->residual; P.out = ep->out; P.scale = ep->scale; P.res_dtype = ep->residual_dtype;
    P.ws = (float*)ep->workspace;
    P.relu = (ep->mode <= DGX_EPI_BIAS) ? ep->relu : 0;
    switch (ep->mode) {
        case DGX_EPI_NONE: case DGX_EPI_BIAS:
            if (!ep->c || ep->ldc < N || (ep->ldc & 7)) return DGX_ERR_BAD_ARG;
            if (ep->mode == DGX_EPI_NONE) P.bias = nullptr;
            break;
        case DGX_EPI_BIAS_GELU:
            if (!ep->c || !ep->c2 || ep->ldc < N || (ep->ldc & 7)) return DGX_ERR_BAD_ARG;
            break;
        case DGX_EPI_GELU_GRAD: case DGX_EPI_RELU_GRAD:
            if (!ep->c || !ep->aux || ep->ldc < N || ep->ldaux < N || (ep->ldc & 7) || (ep->ldaux & 7)) return DGX_ERR_BAD_ARG;
            P.bias = nullptr;
            break;
        case DGX_EPI_BIAS_RESIDUAL: {
            // ws < 0: the rows are in COMPACT window order (winmap.h: real tokens only, M = B*H*W)
            if (!ep->residual || !ep->out || ep->B <= 0 || ep->H <= 0 || ep->W <= 0 || ep->B > 4095 ||
                (ep->residual_dtype != DGX_F32 && ep->residual_dtype != DGX_BF16) ||
                !wm_map_ok(ep->B, ep->H, ep->W, ep->ws, ep->shift, G_ORDERS))
                return DGX_ERR_BAD_ARG;
            P.map = wm_map(ep->B, ep->H, ep->W, ep->ws, ep->shift);
            if ((ep->ws > 0 ? wm_classic_rows(P.map) : (int64_t)ep->B * ep->H * ep->W) != M) return DGX_ERR_BAD_ARG;
            break;
        }
        default: return DGX_ERR_BAD_ARG;
    }
    // algorithmic traffic: both operands once, every result tensor once (residual mode: residual in, sum out, no C)
    const double mn = (double)M * N, rsz = ep->residual_dtype == DGX_F32 ? 4.0 : 2.0;
    const double obytes = ep->mode == DGX_EPI_BIAS_RESIDUAL ? 2.0 * rsz * mn : (ep->mode >= DGX_EPI_BIAS_GELU ? 4.0 * mn : 2.0 * mn);   // GELU / GELU' / ReLU': two tensors
    DgxProfScope prof(DGX_PROF_GEMM_NT, stream, 2.0 * mn * K, 2.0 * ((double)M * K + (double)N * K) + obytes);
    return launch(P, plan_and_log(P, ep->workspace_bytes), (hipStream_t)stream);
}

extern "C" int64_t dgx_conv3x3_pad_rows(int N, int H, int W) {
    return (N <= 0 || H <= 0 || W <= 0) ? 0 : (int64_t)N * (H + 2) * (W + 2) + 2 * (int64_t)(W + 3);
}

// y_i = conv3x3(x_i, w) (+ bias) for n <= 6 zero-bordered images that share the weights, in ONE launch (see GemmP::grp): the levels of
// a CenterNet tower layer.  Cout <= 256 (one column tile of the instantiations used here).
extern "C" int dgx_conv3x3_gemm_multi(const dgx_conv_item* items, int n, const void* w, const void* bias, int Cin, int Cout, int relu,
                                      void* stream) {
    if (n <= 0) return DGX_OK;
    if (!items || !w || Cin <= 0 || Cout <= 0 || (Cin & 63) || (Cout & 7)) return DGX_ERR_BAD_ARG;
    if (n > dgxgemm::GEMM_MAXG || Cout > 256 || (int64_t)Cout * 9 * Cin * 2 >= (1ll << 31)) return DGX_ERR_UNSUPPORTED;
    GemmP P;
    memset((void*)&P, 0, sizeof(P));
    P.B = (const uint16_t*)w;
    P.N = Cout; P.K = 9 * Cin; P.lda = Cin; P.ldb = 9 * Cin;
    P.mode = bias ? DGX_EPI_BIAS : DGX_EPI_NONE;
    P.ldc = Cout;
    P.bias = (const uint16_t*)bias;
    P.conv_kc = Cin / GBK;
    P.relu = relu;
    P.ngrp = n;
    double fl = 0.0, by = 2.0 * 9.0 * Cin * Cout;
    for (int i = 0; i < n; ++i) {
        const dgx_conv_item& a = items[i];
        if (!a.xpad || !a.y || a.N <= 0 || a.H <= 0 || a.W <= 0) return DGX_ERR_BAD_ARG;
        if (dgx_conv3x3_pad_rows(a.N, a.H, a.W) * Cin * 2 >= (1ll << 31)) return DGX_ERR_UNSUPPORTED;
        P.grp[i].A = (const uint16_t*)a.xpad; P.grp[i].C = (uint16_t*)a.y; P.grp[i].M = a.N * a.H * a.W;
        P.grp[i].cn = a.N; P.grp[i].ch = a.H; P.grp[i].cw = a.W; P.grp[i].wp = a.W + 2;
        const double pix = (double)a.N * a.H * a.W;
        fl += 2.0 * pix * Cout * 9.0 * Cin;
        by += 2.0 * ((double)a.N * (a.H + 2) * (a.W + 2) * Cin + pix * Cout);
    }
    for (int i = n; i < dgxgemm::GEMM_MAXG; ++i) P.grp[i] = P.grp[0];
    // first group's fields also in the single-image slots (the kernel overwrites them per tile)
    P.A = P.grp[0].A; P.C = P.grp[0].C; P.M = P.grp[0].M;
    P.cmap_n = P.grp[0].cn; P.cmap_h = P.grp[0].ch; P.cmap_w = P.grp[0].cw; P.conv_wp = P.grp[0].wp;
    DgxProfScope prof(DGX_PROF_GEMM_NT, stream, fl, by);
    return launch(P, plan_and_log(P, 0), (hipStream_t)stream);
}

extern "C" int dgx_conv3x3_gemm(const void* xpad, const void* w, const void* bias, void* y, int N, int H, int W, int Cin, int Cout,
                                int relu, void* workspace, int64_t workspace_bytes, void* stream) {
    if (N <= 0 || H <= 0 || W <= 0) return DGX_OK;
    if (!xpad || !w || !y || Cin <= 0 || Cout <= 0 || (Cin & 63) || (Cout & 7)) return DGX_ERR_BAD_ARG;
    const int64_t Mp = (int64_t)N * (H + 2) * (W + 2);
    if (dgx_conv3x3_pad_rows(N, H, W) * Cin * 2 >= (1ll << 31) || (int64_t)Cout * 9 * Cin * 2 >= (1ll << 31)) return DGX_ERR_UNSUPPORTED;
    GemmP P;
    memset((void*)&P, 0, sizeof(P));
    P.A = (const uint16_t*)xpad;                   // row 0 of the GEMM = padded position 0 minus (Wp + 1): the leading slack
    P.B = (const uint16_t*)w;
    P.M = N * H * W; P.N = Cout; P.K = 9 * Cin; P.lda = Cin; P.ldb = 9 * Cin;
    P.mode = bias ? DGX_EPI_BIAS : DGX_EPI_NONE;
    P.C = (uint16_t*)y; P.ldc = Cout;
    P.bias = (const uint16_t*)bias;
    P.conv_kc = Cin / GBK; P.conv_wp = W + 2;
    P.cmap_n = N; P.cmap_h = H; P.cmap_w = W;
    P.relu = relu;
    P.ws = (float*)workspace;                      // small FPN levels: few tiles, 9 Cin / 64 K-tiles -> split-K slabs + fold
    const double pix = (double)N * H * W;       // useful work: the H x W interior (border rows of the padded grid are overhead)
    DgxProfScope prof(DGX_PROF_GEMM_NT, stream, 2.0 * pix * Cout * 9.0 * Cin,
                      2.0 * ((double)Mp * Cin + 9.0 * Cin * Cout + pix * Cout));
    return launch(P, plan_and_log(P, workspace_bytes), (hipStream_t)stream);
}

// Development timing hook (not part of include/divergen_hip.h): `iters` back-to-back launches of the same GEMM between two
// HIP events on `stream`; returns the average kernel time in microseconds (host launch cost excluded), < 0 on error.
extern "C" float dgx_dev_gemm_time_us(const void* A, const void* B, int M, int N, int K, int64_t lda, int64_t ldb,
                                      const dgx_gemm_epilogue* ep, int iters, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < 3; ++i)
        if (dgx_gemm_bf16_nt(A, B, M, N, K, lda, ldb, ep, stream) != DGX_OK) return -1.f;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -2.f;
    (void)hipEventRecord(e0, st);
    for (int i = 0; i < iters; ++i) (void)dgx_gemm_bf16_nt(A, B, M, N, K, lda, ldb, ep, stream);
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms * 1000.f / (float)iters;
}
