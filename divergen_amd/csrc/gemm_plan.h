// Which kernel runs a forward / input-gradient GEMM and how it is tiled: the whole decision of the family (gemm_nt.hip, gemm_lw.hip,
// gemm_k192.hip) as plain host C++ -- integer arithmetic on the problem's sizes, no HIP header, so that tests/native/gemm_plan_check.cpp
// checks it with g++ and no GPU.  gemm_nt.hip's entry points fill a GemmProblem, call plan_gemm() and hand the plan to launch().
#pragma once
#include <stdint.h>

namespace dgxplan {
constexpr int BK = 64;                 // K-step (gemm_common.h: GBK)
constexpr int MAXG = 6;                // images of a grouped convolution (gemm_common.h: GEMM_MAXG)
// numbering of dgx_gemm_last_form
enum Form { FORM_NT = 0, FORM_LW = 1, FORM_TWO = 2, FORM_K192 = 3 };

// Test / A-B knobs of the dispatch (dgx_dev_set): -1 / 0 = the library's own plan.  The product never sets them; the GEMM tests
// force every tile shape and the split-K path through the one ABI entry with them, the tools compare own form A with own form B.
struct DevKnobs {
    int lw = -1;        // gemm_lw:     -1 plan, 0 gemm_nt everywhere, 1 gemm_lw everywhere
    int two_wg = -1;    // gemm_2wg:    -1 / 1 plan, 0 never the two-workgroup form, >= 2: its row threshold
    int tile_bm = 0, tile_bn = 0;       // gemm_tile:   bm * 1000 + bn, 0 = plan
    int splitk = 0;     // gemm_splitk: 0 plan, >= 1 forced slab count
    int k192 = -1;      // gemm_k192:   -1 / 1 plan, 0 never the resident-panel kernel
    int wgrad_lw = 1;   // wgrad_lw:    1 plan (wgrad_plan.h), 0 never the loader-wave weight-gradient form, 2 always
};

struct GemmProblem {
    int M = 0, N = 0, K = 0;
    int mode = 0;                // the fused tail (DGX_EPI_*)
    int res_bf16 = 0;            // mode 3: the residual stream is bf16 (else fp32)
    bool conv = false;           // implicit 3x3 convolution
    bool relu = false;
    int ngrp = 0;                // grouped convolution: images, with their row counts in Ms (M is unused then)
    int Ms[MAXG] = {0, 0, 0, 0, 0, 0};
    int64_t ws_bytes = 0;        // split-K workspace (0: none)
    bool k192_operands = false;  // the operands' pointers and strides suit gemm_k192 (16-byte aligned; checked where the pointers are)
};

struct GemmPlan {
    int form = -1;               // Form
    int bm = 0, bn = 0;          // tile of gemm_nt / gemm_lw (FORM_K192: the tile those would take; its own tile is 32 x 192)
    int stages = 0, wg_per_cu = 0, mc = -1;      // gemm_nt: LDS stages, workgroups per CU, compiled-in tail (-1: run-time mode)
    int splits = 1, kt_per_split = 0, tiles_n = 0, total = 0, per_xcd = 0;
    int tile0[MAXG] = {0, 0, 0, 0, 0, 0};        // grouped: first tile of each image
};

// the tail as the MC template argument of the kernels: the mode, 6 for mode 3 with an fp32 residual stream
inline int tail_mc(int mode, int res_bf16) { return mode == 3 ? (res_bf16 ? 3 : 6) : mode; }

// LDS stages of the gemm_nt instantiation of a tile (one workgroup per CU), 0: not instantiated
inline int nt_stages(int bm, int bn) {
    if (bn == 192) return bm == 256 ? 2 : bm == 192 ? 3 : bm == 128 ? 4 : 0;
    if (bn == 256) return bm == 192 ? 2 : bm == 128 ? 3 : 0;       // 256x256 does not fit two waves per SIMD (register file)
    if (bn == 128) return bm == 256 ? 3 : bm == 128 ? 4 : 0;       // 192-row tiles: instantiated for BN = 192 and 256
    return 0;
}
// gemm_lw instantiates the same seven tiles
inline bool lw_has_tile(int bm, int bn) { return nt_stages(bm, bn) != 0; }

// Tile selection: BN from the divisibility of N (every Swin width is a multiple of 192), BM from how well the tile count
// fills whole rounds of 256 CUs (one workgroup per CU), weighted by the CU-side efficiency of the smaller tiles.
inline void choose_tile(int M, int N, const DevKnobs& dev, int& bm_out, int& bn_out) {
    if (dev.tile_bm && nt_stages(dev.tile_bm, dev.tile_bn)) {
        bm_out = dev.tile_bm; bn_out = dev.tile_bn;
        return;
    }
    int bn;
    if (N % 192 == 0) bn = 192;
    else if (N % 256 == 0 || N > 1024) bn = 256;
    else bn = 128;
    const int cand[3] = {256, 192, 128};
    const double eff[3] = {1.0, 0.97, 0.85};
    double best = -1.0;
    int bm = 128;
    for (int i = 0; i < 3; ++i) {
        const int b = cand[i];
        if (!nt_stages(b, bn)) continue;
        const int64_t tiles = (int64_t)((M + b - 1) / b) * ((N + bn - 1) / bn);
        const int64_t rounds = (tiles + 255) / 256;
        const double fill = (double)M * N / ((double)rounds * 256 * b * bn);
        const double sc = fill * eff[i];
        if (sc > best) { best = sc; bm = b; }
    }
    bm_out = bm; bn_out = bn;
}

// split-K plan: few output tiles and a long contraction (box-head FC 1024 x 1024 x 12544, 3x3 convolutions over the small
// FPN levels, stage-3 Linears) leave most CUs idle; S slabs of >= 4 K-tiles each fill them.  Returns 1 when not worth it.
inline int choose_splits(int64_t tiles, int K, int64_t M, int64_t N, int64_t ws_bytes, const DevKnobs& dev) {
    const int nt = (K + BK - 1) / BK;
    if (dev.splitk >= 1) {
        const int v = dev.splitk;
        return (v <= nt && (int64_t)v * M * N * 4 <= ws_bytes) ? v : 1;
    }
    if (tiles > 128 || nt < 8) return 1;
    int S = (int)(256 / tiles);
    if (S > nt / 4) S = nt / 4;
    if (S > 16) S = 16;
    while (S > 1 && (int64_t)S * M * N * 4 > ws_bytes) --S;
    return S < 2 ? 1 : S;
}

// reserved_per_xcd: CUs of each XCD left to a concurrent collective (dgx_set_reserved_cus)
inline GemmPlan plan_gemm(const GemmProblem& q, const DevKnobs& dev, int reserved_per_xcd) {
    GemmPlan p;
    const int nt = (q.K + BK - 1) / BK;
    if (q.ngrp > 0) {
        // Grouped convolution (Cout <= 256: one column tile).  192-row tiles when they save a round of the chip (the five tower levels at
        // 1024^2 x 2 images: 341 tiles of 128 rows = two rounds, 229 tiles of 192 rows = one).  No split-K in this form.
        int t128 = 0, t192 = 0;
        for (int i = 0; i < q.ngrp; ++i) { t128 += (q.Ms[i] + 127) / 128; t192 += (q.Ms[i] + 191) / 192; }
        const bool big = q.N > 128 && ((t192 + 255) / 256) * 192 < ((t128 + 255) / 256) * 128;
        p.bm = big ? 192 : 128;
        p.bn = q.N > 128 ? 256 : 128;
        p.form = dev.lw != 0 ? FORM_LW : FORM_NT;
        p.tiles_n = (q.N + p.bn - 1) / p.bn;
        for (int i = 0; i < q.ngrp; ++i) {
            p.tile0[i] = p.total;
            p.total += ((q.Ms[i] + p.bm - 1) / p.bm) * p.tiles_n;
        }
        p.kt_per_split = nt;
    } else {
        // Which form runs a problem (measured in situ, profiles/r04_gemm_insitu_*.txt): the loader-wave persistent kernel wins wherever
        // the read-out is plain (modes 0 / 1, the implicit convolutions: 0.65-0.97x the time, the skinny K = N = 192 projection excepted)
        // and on the long contractions (K > 768) with a residual or GELU tail; the two-workgroup form of gemm_nt keeps the K <= 768 GEMMs
        // whose tails read a cold operand or write two tensors (its second workgroup's main loop hides them).
        choose_tile(q.M, q.N, dev, p.bm, p.bn);
        bool lw;
        if (dev.lw >= 0) lw = dev.lw == 1;
        else if (q.mode <= 1) lw = !(q.N <= 192 && q.K <= 192);
        else lw = (q.mode == 2 || q.mode == 3) && q.K > 768;
        // Contractions of up to 12 K-tiles (K <= 768: every qkv / proj / fc1 / fc2-input-gradient GEMM of the backbone) spend a third of
        // a tile's time in prologue and read-out: TWO workgroups share a CU there (128 x 192 tiles, 2 stages = 80 KB of LDS, 128
        // registers per lane), so one's read-out -- with its GELU / GELU' / residual tail -- runs beside the other's main loop.
        // Round 2 measured this geometry back to back with the bias tail only (-4 % at K = 768, +10..30 % at long K) and dropped it;
        // inside the step, where the tails are the real ones, it wins wherever K <= 768 (round 3, same call: GEMM family
        // 11.80 -> 11.18 ms/step; K <= 384 only: 11.58; every K: 11.70) and loses on the long contractions, which keep the deeper rings.
        const bool two = !lw && p.bn == 192 && dev.two_wg != 0 && q.N % 192 == 0 && q.K <= 768 &&
                         q.M >= (dev.two_wg >= 2 ? dev.two_wg : 4096) && !q.conv;
        if (two) p.bm = 128;
        // The HBM-bound K = 192 problems of Swin stage 0 go to the resident-panel kernel: one workgroup per 192-column panel and XCD at least
        const bool k192 = dev.k192 != 0 && dev.lw < 0 && dev.tile_bm == 0 && dev.splitk == 0 && (dev.two_wg < 0 || dev.two_wg == 1) && q.K == 192 && q.N >= 192 &&
                          q.N % 192 == 0 && q.M >= 32768 && !q.conv && !q.relu && q.mode >= 0 && q.mode <= 4 && q.k192_operands &&
                          32 - reserved_per_xcd >= q.N / 192;
        p.form = k192 ? FORM_K192 : lw ? FORM_LW : two ? FORM_TWO : FORM_NT;
        p.tiles_n = (q.N + p.bn - 1) / p.bn;
        p.total = ((q.M + p.bm - 1) / p.bm) * p.tiles_n;
        p.splits = choose_splits(p.total, q.K, q.M, q.N, q.ws_bytes, dev);
        p.kt_per_split = (nt + p.splits - 1) / p.splits;
        p.splits = (nt + p.kt_per_split - 1) / p.kt_per_split;          // no empty split
        if (p.form == FORM_TWO) {        // the tails this form exists for, each with its mode compiled in
            const int mc = tail_mc(q.mode, q.res_bf16);
            p.mc = (mc == 2 || mc == 3 || mc == 4 || mc == 6) ? mc : -1;
        }
    }
    p.stages = p.form == FORM_TWO ? 2 : nt_stages(p.bm, p.bn);
    p.wg_per_cu = p.form == FORM_TWO ? 2 : 1;
    p.per_xcd = (p.total * p.splits + 7) / 8;
    return p;
}
}  // namespace dgxplan
