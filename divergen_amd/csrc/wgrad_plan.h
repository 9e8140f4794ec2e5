// Which kernel runs a group of weight gradients and how its rows are cut: the whole decision of the family (wgrad256.hip: 256 x 256
// tiles, M split into slabs, partial tiles folded by a reduce launch; wgrad_lw.hip: persistent loader-wave form, whole-M tiles) as plain
// host C++ in the manner of gemm_plan.h -- integer arithmetic on sizes, no HIP header, so that tests/native/wgrad_plan_check.cpp checks
// it with g++ and no GPU.  The entry points of wgrad256.hip size their workspaces from these plans and hand them to the one launch path.
// A problem is anything with int M, Nn, Kk and a gb that converts to bool (dgx_wgrad_problem; the checker's own struct).
#pragma once
#include <stdint.h>

#include "gemm_plan.h"

namespace dgxplan {
constexpr int W_TILE = 256;            // wgrad256: tile edge (T256)
constexpr int W_STAGE = 32;            //           rows of a pipeline stage (BM256): slabs are whole stages
constexpr int W_MAXP = 12;             //           problems per launch (MAXP256)
constexpr int W_MAXIMG = 6;            //           images of a multi-image convolution
constexpr int W_ROUND = 256;           // workgroups of one round of the chip
constexpr int WL_TILE_N = 256, WL_TILE_K = 192, WL_MAXP = 32;      // wgrad_lw: tile (WL_TN x WL_TK), problems per launch

inline int64_t wcdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- form.  Is a group worth the persistent loader-wave form?  Many tiles of that kernel (>= 3/4 of a round of the chip) whose
// contraction is long enough for the main loop to dominate, and whose item count fills whole rounds to >= 74 % (4 stage-2 blocks =
// 2.25 rounds still win).  dev.wgrad_lw: 1 = this rule, 0 = never, 2 = always (every M >= 1024 still holds)
template <class P> bool wgrad_lw_wants(const P* pr, int n, const DevKnobs& dev) {
    if (!dev.wgrad_lw || n <= 0 || n > WL_MAXP) return false;
    int items = 0;
    for (int i = 0; i < n; ++i) {
        if (pr[i].M < 1024) return false;
        items += (int)(wcdiv(pr[i].Nn, WL_TILE_N) * wcdiv(pr[i].Kk, WL_TILE_K));
    }
    if (dev.wgrad_lw == 2) return true;
    if (items < 192) return false;
    const int rounds = (items + W_ROUND - 1) / W_ROUND;
    return (double)items / ((double)W_ROUND * rounds) >= 0.74;
}
// a group the loader-wave launch refuses (an operand over 2^31 bytes, ...) still runs on the split form when that form takes it;
// the sizing call and the launch both ask here, so the fall-back never writes past the caller's buffer
inline bool wgrad_lw_may_fall_back(int n) { return n <= W_MAXP; }

// the item table of a loader-wave launch: one item = one 256 x 192 tile contracting its whole M
struct WgradLwPlan {
    int item0[WL_MAXP], tiles_k[WL_MAXP];
    int total = 0, per_xcd = 0;
};
template <class P> WgradLwPlan plan_wgrad_lw(const P* pr, int n) {
    WgradLwPlan pl;
    for (int i = 0; i < WL_MAXP; ++i) {
        pl.item0[i] = 0x7fffffff;      // unused entries: never found by the kernel's search
        pl.tiles_k[i] = 0;
        if (i >= n) continue;
        pl.tiles_k[i] = (int)wcdiv(pr[i].Kk, WL_TILE_K);
        pl.item0[i] = pl.total;
        pl.total += (int)wcdiv(pr[i].Nn, WL_TILE_N) * pl.tiles_k[i];
    }
    pl.per_xcd = (pl.total + 7) / 8;
    return pl;
}

// ---- the row search, once: the smallest multiple of 32 rows R for which sum_i tiles[i] * ceil(rows[i] / R) workgroups fit one round
// of 256 -- or R >= the longest contraction, where cutting deeper is impossible
inline int wgrad_slab_rows(const int64_t* tiles, const int* rows, int n) {
    int max_rows = 0;
    for (int i = 0; i < n; ++i) max_rows = rows[i] > max_rows ? rows[i] : max_rows;
    for (int R = W_STAGE;; R += W_STAGE) {
        int64_t wgs = 0;
        for (int i = 0; i < n; ++i) wgs += tiles[i] * wcdiv(rows[i], R);
        if (wgs <= W_ROUND || R >= max_rows) return R;
    }
}

enum WgradReduce { W_RED_NONE = 0, W_RED_LPQ1 = 1, W_RED_LPQ16 = 16 };      // lanes per output quad of wgrad256_reduce_kernel

// Everything a launch of the split form needs.  Workspace (floats): the partial tiles [S][Nn][Kk] of the split problems in order, then
// their partial bias sums [S][Nn] (each padded to a multiple of 4).
struct WgradSplitPlan {
    struct Prob {
        int S, slab, tiles, tiles_k, wg0;
        int64_t red0;                  // first float4 of this problem in the reduce kernel's index space
        int64_t ws_off, wsb_off;       // partial tiles / partial bias sums (floats)
    } p[W_MAXP];
    int n = 0, total = 0, per_xcd = 0, interleave = 0;
    int reduce = W_RED_NONE, reduce_grid = 0, bias_cb = 1, bias_blocks = 0;
    int64_t red_total = 0;             // float4s the reduce kernel folds
    int64_t ws_floats = 0;
    int R = 0;                         // the row search's answer
    int nimg = 0, slab0[W_MAXIMG] = {0, 0, 0, 0, 0, 0};     // multi-image convolution: first slab of each image
};

// The plan of n <= 12 problems.
//   img_rows == nullptr: a group; each problem gets S = ceil(M / R) BALANCED slabs of ceil32(ceil(M / S)) rows.
//   img_rows[nimg]: the problems are the nine taps of ONE convolution whose M axis runs over nimg images; every problem gets the same
//     slabs of R rows that never straddle an image (S = sum_i ceil(rows_i / R), image i starts at slab0[i]); the bias sums' region is
//     reserved whether or not a bias gradient is asked for.
//   taps: the problems share their operands (the taps of a convolution): consecutive workgroups take the same (slab, tile) of consecutive
//     problems when all are alike.
template <class P> WgradSplitPlan plan_wgrad_split(const P* pr, int n, bool taps, const int* img_rows = nullptr, int nimg = 0) {
    WgradSplitPlan pl;
    pl.n = n;
    pl.nimg = img_rows ? nimg : 0;
    int64_t tiles[W_MAXP], img_tiles[W_MAXIMG];
    int rows[W_MAXP];
    int64_t all_tiles = 0;
    for (int i = 0; i < n; ++i) {
        pl.p[i].tiles_k = (int)wcdiv(pr[i].Kk, W_TILE);
        pl.p[i].tiles = (int)wcdiv(pr[i].Nn, W_TILE) * pl.p[i].tiles_k;
        tiles[i] = pl.p[i].tiles;
        rows[i] = pr[i].M;
        all_tiles += tiles[i];
    }
    int S_all = 0;
    if (pl.nimg) {
        for (int i = 0; i < nimg; ++i) img_tiles[i] = all_tiles;       // every problem runs over every image
        pl.R = wgrad_slab_rows(img_tiles, img_rows, nimg);
        for (int i = 0; i < nimg; ++i) { pl.slab0[i] = S_all; S_all += (int)wcdiv(img_rows[i], pl.R); }
    } else {
        pl.R = wgrad_slab_rows(tiles, rows, n);
    }
    int maxS = 1, bias_nn = 0;
    for (int i = 0; i < n; ++i) {
        WgradSplitPlan::Prob& q = pl.p[i];
        if (pl.nimg) {
            q.S = S_all;
            q.slab = pl.R;
        } else {
            q.S = (int)wcdiv(pr[i].M, pl.R);
            if (q.S < 1) q.S = 1;
            q.slab = (int)wcdiv(wcdiv(pr[i].M, q.S), W_STAGE) * W_STAGE;
        }
        q.wg0 = pl.total;
        q.red0 = pl.red_total;
        q.ws_off = pl.ws_floats;
        pl.total += q.tiles * q.S;
        if (q.S > 1) {                 // unsplit problems are finished by the partial kernel itself
            pl.red_total += (int64_t)pr[i].Nn * pr[i].Kk / 4;
            pl.ws_floats += (int64_t)q.S * pr[i].Nn * pr[i].Kk;
            if (pr[i].gb && pr[i].Nn > bias_nn) bias_nn = pr[i].Nn;
        }
        maxS = q.S > maxS ? q.S : maxS;
    }
    const int64_t bias0 = pl.ws_floats;
    for (int i = 0; i < n; ++i) {
        pl.p[i].wsb_off = pl.nimg ? bias0 : pl.ws_floats;
        if (pl.p[i].S > 1 && (pr[i].gb || (pl.nimg && i == 0))) pl.ws_floats += ((int64_t)pl.p[i].S * pr[i].Nn + 3) / 4 * 4;
    }
    pl.per_xcd = (pl.total + 7) / 8;
    if (taps && n > 1) {
        pl.interleave = 1;
        for (int i = 1; i < n; ++i)
            if (pl.p[i].tiles != pl.p[0].tiles || pl.p[i].S != pl.p[0].S || pr[i].M != pr[0].M) pl.interleave = 0;
    }
    // the bias-gradient folds of the split problems ride in the reduce launch: its last bias_blocks workgroups, (problem, 256 columns) each
    if (bias_nn > 0) { pl.bias_cb = (bias_nn + 255) / 256; pl.bias_blocks = pl.bias_cb * n; }
    else if (pl.nimg) pl.bias_cb = (pr[0].Nn + 255) / 256;
    if (pl.red_total > 0 || pl.bias_blocks > 0) {
        if (pl.red_total > 0 && pl.red_total <= 32768 && maxS >= 16) {      // small output, deep split: 16 lanes share the walk over the slabs
            // (red_total * 16 is a multiple of 64, so the xor-shuffles never mix lanes of different quads with idle ones)
            pl.reduce = W_RED_LPQ16;
            pl.reduce_grid = (int)((pl.red_total * 16 + 255) / 256) + pl.bias_blocks;
        } else {
            pl.reduce = W_RED_LPQ1;
            const int64_t blocks = (pl.red_total + 255) / 256;
            pl.reduce_grid = (int)(blocks < 8192 ? blocks : 8192) + pl.bias_blocks;
        }
    }
    return pl;
}

// ---- workspace rules (floats; the entry points report bytes)
// dgx_wgrad_grouped_workspace_bytes: a group the loader-wave form takes needs none -- unless its launch checks can still send it to the
// split form: then the split form's size is reported.  So the size never depends on the form: the split form's wherever that form can
// run (n <= 12), nothing for the larger groups only the loader-wave form takes.
template <class P> int64_t wgrad_grouped_workspace_floats(const P* pr, int n) {
    if (!pr || n <= 0 || n > WL_MAXP || !wgrad_lw_may_fall_back(n)) return 0;
    return plan_wgrad_split(pr, n, false).ws_floats;
}
// dgx_wgrad_workspace_bytes, the single-problem entry point: a one-problem group.  Never 0 for a valid size: its launch refuses a null
// workspace, as it always has
inline int64_t wgrad_single_workspace_floats(int M, int Nn, int Kk) {
    if (M <= 0 || Nn <= 0 || Kk <= 0) return 0;
    const struct { int M, Nn, Kk; bool gb; } p = {M, Nn, Kk, false};
    const int64_t f = wgrad_grouped_workspace_floats(&p, 1);
    return f > 4 ? f : 4;
}
}  // namespace dgxplan
