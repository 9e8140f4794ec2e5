// Host check of divergen_amd/csrc/gemm_plan.h (which kernel form, tile and split-K plan a GEMM problem gets), driven by
// tests/test_host_gemm_plan.py:   gemm_plan_check <cases.txt>
// cases.txt, one case per line (written by the test from BENCH_GEMMS of tests/test_gpu_pins.py and tests/golden/gemm_plans.json):
//   pin  M N K mode res_bf16 ws  form bm bn           expected under default knobs at reserved CUs 0 and 16; form -1: LW or TWO
//   k192 M N K mode res_bf16 ws                       must take the resident-panel kernel at reserved CUs 0 and 16
//   row  ngrp Ms.. M N K mode res_bf16 conv ws lw reserved  form bm bn splits      a recorded dispatch of the parent library
//   tab  M N K mode res_bf16 relu ws  lw two_wg tile splitk k192  reserved  form bm bn splits      a table row of tests/_gemm_ref64.py: all
//        five knobs as dgx_dev_set takes them (tile = bm * 1000 + bn), reserved CUs, and what dgx_gemm_last_form must report
// Then the invariants of every plan over a grid of small shapes.  Prints "ok <cases> <plans>" and exits 0, or the first failure.
#include "../../divergen_amd/csrc/gemm_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace dgxplan;

static long g_plans = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("FAILED %s:%d  %s\n  ", __FILE__, __LINE__, #cond);        \
            printf(__VA_ARGS__);                                              \
            printf("\n");                                                     \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static bool same(const GemmPlan& a, const GemmPlan& b) {
    bool s = a.form == b.form && a.bm == b.bm && a.bn == b.bn && a.stages == b.stages && a.wg_per_cu == b.wg_per_cu && a.mc == b.mc &&
             a.splits == b.splits && a.kt_per_split == b.kt_per_split && a.tiles_n == b.tiles_n && a.total == b.total && a.per_xcd == b.per_xcd;
    for (int i = 0; i < MAXG; ++i) s = s && a.tile0[i] == b.tile0[i];
    return s;
}
// the seven tiles both launch tables (gemm_nt_launch, gemm_lw_launch) instantiate
static bool tile_instantiated(int bm, int bn) {
    static const int t[7][2] = {{256, 192}, {192, 192}, {128, 192}, {192, 256}, {128, 256}, {256, 128}, {128, 128}};
    for (auto& e : t)
        if (e[0] == bm && e[1] == bn) return true;
    return false;
}
static int cdiv(int a, int b) { return (a + b - 1) / b; }

// what must hold for every plan
static void invariants(const GemmProblem& q, const DevKnobs& dev, int reserved, const GemmPlan& p) {
    ++g_plans;
    const int nt = cdiv(q.K, BK);
#define WHERE "M %d N %d K %d mode %d ngrp %d ws %lld | lw %d 2wg %d tile %dx%d splitk %d k192 %d reserved %d -> form %d %dx%d splits %d x %d", q.M, q.N, q.K, \
              q.mode, q.ngrp, (long long)q.ws_bytes, dev.lw, dev.two_wg, dev.tile_bm, dev.tile_bn, dev.splitk, dev.k192, reserved, p.form, p.bm, p.bn, \
              p.splits, p.kt_per_split
    CHECK(p.form >= FORM_NT && p.form <= FORM_K192, WHERE);
    CHECK(p.splits >= 1 && (p.splits - 1) * p.kt_per_split < nt && nt <= p.splits * p.kt_per_split, WHERE);     // no empty split
    CHECK(8 * p.per_xcd >= p.total * p.splits, WHERE);
    CHECK(tile_instantiated(p.bm, p.bn) && nt_stages(p.bm, p.bn) != 0 && lw_has_tile(p.bm, p.bn), WHERE);
    CHECK(p.tiles_n == cdiv(q.N, p.bn), WHERE);
    if (q.ngrp > 0) {
        int run = 0;
        for (int i = 0; i < q.ngrp; ++i) {
            CHECK(p.tile0[i] == run, WHERE);
            run += cdiv(q.Ms[i], p.bm) * p.tiles_n;
        }
        CHECK(p.total == run && p.splits == 1 && p.kt_per_split == nt, WHERE);
        CHECK(p.form == FORM_LW || p.form == FORM_NT, WHERE);
    } else {
        CHECK(p.total == cdiv(q.M, p.bm) * cdiv(q.N, p.bn), WHERE);
        CHECK(p.splits == 1 || (int64_t)p.splits * q.M * q.N * 4 <= q.ws_bytes, WHERE);
    }
    if (p.form == FORM_TWO) CHECK(p.bm == 128 && p.bn == 192 && p.stages == 2 && p.wg_per_cu == 2, WHERE);
    else CHECK(p.wg_per_cu == 1 && p.stages == nt_stages(p.bm, p.bn) && p.mc == -1, WHERE);
    if (p.form == FORM_K192) CHECK(32 - reserved >= q.N / 192 && q.K == 192 && q.N % 192 == 0 && q.mode <= 4, WHERE);
#undef WHERE
}

static GemmPlan plan(const GemmProblem& q, const DevKnobs& dev, int reserved) {
    const GemmPlan p = plan_gemm(q, dev, reserved);
    invariants(q, dev, reserved, p);
    return p;
}

static int run_cases(const char* path) {
    std::ifstream in(path);
    CHECK(in.good(), "cannot read %s", path);
    std::string line;
    int n = 0, split_pin = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream s(line);
        std::string kind;
        s >> kind;
        GemmProblem q;
        q.k192_operands = true;                    // the tests' tensors are 16-byte aligned
        if (kind == "pin" || kind == "k192") {
            int form = FORM_K192, bm = 32, bn = 192, res_bf16;
            s >> q.M >> q.N >> q.K >> q.mode >> res_bf16 >> q.ws_bytes;
            q.res_bf16 = res_bf16;
            if (kind == "pin") s >> form >> bm >> bn;
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            for (int reserved = 0; reserved <= 2; reserved += 2) {       // dgx_set_reserved_cus(0 | 16): 0 | 2 CUs per XCD
                const GemmPlan p = plan(q, DevKnobs(), reserved);
                const int rbm = p.form == FORM_K192 ? 32 : p.bm, rbn = p.form == FORM_K192 ? 192 : p.bn;     // as dgx_gemm_last_form reports
                if (form < 0) CHECK(p.form == FORM_LW || p.form == FORM_TWO, "%s -> form %d", line.c_str(), p.form);
                else CHECK(p.form == form && rbm == bm && rbn == bn, "%s -> form %d %dx%d (reserved %d)", line.c_str(), p.form, rbm, rbn, 8 * reserved);
                if (q.M == 1024 && q.N == 1024 && q.K == 12544) { CHECK(p.splits > 1, "%s must split K", line.c_str()); ++split_pin; }
            }
        } else if (kind == "row") {
            int res_bf16, conv, lw, reserved, form, bm, bn, splits;
            s >> q.ngrp;
            CHECK(q.ngrp >= 0 && q.ngrp <= MAXG, "bad line: %s", line.c_str());
            for (int i = 0; i < q.ngrp; ++i) s >> q.Ms[i];
            s >> q.M >> q.N >> q.K >> q.mode >> res_bf16 >> conv >> q.ws_bytes >> lw >> reserved >> form >> bm >> bn >> splits;
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            q.res_bf16 = res_bf16; q.conv = conv != 0;
            DevKnobs dev;
            dev.lw = lw;
            const GemmPlan p = plan(q, dev, reserved / 8);
            if (form >= 0) {                       // (form -1: that launch of the parent library reported nothing)
                const bool k = p.form == FORM_K192;
                CHECK(p.form == form && (k ? 32 : p.bm) == bm && (k ? 192 : p.bn) == bn && (k ? 1 : p.splits) == splits,
                      "%s -> form %d %dx%d splits %d", line.c_str(), p.form, k ? 32 : p.bm, k ? 192 : p.bn, k ? 1 : p.splits);
            } else {
                CHECK(q.ngrp > 0 && lw == 0 && p.form == FORM_NT, "%s -> form %d", line.c_str(), p.form);
            }
        } else if (kind == "tab") {
            int res_bf16, relu, tile, reserved, form, bm, bn, splits;
            DevKnobs dev;
            s >> q.M >> q.N >> q.K >> q.mode >> res_bf16 >> relu >> q.ws_bytes >> dev.lw >> dev.two_wg >> tile >> dev.splitk >> dev.k192 >> reserved >> form >> bm >>
                bn >> splits;
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            q.res_bf16 = res_bf16; q.relu = relu != 0;
            dev.tile_bm = tile / 1000; dev.tile_bn = tile % 1000;                    // dgx_dev_set("gemm_tile")
            const GemmPlan p = plan(q, dev, (reserved + 7) / 8 > 24 ? 24 : (reserved + 7) / 8);      // dgx_set_reserved_cus
            const bool k = p.form == FORM_K192;
            CHECK(p.form == form && (k ? 32 : p.bm) == bm && (k ? 192 : p.bn) == bn && (k ? 1 : p.splits) == splits,
                  "%s -> form %d %dx%d splits %d x %d, per XCD %d", line.c_str(), p.form, k ? 32 : p.bm, k ? 192 : p.bn, k ? 1 : p.splits, p.kt_per_split, p.per_xcd);
        } else {
            CHECK(false, "bad line: %s", line.c_str());
        }
        ++n;
    }
    CHECK(split_pin == 2, "the split-K pin (1024, 1024, 12544) is missing");
    return n;
}

static void grid() {
    const int Ms[] = {1, 8, 127, 128, 129, 300, 4096}, Ns[] = {8, 128, 192, 200, 384, 1160}, Ks[] = {8, 64, 72, 192, 768, 832, 12544};
    for (int M : Ms)
        for (int N : Ns)
            for (int K : Ks)
                for (int mode = 0; mode <= 5; ++mode)
                    for (int bf = 0; bf <= (mode == 3 ? 1 : 0); ++bf)
                        for (int w = 0; w < 3; ++w) {
                            GemmProblem q;
                            q.M = M; q.N = N; q.K = K; q.mode = mode; q.res_bf16 = bf;
                            q.k192_operands = true;
                            q.ws_bytes = w == 0 ? 0 : w == 1 ? (int64_t)2 * M * N * 4 : (int64_t)1 << 40;      // none | two slabs | ample
                            const GemmPlan def = plan(q, DevKnobs(), 0);
                            for (int reserved = 1; reserved <= 24; reserved += 23) plan(q, DevKnobs(), reserved);
                            for (int conv = 0; conv <= 1; ++conv)
                                for (int relu = 0; relu <= (mode <= 1 ? 1 : 0); ++relu) {
                                    GemmProblem c = q;
                                    c.conv = conv; c.relu = relu;
                                    plan(c, DevKnobs(), 0);
                                }
                            for (int S = 1; S <= 5; ++S) {
                                DevKnobs dev;
                                dev.splitk = S;
                                const GemmPlan p = plan(q, dev, 0);
                                CHECK(p.splits <= S, "forced %d slabs -> %d", S, p.splits);
                            }
                            for (int lw = 0; lw <= 1; ++lw) {
                                DevKnobs dev;
                                dev.lw = lw;
                                const GemmPlan p = plan(q, dev, 0);
                                CHECK(p.form == (lw ? FORM_LW : p.form == FORM_TWO ? FORM_TWO : FORM_NT), "gemm_lw %d -> form %d", lw, p.form);
                            }
                            // every instantiated tile can be forced; the two that are not fall back to the library's choice
                            const int tiles[9][2] = {{256, 192}, {192, 192}, {128, 192}, {192, 256}, {128, 256}, {256, 128}, {128, 128}, {256, 256}, {192, 128}};
                            for (int t = 0; t < 9; ++t) {
                                DevKnobs dev;
                                dev.tile_bm = tiles[t][0]; dev.tile_bn = tiles[t][1];
                                const GemmPlan p = plan(q, dev, 0);
                                if (t < 7) CHECK(p.form == FORM_TWO || (p.bm == tiles[t][0] && p.bn == tiles[t][1]), "forced tile %d", t);
                                else CHECK(same(p, def), "tile %dx%d must fall back to the library's choice", tiles[t][0], tiles[t][1]);
                            }
                            // every knob at its "plan" value is the default plan
                            for (int v = 0; v < 4; ++v) {
                                DevKnobs dev;
                                if (v == 1) dev.two_wg = 1;
                                if (v == 2) dev.k192 = 1;
                                if (v == 3) { dev.two_wg = 1; dev.k192 = 1; }
                                CHECK(same(def, plan(q, dev, 0)), "knobs at their plan values change the plan (%d)", v);
                            }
                        }
    // the resident-panel kernel's own conditions, next to the grid's row counts (which are all below its threshold)
    for (int N = 192; N <= 6144; N += 192)
        for (int reserved = 0; reserved <= 24; ++reserved) {
            GemmProblem q;
            q.M = 32768; q.N = N; q.K = 192; q.mode = 1; q.k192_operands = true;
            CHECK((plan(q, DevKnobs(), reserved).form == FORM_K192) == (32 - reserved >= N / 192), "k192 feasibility N %d reserved %d", N, reserved);
            q.k192_operands = false;
            CHECK(plan(q, DevKnobs(), reserved).form != FORM_K192, "unaligned operands");
        }
    // grouped convolutions
    const int sets[][MAXG] = {{2048, 512, 128, 30, 4, 0}, {32768, 8192, 2048, 30, 4, 0}, {1, 0, 0, 0, 0, 0}, {127, 129, 0, 0, 0, 0}, {32768, 8192, 2048, 512, 128, 50},
                              {300, 300, 300, 300, 300, 300}};
    for (auto& set : sets)
        for (int N : {8, 64, 128, 136, 256})
            for (int K : {576, 2304})
                for (int lw = -1; lw <= 1; ++lw) {
                    GemmProblem q;
                    q.N = N; q.K = K; q.mode = 1; q.conv = true;
                    for (int i = 0; i < MAXG && set[i] > 0; ++i) q.Ms[q.ngrp++] = set[i];
                    DevKnobs dev;
                    dev.lw = lw;
                    const GemmPlan p = plan(q, dev, 0);
                    CHECK(p.form == (lw == 0 ? FORM_NT : FORM_LW) && p.bn == (N > 128 ? 256 : 128) && (p.bm == 128 || (p.bm == 192 && N > 128)), "grouped N %d", N);
                }
}

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: gemm_plan_check <cases.txt>");
    const int n = run_cases(argv[1]);
    grid();
    printf("ok %d %ld\n", n, g_plans);
    return 0;
}
