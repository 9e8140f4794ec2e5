// Host check of divergen_amd/csrc/wgrad_plan.h (which form runs a group of weight gradients, how the split form cuts its rows, what
// workspace every entry point reports), driven by tests/test_host_wgrad_plan.py:   wgrad_plan_check <cases.txt>
// cases.txt, one case per line (written by the test from tests/golden/wgrad_plans.json and the tables of tests/_conv_ref64.py):
//   group  n (M Nn Kk gb) x n  form0 form1 form2  ws0 ws1 ws2      recorded from the parent library at wgrad_lw 0 / 1 / 2 (bytes)
//   single M Nn Kk                                                 the one-problem entry point: the size of a one-problem group
//   conv   N H W Cin Cout  ws ws_bias                              recorded
//   multi  n (N H W) x n  Cin Cout  ws                             recorded
//   planconv  N H W Cin Cout        -> prints  planconv S slab stages reduce ws_floats
//   planmulti n (N H W) x n Cin Cout -> prints planmulti R nslabs.. ws_floats
//   plangroup n (M Nn Kk) x n       -> prints  plangroup reduce (S slab) x n
// Then the invariants of every plan over a sweep of small sizes.  Prints "ok <cases> <plans>" last and exits 0, or the first failure.
#include "../../divergen_amd/csrc/wgrad_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

using namespace dgxplan;

struct Prob { int M, Nn, Kk; bool gb; };

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

static std::string show(const Prob* pr, int n, const int* img, int nimg) {
    std::ostringstream s;
    for (int i = 0; i < n; ++i) s << "(" << pr[i].M << "," << pr[i].Nn << "," << pr[i].Kk << "," << pr[i].gb << ")";
    for (int i = 0; i < nimg; ++i) s << " img " << img[i];
    return s.str();
}

// what must hold for every plan of the split form
static WgradSplitPlan split(const Prob* pr, int n, bool taps, const int* img = nullptr, int nimg = 0) {
    const WgradSplitPlan p = plan_wgrad_split(pr, n, taps, img, nimg);
    ++g_plans;
    const std::string w = show(pr, n, img, nimg);
#define WHERE "%s", w.c_str()
    CHECK(p.n == n && p.R >= W_STAGE && p.R % W_STAGE == 0, WHERE);
    int total = 0, max_rows = 0;
    int64_t red = 0;
    std::vector<std::pair<int64_t, int64_t>> regions;
    bool any_split = false, any_bias = false;
    for (int i = 0; i < n; ++i) {
        const WgradSplitPlan::Prob& q = p.p[i];
        CHECK(q.tiles_k == (pr[i].Kk + 255) / 256 && q.tiles == ((pr[i].Nn + 255) / 256) * q.tiles_k, WHERE);
        CHECK(q.S >= 1 && q.slab >= W_STAGE && q.slab % W_STAGE == 0, WHERE);
        CHECK(q.wg0 == total, WHERE);
        total += q.tiles * q.S;
        if (!nimg) {               // every row of M lies in exactly one slab: S slabs of `slab` rows cover M, the last one is not empty
            CHECK((int64_t)q.slab * q.S >= pr[i].M && (int64_t)q.slab * (q.S - 1) < pr[i].M, WHERE);
            max_rows = std::max(max_rows, pr[i].M);
        }
        if (q.S > 1) {
            CHECK(q.red0 == red, WHERE);               // reduce offsets: increasing, dense
            red += (int64_t)pr[i].Nn * pr[i].Kk / 4;
            regions.push_back({q.ws_off, q.ws_off + (int64_t)q.S * pr[i].Nn * pr[i].Kk});
            if (pr[i].gb) { regions.push_back({q.wsb_off, q.wsb_off + (int64_t)q.S * pr[i].Nn}); any_bias = true; }
            any_split = true;
        }
    }
    if (nimg) {                    // slabs of R rows per image: image i owns slabs slab0[i] .. slab0[i+1] - 1, none straddles
        int s = 0;
        for (int i = 0; i < nimg; ++i) {
            CHECK(p.slab0[i] == s, WHERE);
            const int nsl = (img[i] + p.R - 1) / p.R;
            CHECK((int64_t)nsl * p.R >= img[i] && (int64_t)(nsl - 1) * p.R < img[i], WHERE);
            s += nsl;
            max_rows = std::max(max_rows, img[i]);
        }
        for (int i = 0; i < n; ++i) CHECK(p.p[i].S == s && p.p[i].slab == p.R, WHERE);
    }
    CHECK(p.total == total && 8 * p.per_xcd >= p.total && 8 * (p.per_xcd - 1) < p.total, WHERE);
    CHECK(p.total <= W_ROUND || p.R >= max_rows, WHERE);
    CHECK(p.red_total == red, WHERE);
    std::sort(regions.begin(), regions.end());
    int64_t end = 0;
    for (auto& r : regions) {      // workspace regions: disjoint, inside the reported size
        CHECK(r.first >= end && r.second > r.first, WHERE);
        end = r.second;
    }
    CHECK(end <= p.ws_floats && (any_split || p.ws_floats == 0), WHERE);
    CHECK((p.reduce != W_RED_NONE) == any_split && (p.bias_blocks > 0) == any_bias, WHERE);
    if (any_split) {
        const int main_blocks = p.reduce_grid - p.bias_blocks;
        CHECK(main_blocks >= 1 && main_blocks <= std::max<int64_t>(8192, (red * 16 + 255) / 256), WHERE);
        if (p.reduce == W_RED_LPQ16) CHECK(red <= 32768 && (int64_t)main_blocks * 256 >= red * 16, WHERE);
        if (any_bias) CHECK(p.bias_blocks == p.bias_cb * n, WHERE);
        for (int i = 0; i < n; ++i)
            if (p.p[i].S > 1 && pr[i].gb) CHECK(p.bias_cb * 256 >= pr[i].Nn, WHERE);
    }
    if (p.interleave) {
        CHECK(taps && n > 1, WHERE);
        for (int i = 1; i < n; ++i) CHECK(p.p[i].tiles == p.p[0].tiles && p.p[i].S == p.p[0].S, WHERE);
    }
#undef WHERE
    return p;
}

static void taps_of(Prob (&pr)[9], int rows, int Cin, int Cout, bool bias) {
    for (int t = 0; t < 9; ++t) pr[t] = {rows, Cout, Cin, bias && t == 0};
}
static int pad_rows(int N, int H, int W) { return N * (H + 2) * (W + 2); }

// what every group must satisfy, whatever the knob
static void group_invariants(const Prob* pr, int n) {
    DevKnobs dev;
    const WgradLwPlan lw = plan_wgrad_lw(pr, n);
    int items = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(lw.item0[i] == items && lw.tiles_k[i] == (pr[i].Kk + 191) / 192, "%s", show(pr, n, nullptr, 0).c_str());
        items += ((pr[i].Nn + 255) / 256) * lw.tiles_k[i];
    }
    CHECK(lw.total == items && 8 * lw.per_xcd >= items, "%s", show(pr, n, nullptr, 0).c_str());
    for (int i = n; i < WL_MAXP; ++i) CHECK(lw.item0[i] == 0x7fffffff, "unused item0");
    const int64_t ws = wgrad_grouped_workspace_floats(pr, n);
    dev.wgrad_lw = 0;
    CHECK(!wgrad_lw_wants(pr, n, dev), "knob 0");
    // a group the loader-wave form may refuse, with n <= 12, reports the split form's workspace (whatever the form: the size does not
    // take the knobs); a larger one has no fall-back and no workspace
    if (n <= W_MAXP) CHECK(wgrad_lw_may_fall_back(n) && ws == split(pr, n, false).ws_floats, "%s", show(pr, n, nullptr, 0).c_str());
    else CHECK(ws == 0 && !wgrad_lw_may_fall_back(n), "n > 12");
}

static int run_cases(const char* path) {
    std::ifstream in(path);
    CHECK(in.good(), "cannot read %s", path);
    std::string line;
    int cases = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream s(line);
        std::string kind;
        s >> kind;
        if (kind == "group") {
            int n;
            s >> n;
            CHECK(n >= 1 && n <= 64, "bad line: %s", line.c_str());
            std::vector<Prob> pr(n);
            for (auto& p : pr) { int gb; s >> p.M >> p.Nn >> p.Kk >> gb; p.gb = gb != 0; }
            int form[3];
            long long ws[3];
            s >> form[0] >> form[1] >> form[2] >> ws[0] >> ws[1] >> ws[2];
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            for (int knob = 0; knob <= 2; ++knob) {
                DevKnobs dev;
                dev.wgrad_lw = knob;
                const int f = n <= WL_MAXP && wgrad_lw_wants(pr.data(), n, dev) ? 1 : 0;          // dgx_wgrad_grouped_form
                const long long b = wgrad_grouped_workspace_floats(pr.data(), n) * 4;
                CHECK(f == form[knob] && b == ws[knob], "%s -> knob %d form %d ws %lld", line.c_str(), knob, f, b);
            }
            if (n <= WL_MAXP) group_invariants(pr.data(), n);
        } else if (kind == "plangroup") {
            int n;
            s >> n;
            CHECK(n >= 1 && n <= W_MAXP, "bad line: %s", line.c_str());
            std::vector<Prob> pr(n);
            for (auto& p : pr) { s >> p.M >> p.Nn >> p.Kk; p.gb = true; }
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            const WgradSplitPlan p = split(pr.data(), n, false);
            printf("plangroup %d", p.reduce);
            for (int i = 0; i < n; ++i) printf(" %d %d", p.p[i].S, p.p[i].slab);
            printf("\n");
        } else if (kind == "single") {
            Prob p = {0, 0, 0, false};
            s >> p.M >> p.Nn >> p.Kk;
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            const int64_t f = wgrad_single_workspace_floats(p.M, p.Nn, p.Kk);
            if (p.M <= 0 || p.Nn <= 0 || p.Kk <= 0) CHECK(f == 0, "%s", line.c_str());
            else CHECK(f >= 4 && f == std::max<int64_t>(4, split(&p, 1, false).ws_floats), "%s", line.c_str());
        } else if (kind == "conv" || kind == "planconv") {
            int N, H, W, Cin, Cout;
            long long ws = 0, wsb = 0;
            s >> N >> H >> W >> Cin >> Cout;
            if (kind == "conv") s >> ws >> wsb;
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            Prob pr[9];
            taps_of(pr, pad_rows(N, H, W), Cin, Cout, false);
            const WgradSplitPlan a = split(pr, 9, true);
            taps_of(pr, pad_rows(N, H, W), Cin, Cout, true);
            const WgradSplitPlan b = split(pr, 9, true);
            if (kind == "conv")
                CHECK(a.ws_floats * 4 == ws && b.ws_floats * 4 == wsb, "%s -> %lld %lld", line.c_str(), (long long)a.ws_floats * 4, (long long)b.ws_floats * 4);
            else
                printf("planconv %d %d %d %d %lld\n", b.p[0].S, b.p[0].slab, b.p[0].slab / W_STAGE, b.reduce, (long long)b.ws_floats);
            CHECK(b.interleave == 1 && a.p[0].S == b.p[0].S, "%s", line.c_str());
        } else if (kind == "multi" || kind == "planmulti") {
            int n, Cin, Cout, rows[W_MAXIMG];
            long long ws = 0;
            s >> n;
            CHECK(n >= 1 && n <= W_MAXIMG, "bad line: %s", line.c_str());
            for (int i = 0; i < n; ++i) { int N, H, W; s >> N >> H >> W; rows[i] = pad_rows(N, H, W); }
            s >> Cin >> Cout;
            if (kind == "multi") s >> ws;
            CHECK(!s.fail(), "bad line: %s", line.c_str());
            Prob pr[9];
            taps_of(pr, rows[0], Cin, Cout, true);
            // (one image: the entry point delegates to the per-image plan)
            const WgradSplitPlan p = n == 1 ? split(pr, 9, true) : split(pr, 9, true, rows, n);
            if (kind == "multi") {
                CHECK(p.ws_floats * 4 == ws, "%s -> %lld", line.c_str(), (long long)p.ws_floats * 4);
                if (n > 1) {           // the size does not depend on whether a bias gradient is asked for
                    taps_of(pr, rows[0], Cin, Cout, false);
                    CHECK(plan_wgrad_split(pr, 9, true, rows, n).ws_floats == p.ws_floats, "%s", line.c_str());
                }
            } else {
                printf("planmulti %d", p.R);
                for (int i = 0; i < n; ++i) printf(" %d", (i + 1 < n ? p.slab0[i + 1] : p.p[0].S) - p.slab0[i]);
                printf(" %lld\n", (long long)p.ws_floats);
            }
        } else {
            CHECK(false, "bad line: %s", line.c_str());
        }
        ++cases;
    }
    return cases;
}

static void sweep() {
    const int Ms[] = {1, 31, 32, 33, 64, 100, 300, 1000, 1023, 1024, 1064, 4000, 17000};
    const int Ws[] = {8, 64, 72, 200, 256, 264, 512, 520, 1536};
    uint32_t seed = 12345;
    auto rnd = [&](int n) { seed = seed * 1664525u + 1013904223u; return (int)((seed >> 8) % (uint32_t)n); };
    // alike problems: n across 12 / 13 and up to 32
    for (int n : {1, 2, 3, 9, 11, 12, 13, 31, 32})
        for (int M : Ms)
            for (int Nn : Ws)
                for (int Kk : Ws)
                    for (int gb = 0; gb <= 1; ++gb) {
                        std::vector<Prob> pr(n, Prob{M, Nn, Kk, gb != 0});
                        group_invariants(pr.data(), n);
                        if (n <= W_MAXP) split(pr.data(), n, true);
                    }
    // mixed groups
    for (int it = 0; it < 20000; ++it) {
        const int n = 1 + rnd(14);
        std::vector<Prob> pr(n);
        for (auto& p : pr) p = {Ms[rnd(13)] + 8 * rnd(2), Ws[rnd(9)], Ws[rnd(9)], rnd(2) != 0};
        group_invariants(pr.data(), n);
    }
    // the thresholds of the loader-wave form
    {
        DevKnobs dev;
        std::vector<Prob> pr(4, Prob{1024, 1536, 1536, true});                 // 4 x 48 = 192 items, fill 0.75
        CHECK(wgrad_lw_wants(pr.data(), 4, dev), "192 items");
        pr[3].Kk = 1344;                                                       // 186 items
        CHECK(!wgrad_lw_wants(pr.data(), 4, dev), "186 items");
        pr[3].Kk = 1536; pr[2].M = 1023;
        CHECK(!wgrad_lw_wants(pr.data(), 4, dev), "M 1023");
        dev.wgrad_lw = 2;
        CHECK(!wgrad_lw_wants(pr.data(), 4, dev), "M 1023, forced");
        std::vector<Prob> big(8, Prob{1024, 1536, 1536, false});
        dev.wgrad_lw = 1;
        big[7] = {1024, 43 * 256, 192, false};                                 // 379 items of 512: 0.7402
        CHECK(wgrad_lw_wants(big.data(), 8, dev), "379 items");
        big[7] = {1024, 42 * 256, 192, false};                                 // 378: 0.7383
        CHECK(!wgrad_lw_wants(big.data(), 8, dev), "378 items");
        std::vector<Prob> many(33, Prob{1024, 1536, 1536, false});
        CHECK(wgrad_lw_wants(many.data(), 32, dev) && !wgrad_lw_wants(many.data(), 33, dev), "32 / 33 problems");
    }
    // convolutions: one image and several
    const int geo[][3] = {{1, 1, 1}, {1, 2, 2}, {2, 3, 3}, {2, 7, 9}, {2, 12, 12}, {2, 32, 32}, {2, 56, 56}, {2, 128, 128}};
    for (int Cin : {8, 64, 264, 320})
        for (int Cout : {8, 64, 256, 264})
            for (int bias = 0; bias <= 1; ++bias) {
                Prob pr[9];
                for (auto& g : geo) {
                    taps_of(pr, pad_rows(g[0], g[1], g[2]), Cin, Cout, bias != 0);
                    CHECK(split(pr, 9, true).interleave == 1, "taps interleave");
                }
                for (int n = 2; n <= W_MAXIMG; ++n)
                    for (int first = 0; first + n <= 8; ++first) {
                        int rows[W_MAXIMG];
                        for (int i = 0; i < n; ++i) rows[i] = pad_rows(geo[7 - first - i][0], geo[7 - first - i][1], geo[7 - first - i][2]);
                        taps_of(pr, rows[0], Cin, Cout, bias != 0);
                        const WgradSplitPlan p = split(pr, 9, true, rows, n);
                        CHECK(p.interleave == 1 && p.reduce != W_RED_NONE &&
                                  p.ws_floats == 9 * (int64_t)p.p[0].S * Cin * Cout + ((int64_t)p.p[0].S * Cout + 3) / 4 * 4,
                              "multi Cin %d Cout %d n %d", Cin, Cout, n);
                    }
            }
}

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: wgrad_plan_check <cases.txt>");
    const int n = run_cases(argv[1]);
    sweep();
    printf("ok %d %ld\n", n, g_plans);
    return 0;
}
