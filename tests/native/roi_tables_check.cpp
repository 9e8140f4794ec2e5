// Host check of divergen_amd/csrc/roi_tables.h: the real header code run with bounds-checked host arrays in place of the kernels' LDS,
// sized exactly as the launches size them.  Reads request lines from the file named on the command line (floats as the hexadecimal bits
// of their fp32 value), asserts that every index the header code and the kernels' loops over its results form is in range, and prints
// the geometry for tests/test_host_roi_ref.py to compare with the float64 restatement's:
//   pool   nl H.. W.. C R ph pw nhwc aligned16           -> pool <vec|sep> ok bpb nsplit spy spx tbl sm
//   gplan  nl H.. W.. N C ph pw                          -> gplan supported tw th total tiles_x.. tiles_y..
//   crop   S                                             -> crop slices
//   roi    nl min_level H.. W.. scale0 aligned ph pw sr roi[5]
//          -> roi lvl gh gw count sw sh bin_w bin_h Y <ph x: base n w[n]> X <pw x: base n w[n]>
//   gather nl min_level H.. W.. scale0 aligned N C ph pw sr R roi[5 R]
//          -> one line per tile: tile l n y0 x0 <hits x: r i_lo i_hi>; and checks that the hit list and the bin ranges are supersets of
//             what the restricted tables weigh (a box that is not listed weighs no pixel of the tile, a bin outside a range weighs none)
// The last line is `ok <requests> <checked indices>`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../divergen_amd/csrc/roi_tables.h"

using namespace roitab;

static long long g_checked = 0;
static std::string g_line;

[[noreturn]] static void fail(const char* what, long long a = 0, long long b = 0, long long c = 0) {
    std::printf("FAIL %s (%lld %lld %lld) on: %s\n", what, a, b, c, g_line.c_str());
    std::exit(1);
}

// a float array that checks every index; + int gives the view from that offset, as pointer arithmetic would
struct Chk {
    float* p;
    int lo, hi;
    float& operator[](int k) const {
        ++g_checked;
        if (k < lo || k >= hi) fail("index out of range", k, lo, hi);
        return p[k];
    }
    Chk operator+(int d) const { return Chk{p + d, lo - d, hi - d}; }
};

static float fbits(std::istream& in) {
    std::string t;
    in >> t;
    const uint32_t u = (uint32_t)std::strtoul(t.c_str(), nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static unsigned bitsf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Levels {
    int nl, min_level, H[MAX_LEVELS], W[MAX_LEVELS];
    float scale[MAX_LEVELS];
    int aligned;
};
static void read_maps(std::istream& in, Levels& L, bool with_min) {
    in >> L.nl;
    if (L.nl < 1 || L.nl > MAX_LEVELS) fail("levels");
    L.min_level = 0;
    if (with_min) in >> L.min_level;
    for (int l = 0; l < L.nl; ++l) in >> L.H[l];
    for (int l = 0; l < L.nl; ++l) in >> L.W[l];
}
static void read_scales(std::istream& in, Levels& L) {
    const float s0 = fbits(in);
    in >> L.aligned;
    for (int l = 0; l < L.nl; ++l) L.scale[l] = L.nl > 1 ? 1.0f / (float)(1 << (L.min_level + l)) : s0;   // fill_levels / the gather entry
    if (L.nl > 1) L.aligned = 1;
}

static void do_pool(std::istream& in) {
    Levels L;
    int C, R, ph, pw, nhwc, a16;
    read_maps(in, L, false);
    in >> C >> R >> ph >> pw >> nhwc >> a16;
    const PoolPlan p = plan_pool(L.H, L.W, L.nl, C, R, ph, pw, nhwc);
    if (p.ok) {
        if (p.bpb < 1 || p.nsplit < 1 || (long long)p.nsplit * p.bpb < ph * pw || (long long)(p.nsplit - 1) * p.bpb >= ph * pw) fail("slices do not cover the bins");
        if (p.sm > LDS_BYTES) fail("LDS");
    }
    std::printf("pool %s %d %d %d %d %d %zu %zu\n", pool_wants_vec(nhwc, C, a16 != 0) ? "vec" : "sep", (int)p.ok, p.bpb, p.nsplit, p.spy, p.spx, p.tbl, p.sm);
}

static void do_gplan(std::istream& in) {
    Levels L;
    int N, C, ph, pw;
    read_maps(in, L, false);
    in >> N >> C >> ph >> pw;
    if (!gather_supported(C, ph, pw)) { std::printf("gplan 0\n"); return; }
    const GatherPlan p = plan_gather(L.H, L.W, L.nl, N, C);
    std::printf("gplan 1 %d %d %d", p.tw, p.th, p.total);
    for (int l = 0; l < L.nl; ++l) std::printf(" %d", p.tiles_x[l]);
    for (int l = 0; l < L.nl; ++l) std::printf(" %d", p.tiles_y[l]);
    std::printf("\n");
}

// one RoI through the table build of roi_align_sep_kernel / roi_align_vec_kernel, LDS laid out as launch_pool sizes it
static void do_roi(std::istream& in) {
    Levels L;
    int ph, pw, sr;
    float roi[5];
    read_maps(in, L, true);
    read_scales(in, L);
    in >> ph >> pw >> sr;
    for (float& v : roi) v = fbits(in);
    const PoolPlan p = plan_pool(L.H, L.W, L.nl, 8, 1, ph, pw, 1);
    std::vector<float> lds(p.tbl / 4, -1.0f);             // WY [ph][spy], WX [pw][spx], then the spans
    const int ny = ph * p.spy, nx = pw * p.spx;
    if ((size_t)(ny + nx) * 4 + (size_t)(ph + pw) * sizeof(Span) != p.tbl) fail("table bytes");
    Chk WY{lds.data(), 0, ny}, WX{lds.data() + ny, 0, nx};
    std::vector<Span> SY(ph), SX(pw);
    const int lvl = L.nl > 1 ? assign_level(roi, L.min_level, L.nl) : 0;
    if (lvl < 0 || lvl >= L.nl) fail("level");
    const int H = L.H[lvl], W = L.W[lvl];
    const RoiGeom G = roi_geom(roi, L.scale[lvl], ph, pw, sr, L.aligned != 0);
    for (int tid = 0; tid < 256; ++tid) {
        build_axis_table(WY, SY.data(), ph, p.spy, G.sh, G.bin_h, G.gh, H, tid, 0);
        build_axis_table(WX, SX.data(), pw, p.spx, G.sw, G.bin_w, G.gw, W, tid, 64);
    }
    std::printf("roi %d %d %d %08x %08x %08x %08x %08x Y", lvl, G.gh, G.gw, bitsf(G.count), bitsf(G.sw), bitsf(G.sh), bitsf(G.bin_w), bitsf(G.bin_h));
    for (int ax = 0; ax < 2; ++ax) {
        const int nb = ax ? pw : ph, stride = ax ? p.spx : p.spy, extent = ax ? W : H;
        const Span* sp = ax ? SX.data() : SY.data();
        const Chk T = ax ? WX : WY;
        if (ax) std::printf(" X");
        for (int i = 0; i < nb; ++i) {
            // what the kernels do with a span: rows base .. base + n - 1 of the map, weights w[0 .. n - 1] of the bin's table row
            if (sp[i].n < 0 || sp[i].n > stride || sp[i].base < 0 || sp[i].base + sp[i].n > extent) fail("span", i, sp[i].base, sp[i].n);
            std::printf(" %d %d", sp[i].base, sp[i].n);
            const Chk w = T + i * stride;
            for (int k = 0; k < sp[i].n; ++k) std::printf(" %08x", bitsf(w[k]));
            for (int k = sp[i].n; k < stride; ++k)
                if (w[k] != 0.0f) fail("weight behind the span", i, k);
        }
    }
    std::printf("\n");
}

// the whole launch of roi_pool_bwd_gather_kernel on the host, tile by tile, with its shared arrays checked
template <int TH> static void gather_tiles(const Levels& L, const GatherPlan& pl, int N, int C, int ph, int pw, int sr, int R, const std::vector<float>& rois) {
    const int CV = C >> 3, TW = 256 / CV;
    std::vector<float> wy_s(GT_QB * GT_PMAX * TH), wx_s(GT_QB * GT_PMAX * GT_TWMAX), full(GT_PMAX * GT_TWMAX);
    std::vector<int> list(256);
    for (int t = 0; t < pl.total; ++t) {
        int l = 0;
        while (l + 1 < L.nl && t >= pl.tile0[l + 1]) ++l;
        int local = t - pl.tile0[l];
        const int H = L.H[l], W = L.W[l], txn = pl.tiles_x[l], tyn = pl.tiles_y[l];
        const int n = local / (txn * tyn);
        local -= n * txn * tyn;
        const int y0 = (local / txn) * TH, x0 = (local % txn) * TW;
        if (n < 0 || n >= N || y0 >= H || x0 >= W) fail("tile", t, y0, x0);
        std::printf("tile %d %d %d %d", l, n, y0, x0);
        for (int base = 0; base < R; base += 256) {
            int hits = 0;
            for (int tid = 0; tid < 256; ++tid) {
                const int r = base + tid;
                if (r >= R) break;
                const float* roi = &rois[5 * (size_t)r];
                const int lvl = L.nl > 1 ? assign_level(roi, L.min_level, L.nl) : 0;
                if ((int)roi[0] != n || lvl != l) continue;
                const RoiGeom G = roi_geom(roi, L.scale[l], ph, pw, sr, L.aligned != 0);
                const bool hit = gather_hit(G, ph, pw, y0, x0, TH, TW);
                if (hit) {
                    if (hits >= 256) fail("list");
                    list[hits++] = r;
                }
                // superset: the restricted tables of this box
                bool anyy = false, anyx = false;
                int i_lo = 0, i_hi = 0;
                if (hit) gather_bin_range((float)(y0 - 1), (float)(y0 + TH), G.sh, G.bin_h, ph, i_lo, i_hi);
                if (i_lo < 0 || i_hi > ph) fail("i range", i_lo, i_hi);
                for (int i = 0; i < ph; ++i) {
                    Chk w{full.data(), 0, TH};
                    gather_axis_rows(w, TH, i, G.sh, G.bin_h, G.gh, H, y0);
                    bool nz = false;
                    for (int k = 0; k < TH; ++k) nz = nz || w[k] != 0.0f;
                    anyy = anyy || nz;
                    if (hit && nz && (i < i_lo || i >= i_hi)) fail("bin row outside the i range weighs the tile", r, i, y0);
                }
                for (int j = 0; j < pw; ++j) {
                    Chk w{full.data() + j * GT_TWMAX, 0, TW};
                    gather_axis_rows(w, TW, j, G.sw, G.bin_w, G.gw, W, x0);
                    for (int k = 0; k < TW; ++k) anyx = anyx || w[k] != 0.0f;
                }
                if (hit)
                    for (int tx = 0; tx < TW; ++tx) {
                        int j_lo, j_hi;
                        const float xf = (float)(x0 + tx);
                        gather_bin_range(xf - 1.0f, xf + 1.0f, G.sw, G.bin_w, pw, j_lo, j_hi);
                        if (j_lo < 0 || j_hi > pw) fail("j range", j_lo, j_hi);
                        for (int j = 0; j < pw; ++j)
                            if (full[j * GT_TWMAX + tx] != 0.0f && (j < j_lo || j >= j_hi)) fail("bin column outside the j range weighs the pixel", r, j, x0 + tx);
                    }
                if (!hit && anyy && anyx) fail("a box that is not listed weighs the tile", r, y0, x0);
            }
            // the resident batches: tables into WY[GT_QB][GT_PMAX][TH] / WX[GT_QB][GT_PMAX][GT_TWMAX] as the kernel indexes them
            for (int q0 = 0; q0 < hits; q0 += GT_QB) {
                const int nq = hits - q0 < GT_QB ? hits - q0 : GT_QB;
                for (int tid = 0; tid < 256; ++tid) {
                    const int q = tid >> 5, t5 = tid & 31;
                    if (q >= nq) continue;
                    const int rr = list[q0 + q];
                    const RoiGeom G = roi_geom(&rois[5 * (size_t)rr], L.scale[l], ph, pw, sr, L.aligned != 0);
                    if (t5 < 16) {
                        if (t5 < ph) gather_axis_rows(Chk{wy_s.data() + (q * GT_PMAX + t5) * TH, 0, TH}, TH, t5, G.sh, G.bin_h, G.gh, H, y0);
                    } else if (t5 - 16 < pw) {
                        gather_axis_rows(Chk{wx_s.data() + (q * GT_PMAX + t5 - 16) * GT_TWMAX, 0, TW}, TW, t5 - 16, G.sw, G.bin_w, G.gw, W, x0);
                    }
                    if (t5 == 0) {
                        int i_lo, i_hi;
                        gather_bin_range((float)(y0 - 1), (float)(y0 + TH), G.sh, G.bin_h, ph, i_lo, i_hi);
                        std::printf(" %d %d %d", rr, i_lo, i_hi);
                    }
                }
            }
        }
        std::printf("\n");
    }
}

static void do_gather(std::istream& in) {
    Levels L;
    int N, C, ph, pw, sr, R;
    read_maps(in, L, true);
    read_scales(in, L);
    in >> N >> C >> ph >> pw >> sr >> R;
    std::vector<float> rois(5 * (size_t)R + 1);
    for (int k = 0; k < 5 * R; ++k) rois[k] = fbits(in);
    if (!in) fail("short request");
    if (!gather_supported(C, ph, pw)) fail("unsupported gather shape");
    const GatherPlan pl = plan_gather(L.H, L.W, L.nl, N, C);
    if (pl.tw > GT_TWMAX || ph > GT_PMAX || pw > GT_PMAX) fail("tile");
    if (pl.th == 4) gather_tiles<4>(L, pl, N, C, ph, pw, sr, R, rois);
    else gather_tiles<8>(L, pl, N, C, ph, pw, sr, R, rois);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    long long reqs = 0;
    while (std::getline(f, g_line)) {
        if (g_line.empty()) continue;
        std::istringstream in(g_line);
        std::string kind;
        in >> kind;
        if (kind == "pool") do_pool(in);
        else if (kind == "gplan") do_gplan(in);
        else if (kind == "crop") { int S; in >> S; std::printf("crop %d\n", mask_crop_slices(S)); }
        else if (kind == "roi") do_roi(in);
        else if (kind == "gather") do_gather(in);
        else fail("unknown request");
        if (!in) fail("short request");
        ++reqs;
    }
    std::printf("ok %lld %lld\n", reqs, g_checked);
    return 0;
}
