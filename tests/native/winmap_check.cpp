// CPU check of divergen_amd/csrc/winmap.h (the header is shared by the HIP kernels): the compact and the classic window order against a
// brute-force enumeration of the reference's pad -> roll -> partition (swintransformer.py:216-233), the 32- and 64-bit instantiations
// of the map against each other, and the host validity check against the per-entry-point checks it replaced.
// Prints "ok <compact cases> <classic cases> <validity cases>" or the first mismatch.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../divergen_amd/csrc/winmap.h"
#include <cstdio>
#include <vector>

// ---- classic order: brute force ----
// table[row] = token index or -1, built the way the reference does it: the padded grid, rolled by -shift, cut into windows
static std::vector<int> brute_classic(int B, int H, int W, int ws, int shift) {
    const int nWh = (H + ws - 1) / ws, nWw = (W + ws - 1) / ws, Hp = nWh * ws, Wp = nWw * ws;
    std::vector<int> padded((size_t)B * Hp * Wp, -1), rolled(padded.size()), table(padded.size());
    for (int b = 0; b < B; ++b)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w) padded[((size_t)b * Hp + h) * Wp + w] = (b * H + h) * W + w;
    for (int b = 0; b < B; ++b)                       // torch.roll(x, shifts=(-shift, -shift)): rolled[h] = x[(h + shift) % Hp]
        for (int h = 0; h < Hp; ++h)
            for (int w = 0; w < Wp; ++w) rolled[((size_t)b * Hp + h) * Wp + w] = padded[((size_t)b * Hp + (h + shift) % Hp) * Wp + (w + shift) % Wp];
    size_t row = 0;
    for (int b = 0; b < B; ++b)                       // window_partition: (b, wr, wc, i, j)
        for (int wr = 0; wr < nWh; ++wr)
            for (int wc = 0; wc < nWw; ++wc)
                for (int i = 0; i < ws; ++i)
                    for (int j = 0; j < ws; ++j) table[row++] = rolled[((size_t)b * Hp + wr * ws + i) * Wp + wc * ws + j];
    return table;
}
static int check_classic() {
    const int wss[] = {2, 3, 7, 12};
    int ncases = 0;
    for (int H = 1; H <= 30; ++H)
        for (int W = 1; W <= 30; ++W)
            for (int ws : wss)
                for (int shift = 0; shift < ws; ++shift)
                    for (int B = 1; B <= 2; ++B) {
                        if (!wm_map_ok(B, H, W, ws, shift, WM_CLASSIC, (int64_t)B * H * W)) { printf("classic refused H%d W%d ws%d s%d\n", H, W, ws, shift); return -1; }
                        const WmMap m = wm_map(B, H, W, ws, shift);
                        const std::vector<int> table = brute_classic(B, H, W, ws, shift);
                        if (wm_classic_rows(m) != (int64_t)table.size()) { printf("classic rows H%d W%d ws%d s%d\n", H, W, ws, shift); return -1; }
                        int pad = 0;
                        for (int row = 0; row < (int)table.size(); ++row) {
                            int b32 = -1, b64 = -1;
                            const int t32 = wm_row_token<int, WM_CLASSIC>(m, row, b32);
                            const int64_t t64 = wm_row_token<int64_t>(m, (int64_t)row, b64);
                            if (t32 != table[row] || t64 != table[row] || b32 != b64 || (t32 >= 0 && b32 != t32 / (H * W))) {
                                printf("classic row->token B%d H%d W%d ws%d s%d row %d: %d / %lld vs %d\n", B, H, W, ws, shift, row, t32, (long long)t64, table[row]);
                                return -1;
                            }
                            if (t32 < 0) { ++pad; continue; }
                            const int r32 = wm_token_row<int, WM_CLASSIC>(m, t32);
                            const int64_t r64 = wm_token_row<int64_t>(m, t64), rb = wm_token_row<int64_t>(m, b32, (t32 / W) % H, t32 % W);
                            if (r32 != row || r64 != row || rb != row) {
                                printf("classic token->row B%d H%d W%d ws%d s%d tok %d: %d / %lld / %lld vs %d\n", B, H, W, ws, shift, t32, r32, (long long)r64, (long long)rb, row);
                                return -1;
                            }
                        }
                        if (pad != (int)table.size() - B * H * W) { printf("classic padding count H%d W%d ws%d s%d\n", H, W, ws, shift); return -1; }
                        ++ncases;
                    }
    return ncases;
}

// ---- the host validity check against the checks it replaced (as they stood in layernorm.hip, residual.hip, window_shuffle.hip and the
// DGX_EPI_BIAS_RESIDUAL block of gemm_nt.hip; each after its entry point's early return for an empty problem) ----
static bool old_ln(int B, int H, int W, int ws, int shift, int64_t T) {                 // map_args_ok
    if (ws == 0) return true;
    const int a = ws < 0 ? -ws : ws;
    if ((int64_t)B * H * W != T || shift < 0 || shift >= a) return false;
    return ws > 0 || wm_compact_ok(H, W, a, shift);
}
static bool old_residual(int ws, int shift) { return !(shift < 0 || (ws > 0 && shift >= ws)); }
static bool old_shuffle(int ws, int shift) { return !(ws <= 0 || shift < 0 || shift >= ws); }
static bool old_gemm(int H, int W, int ws, int shift) {
    const int aws = ws < 0 ? -ws : ws;
    return !(shift < 0 || (aws > 0 && shift >= aws) || (ws < 0 && !wm_compact_ok(H, W, aws, shift)));
}
static int check_valid() {
    int n = 0;
    const int wss[] = {-12, -7, -2, -1, 0, 1, 2, 7, 12}, dims[] = {1, 2, 5, 6, 7, 13, 30};
    for (int ws : wss)
        for (int shift = -1; shift <= 13; ++shift)
            for (int H : dims)
                for (int W : dims)
                    for (int B = 1; B <= 2; ++B)
                        for (int dT = 0; dT <= 1; ++dT) {
                            const int64_t T = (int64_t)B * H * W + dT;
                            const bool ln = ws == 0 || wm_map_ok(B, H, W, ws, shift, WM_CLASSIC | WM_COMPACT, T);   // as layernorm.hip calls it
                            const bool rs = wm_map_ok(B, H, W, ws, shift, WM_IDENTITY | WM_CLASSIC);
                            const bool sh = wm_map_ok(B, H, W, ws, shift, WM_CLASSIC);
                            const bool ge = wm_map_ok(B, H, W, ws, shift, WM_IDENTITY | WM_CLASSIC | WM_COMPACT);
                            // the residual entry points took ws < 0 unchecked and divided by nWw = 0 in the kernel: refused now
                            const bool rs_want = ws < 0 ? false : old_residual(ws, shift);
                            if (ln != old_ln(B, H, W, ws, shift, T) || rs != rs_want || sh != old_shuffle(ws, shift) || ge != old_gemm(H, W, ws, shift)) {
                                printf("validity B%d H%d W%d ws%d s%d T%lld: ln %d rs %d sh %d ge %d\n", B, H, W, ws, shift, (long long)T, ln, rs, sh, ge);
                                return -1;
                            }
                            ++n;
                        }
    // the cases by name
    struct { int B, H, W, ws, shift, orders; int64_t T; bool ok; } named[] = {
        {2, 10, 13, 7, 3, WM_CLASSIC, -1, true},                   // a classic geometry
        {2, 5, 9, 7, 3, WM_CLASSIC, -1, true},                     // H < ws
        {2, 10, 13, 7, 7, WM_CLASSIC, -1, false},                  // shift == ws
        {2, 10, 13, 7, -1, WM_CLASSIC, -1, false},                 // negative shift
        {2, 10, 13, 0, 0, WM_CLASSIC, -1, false},                  // ws == 0 where only a window order is implemented (window_shuffle)
        {2, 10, 13, 0, 5, WM_IDENTITY | WM_CLASSIC, -1, true},     // identity: any shift >= 0
        {2, 10, 13, 0, -1, WM_IDENTITY | WM_CLASSIC, -1, false},   // identity, negative shift (residual, GEMM epilogue)
        {2, 10, 13, -7, 3, WM_IDENTITY | WM_CLASSIC, -1, false},   // compact where it is not implemented
        {2, 10, 13, -7, 3, WM_CLASSIC | WM_COMPACT, 260, true},    // compact
        {2, 2, 13, -7, 3, WM_CLASSIC | WM_COMPACT, 52, false},     // compact with a wrapping band (H < shift)
        {2, 10, 13, 7, 3, WM_CLASSIC | WM_COMPACT, 261, false},    // B*H*W != T
    };
    for (auto& c : named) {
        if (wm_map_ok(c.B, c.H, c.W, c.ws, c.shift, c.orders, c.T) != c.ok) { printf("named validity case ws%d s%d orders%d\n", c.ws, c.shift, c.orders); return -1; }
        ++n;
    }
    return n;
}

static int classic_src(int B, int H, int W, int ws, int shift, int orow) {
    const int nWh = (H + ws - 1) / ws, nWw = (W + ws - 1) / ws, Hp = nWh * ws, Wp = nWw * ws, N = ws * ws;
    const int n = orow % N;
    int t = orow / N;
    const int wc = t % nWw; t /= nWw;
    const int wr = t % nWh;
    const int b = t / nWh;
    int hh = wr * ws + n / ws + shift, ww = wc * ws + n % ws + shift;
    if (hh >= Hp) hh -= Hp;
    if (ww >= Wp) ww -= Wp;
    (void)B;
    return (hh >= H || ww >= W) ? -1 : (b * H + hh) * W + ww;
}

int main() {
    const int cases[][3] = {{64, 64, 12}, {32, 32, 12}, {56, 56, 12}, {28, 28, 12}, {30, 26, 12}, {13, 25, 12}, {24, 36, 12}, {12, 12, 12},
                            {7, 7, 7}, {10, 9, 7}, {20, 15, 7}, {256, 256, 12}, {6, 18, 12}, {9, 40, 12}, {224, 224, 12}, {112, 96, 12}};
    int ncases = 0;
    for (auto& c : cases)
        for (int sh = 0; sh < 2; ++sh) {
            const int H = c[0], W = c[1], ws = c[2], shift = sh ? ws / 2 : 0, B = 2;
            if (!wm_compact_ok(H, W, ws, shift)) continue;
            const WmGeom g = wm_geom(H, W, ws, shift);
            const int N = ws * ws, Tw = B * g.nWh * g.nWw * N, T = B * H * W;
            int r = 0, p = 0;
            for (int orow = 0; orow < Tw; ++orow) {
                const int tok = classic_src(B, H, W, ws, shift, orow);
                const int n = orow % N, wi = (orow / N) % (g.nWh * g.nWw), b = orow / N / (g.nWh * g.nWw);
                const int wr = wi / g.nWw, wc = wi % g.nWw;
                const WmWindow w = wm_window(g, wr, wc);
                int before;
                const bool real = wm_token_real(g, w, wr, wc, n / ws, n % ws, before);
                if (real != (tok >= 0)) { printf("real? H%d W%d ws%d s%d orow %d\n", H, W, ws, shift, orow); return 1; }
                int mb = -1;
                const WmMap cm = wm_map(B, H, W, -ws, shift);
                if (real) {
                    int bb;
                    if (wm_row_token<int>(cm, r, mb) != tok || wm_row_token<int64_t>(cm, (int64_t)r, mb) != tok || wm_token_row<int>(cm, tok) != r ||
                        wm_token_row<int64_t>(cm, (int64_t)tok) != r) { printf("WmMap compact H%d W%d ws%d s%d row %d\n", H, W, ws, shift, r); return 1; }
                    if (b * H * W + w.base + before != r) { printf("window rank H%d W%d ws%d s%d orow %d: %d vs %d\n", H, W, ws, shift, orow, b * H * W + w.base + before, r); return 1; }
                    if (wm_row_of_token(g, tok / (H * W), (tok / W) % H, tok % W) != r) { printf("row_of_token H%d W%d ws%d s%d tok %d\n", H, W, ws, shift, tok); return 1; }
                    if (wm_token_of_row(g, r, bb) != tok || bb != tok / (H * W)) { printf("token_of_row H%d W%d ws%d s%d row %d\n", H, W, ws, shift, r); return 1; }
                    ++r;
                } else {
                    // padding rows: T + (image, window, token) order among the padding tokens
                    const int P = g.nWh * g.nWw * N - H * W;
                    const int prow = T + b * P + (wi * N - w.base) + (n - before);
                    if (wm_row_token<int>(cm, prow, mb) != -1) { printf("WmMap compact tail H%d W%d ws%d s%d row %d\n", H, W, ws, shift, prow); return 1; }
                    if (prow != T + p) { printf("pad row H%d W%d ws%d s%d orow %d: %d vs %d\n", H, W, ws, shift, orow, prow, T + p); return 1; }
                    ++p;
                }
            }
            if (r != T || r + p != Tw) { printf("counts\n"); return 1; }
            ++ncases;
        }
    const int nclassic = check_classic();
    if (nclassic < 0) return 1;
    const int nvalid = check_valid();
    if (nvalid < 0) return 1;
    printf("ok %d %d %d\n", ncases, nclassic, nvalid);
    return 0;
}
