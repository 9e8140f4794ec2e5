// 'possion' blend of the copy-paste compositor for gfx950: the reference's poisson_edit
// (DG/divergen/data/transforms/possion_blending.py:27-64, called per paste by blend_image, custom_cp_method.py:19-22) as a
// sparse symmetric solve on the device.  The contract is written out in include/divergen_hip.h (dgx_poisson_blend).
//
// The reference factorises an (H*W) x (H*W) matrix per paste.  Only the rows of U = F ∪ frame are not identity rows
// (F: placed alpha > 0; frame: the 1-pixel image border), so the system reduces to |U| unknowns: diagonal 4, -1 between
// neighbouring unknowns, known neighbours moved to the right-hand side.  It is a principal submatrix of the Dirichlet
// Laplacian of the H x W grid: symmetric positive definite, so conjugate gradients apply.  All solver state is fp64.
//   k1 count    : per 1024 pixels, how many lie in U
//   k2 scan     : one workgroup, exclusive scan of the counts -> |U| (device-resident; never read by the host)
//   k3 index    : pixel -> unknown index map, unknown -> pixel list (pixel order: deterministic)
//   k4 setup    : 4-neighbour index table, x0 = T, r0 = b - A x0, partial sums of r0.r0          (per channel)
//   k5 / k6     : one CG iteration = two launches (direction + A p + p.Ap | x, r update + r.r), exactly max_iter times,
//                 max_iter fixed by the host; a channel that has converged makes its workgroups leave at once
//   k7 finish   : clamp, truncate, scatter into the image;  k8: the report record
// Synchronisation inside the solve is the launch boundary and workgroup barriers, nothing else.  Dot products go through
// per-workgroup partial sums that every consumer workgroup adds up in the same order: no atomics, the same bits every run.
#include "poisson_blend.h"

#include <math.h>

#include "dgx_common.h"

constexpr int PB_T = 256, PB_E = 4, PB_BLK = PB_T * PB_E;      // threads per workgroup, items per thread, items per workgroup

struct PbChannel { int32_t done, conv, iters, pad; double resid; };
struct PbHdr { int32_t n, overflow, pad[2]; PbChannel ch[3]; };

struct PbLayout { size_t hdr, cnt, offs, idx, pix, nbr, vec, parts, total; int nsb, nbmax; };
static size_t pb_align(size_t v) { return (v + 255) & ~(size_t)255; }
static PbLayout pb_layout(int H, int W, int64_t nmax) {
    PbLayout L;
    const int64_t HW = (int64_t)H * W;
    L.nsb = (int)((HW + PB_BLK - 1) / PB_BLK);
    L.nbmax = (int)((nmax + PB_BLK - 1) / PB_BLK);
    if (L.nbmax < 1) L.nbmax = 1;
    size_t o = PB_REPORT_BYTES;
    L.hdr = o;   o = pb_align(o + sizeof(PbHdr));
    L.cnt = o;   o = pb_align(o + sizeof(int32_t) * (size_t)L.nsb);
    L.offs = o;  o = pb_align(o + sizeof(int32_t) * (size_t)L.nsb);
    L.idx = o;   o = pb_align(o + sizeof(int32_t) * (size_t)HW);
    L.pix = o;   o = pb_align(o + sizeof(int32_t) * (size_t)nmax);
    L.nbr = o;   o = pb_align(o + sizeof(int32_t) * 4 * (size_t)nmax);
    L.vec = o;   o = pb_align(o + sizeof(double) * 15 * (size_t)nmax);          // 3 channels x (x, r, q, p0, p1)
    L.parts = o; o = pb_align(o + sizeof(double) * 9 * (size_t)L.nbmax);        // 3 channels x (rr0, rr1, pq)
    L.total = o;
    return L;
}

struct PbView {
    PbHdr* hdr;
    int32_t *cnt, *offs, *idx, *pix, *nbr;
    double *vec, *parts;
    int64_t nmax;
    int nsb, nbmax;
    __device__ double* v(int c, int which) const { return vec + ((int64_t)c * 5 + which) * nmax; }      // x r q p0 p1
    __device__ double* part(int c, int which) const { return parts + ((int64_t)c * 3 + which) * nbmax; }  // rr0 rr1 pq
};
static PbView pb_view(void* work, const PbLayout& L, int64_t nmax) {
    char* w = (char*)work;
    PbView v;
    v.hdr = (PbHdr*)(w + L.hdr);
    v.cnt = (int32_t*)(w + L.cnt); v.offs = (int32_t*)(w + L.offs); v.idx = (int32_t*)(w + L.idx);
    v.pix = (int32_t*)(w + L.pix); v.nbr = (int32_t*)(w + L.nbr);
    v.vec = (double*)(w + L.vec); v.parts = (double*)(w + L.parts);
    v.nmax = nmax; v.nsb = L.nsb; v.nbmax = L.nbmax;
    return v;
}

struct PbPatch {                                   // one placed paste: patch pixel (x - dx, y - dy) inside [0, w) x [0, h)
    const uint8_t* px; int h, w, dx, dy;
    __device__ const uint8_t* at(int x, int y) const {
        const int sx = x - dx, sy = y - dy;
        return (sx >= 0 && sy >= 0 && sx < w && sy < h) ? px + 4 * ((int64_t)sy * w + sx) : nullptr;
    }
    __device__ bool mask(int x, int y) const { const uint8_t* p = at(x, y); return p && p[3] > 0; }
    __device__ double src(int x, int y, int c) const { const uint8_t* p = at(x, y); return p ? (double)p[c] : 0.0; }
};
__device__ __forceinline__ PbPatch pb_patch(const uint8_t* rgba, const int32_t* ddesc, PbDesc hd) {
    if (ddesc) { hd.off = ddesc[0]; hd.h = ddesc[1]; hd.w = ddesc[2]; hd.x0 = ddesc[3]; hd.y0 = ddesc[4]; }
    return PbPatch{rgba + hd.off, hd.h, hd.w, hd.x0, hd.y0};
}
__device__ __forceinline__ bool pb_in_u(const PbPatch& P, int x, int y, int H, int W) {
    return x == 0 || y == 0 || x == W - 1 || y == H - 1 || P.mask(x, y);
}

// Sum over the workgroup (PB_T threads), the same value in every thread; the additions always happen in the same order.
__device__ __forceinline__ double pb_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = PB_T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double pb_sum_parts(const double* part, int nb, double* sh) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += PB_T) a += part[i];
    return pb_block_sum(a, sh);
}
// Exclusive scan of one int per thread over the workgroup; *total gets the sum.
__device__ __forceinline__ int pb_block_scan(int v, int* sh, int* total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < PB_T; s <<= 1) {
        const int add = (int)threadIdx.x >= s ? sh[threadIdx.x - s] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const int incl = sh[threadIdx.x];
    *total = sh[PB_T - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(PB_T) void pb_count_kernel(PbView V, int H, int W, const uint8_t* rgba, const int32_t* ddesc, PbDesc hd) {
    __shared__ double sh[PB_T];
    const PbPatch P = pb_patch(rgba, ddesc, hd);
    const int64_t HW = (int64_t)H * W, p0 = (int64_t)blockIdx.x * PB_BLK + (int64_t)threadIdx.x * PB_E;
    int c = 0;
    for (int e = 0; e < PB_E; ++e) {
        const int64_t p = p0 + e;
        if (p < HW) c += pb_in_u(P, (int)(p % W), (int)(p / W), H, W) ? 1 : 0;
    }
    const double s = pb_block_sum((double)c, sh);          // exact: at most 1024
    if (threadIdx.x == 0) V.cnt[blockIdx.x] = (int)s;
}

__global__ __launch_bounds__(PB_T) void pb_scan_kernel(PbView V) {
    __shared__ int sh[PB_T];
    int carry = 0;
    for (int b0 = 0; b0 < V.nsb; b0 += PB_T) {
        const int b = b0 + threadIdx.x;
        const int v = b < V.nsb ? V.cnt[b] : 0;
        int total;
        const int ex = pb_block_scan(v, sh, &total);
        if (b < V.nsb) V.offs[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        const bool over = (int64_t)carry > V.nmax;          // cannot happen when the host sized the workspace from the paste
        V.hdr->n = over ? 0 : carry;
        V.hdr->overflow = over ? 1 : 0;
    }
    if (threadIdx.x < 3) V.hdr->ch[threadIdx.x] = PbChannel{0, 0, 0, 0, -1.0};
}

__global__ __launch_bounds__(PB_T) void pb_index_kernel(PbView V, int H, int W, const uint8_t* rgba, const int32_t* ddesc, PbDesc hd) {
    __shared__ int sh[PB_T];
    const PbPatch P = pb_patch(rgba, ddesc, hd);
    const bool live = V.hdr->overflow == 0;                 // uniform over the grid
    const int64_t HW = (int64_t)H * W, p0 = (int64_t)blockIdx.x * PB_BLK + (int64_t)threadIdx.x * PB_E;
    bool in[PB_E];
    int c = 0;
    for (int e = 0; e < PB_E; ++e) {
        const int64_t p = p0 + e;
        in[e] = p < HW && pb_in_u(P, (int)(p % W), (int)(p / W), H, W);
        c += in[e] ? 1 : 0;
    }
    int total;
    int rank = V.offs[blockIdx.x] + pb_block_scan(c, sh, &total);
    for (int e = 0; e < PB_E; ++e) {
        const int64_t p = p0 + e;
        if (p >= HW) break;
        if (in[e] && live && rank < V.nmax) {
            V.idx[p] = rank;
            V.pix[rank] = (int32_t)p;
            ++rank;
        } else {
            V.idx[p] = -1;
        }
    }
}

// blockIdx.y = channel.  b (reference :54-55): 4 S_k - sum S_j over the neighbours inside the image where mask, T_k elsewhere; the known
// neighbours' +T_j joins it.  x0 = T on all of U, so r0 = b + sum T_j (all neighbours inside the image) - 4 T_k.
__global__ __launch_bounds__(PB_T) void pb_setup_kernel(PbView V, const uint8_t* image, int H, int W, const uint8_t* rgba,
                                                        const int32_t* ddesc, PbDesc hd) {
    __shared__ double sh[PB_T];
    const int n = V.hdr->n, nb = (n + PB_BLK - 1) / PB_BLK, c = blockIdx.y;
    if ((int)blockIdx.x >= nb) return;
    const PbPatch P = pb_patch(rgba, ddesc, hd);
    const uint8_t* T = image + (int64_t)c * H * W;
    double* x = V.v(c, 0);
    double* r = V.v(c, 1);
    double dot = 0.0;
    for (int e = 0; e < PB_E; ++e) {
        const int i = blockIdx.x * PB_BLK + e * PB_T + threadIdx.x;
        if (i >= n) continue;
        const int p = V.pix[i], y = p / W, xx = p - y * W;
        const bool m = P.mask(xx, y);
        const int nx[4] = {xx - 1, xx + 1, xx, xx}, ny[4] = {y, y, y - 1, y + 1};
        double sumS = 0.0, sumT = 0.0;
        for (int d = 0; d < 4; ++d) {
            const bool ex = nx[d] >= 0 && nx[d] < W && ny[d] >= 0 && ny[d] < H;
            const int q = ny[d] * W + nx[d];
            if (ex) {
                sumT += (double)T[q];
                if (m) sumS += P.src(nx[d], ny[d], c);
            }
            if (c == 0) V.nbr[(int64_t)d * V.nmax + i] = ex ? V.idx[q] : -1;
        }
        const double t = (double)T[p];
        const double b = m ? 4.0 * P.src(xx, y, c) - sumS : t;
        const double r0 = b + sumT - 4.0 * t;
        x[i] = t;
        r[i] = r0;
        dot += r0 * r0;
    }
    const double s = pb_block_sum(dot, sh);
    if (threadIdx.x == 0) V.part(c, 0)[blockIdx.x] = s;
}

// First half of iteration `it`: stop test on |r|, p = r + beta p_old (p ping-pongs between two buffers, so a neighbour's new
// direction is formed from r and p_old and no workgroup waits for another), q = A p, partial sums of p.q.
__global__ __launch_bounds__(PB_T) void pb_cg_dir_kernel(PbView V, int it, double tol) {
    __shared__ double sh[PB_T];
    __shared__ int s_done;
    const int n = V.hdr->n, nb = (n + PB_BLK - 1) / PB_BLK, c = blockIdx.y;
    if ((int)blockIdx.x >= nb) return;
    if (threadIdx.x == 0) s_done = V.hdr->ch[c].done;       // read once per workgroup: the decision below must be uniform
    __syncthreads();
    if (s_done) return;
    const double rr = pb_sum_parts(V.part(c, it & 1), nb, sh);
    if (sqrt(rr) <= tol) {                                   // every workgroup of the channel sees the same sum
        if (blockIdx.x == 0 && threadIdx.x == 0) V.hdr->ch[c] = PbChannel{1, 1, it, 0, sqrt(rr)};
        return;
    }
    const double beta = it ? rr / pb_sum_parts(V.part(c, (it & 1) ^ 1), nb, sh) : 0.0;
    const double* r = V.v(c, 1);
    double* q = V.v(c, 2);
    const double* po = V.v(c, 3 + ((it & 1) ^ 1));
    double* pn = V.v(c, 3 + (it & 1));
    double dot = 0.0;
    for (int e = 0; e < PB_E; ++e) {
        const int i = blockIdx.x * PB_BLK + e * PB_T + threadIdx.x;
        if (i >= n) continue;
        const double pi = it ? r[i] + beta * po[i] : r[i];
        double acc = 4.0 * pi;
        for (int d = 0; d < 4; ++d) {
            const int j = V.nbr[(int64_t)d * V.nmax + i];
            if (j >= 0) acc -= it ? r[j] + beta * po[j] : r[j];
        }
        pn[i] = pi;
        q[i] = acc;
        dot += pi * acc;
    }
    const double s = pb_block_sum(dot, sh);
    if (threadIdx.x == 0) V.part(c, 2)[blockIdx.x] = s;
}

// Second half: alpha = r.r / p.q, x += alpha p, r -= alpha q, partial sums of the new r.r.
__global__ __launch_bounds__(PB_T) void pb_cg_step_kernel(PbView V, int it) {
    __shared__ double sh[PB_T];
    __shared__ int s_done;
    const int n = V.hdr->n, nb = (n + PB_BLK - 1) / PB_BLK, c = blockIdx.y;
    if ((int)blockIdx.x >= nb) return;
    if (threadIdx.x == 0) s_done = V.hdr->ch[c].done;
    __syncthreads();
    if (s_done) return;
    const double rr = pb_sum_parts(V.part(c, it & 1), nb, sh);
    const double pq = pb_sum_parts(V.part(c, 2), nb, sh);
    const double alpha = rr / pq;                            // pq > 0: A is positive definite and p != 0 (|r| > tol > 0)
    double* x = V.v(c, 0);
    double* r = V.v(c, 1);
    const double* q = V.v(c, 2);
    const double* p = V.v(c, 3 + (it & 1));
    double dot = 0.0;
    for (int e = 0; e < PB_E; ++e) {
        const int i = blockIdx.x * PB_BLK + e * PB_T + threadIdx.x;
        if (i >= n) continue;
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        r[i] = ri;
        dot += ri * ri;
    }
    const double s = pb_block_sum(dot, sh);
    if (threadIdx.x == 0) V.part(c, (it + 1) & 1)[blockIdx.x] = s;
}

// Clamp to [0, 255], truncate, scatter.  A channel that ran into the cap gets its residual measured here and keeps conv = 0
// unless that residual passes after all; the image takes its last iterate either way.
__global__ __launch_bounds__(PB_T) void pb_finish_kernel(PbView V, uint8_t* image, int H, int W, int max_iter, double tol) {
    __shared__ double sh[PB_T];
    __shared__ int s_done;
    const int n = V.hdr->n, nb = (n + PB_BLK - 1) / PB_BLK, c = blockIdx.y;
    if ((int)blockIdx.x >= nb) return;
    if (threadIdx.x == 0) s_done = V.hdr->ch[c].done;
    __syncthreads();
    if (!s_done) {
        const double rr = pb_sum_parts(V.part(c, max_iter & 1), nb, sh);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            V.hdr->ch[c].conv = sqrt(rr) <= tol ? 1 : 0;
            V.hdr->ch[c].iters = max_iter;
            V.hdr->ch[c].resid = sqrt(rr);
        }
    }
    const double* x = V.v(c, 0);
    uint8_t* out = image + (int64_t)c * H * W;
    for (int e = 0; e < PB_E; ++e) {
        const int i = blockIdx.x * PB_BLK + e * PB_T + threadIdx.x;
        if (i >= n) continue;
        const double v = x[i];
        out[V.pix[i]] = (uint8_t)(int)(!(v > 0.0) ? 0.0 : (v > 255.0 ? 255.0 : v));
    }
}

__global__ void pb_report_kernel(PbView V, double* rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int iters = 0, conv = V.hdr->overflow ? 0 : 1;
    double resid = -1.0;
    for (int c = 0; c < 3; ++c) {
        iters = max(iters, V.hdr->ch[c].iters);
        conv = conv && V.hdr->ch[c].conv;
        resid = fmax(resid, V.hdr->ch[c].resid);
    }
    rec[0] = (double)iters;
    rec[1] = resid;
    rec[2] = (double)conv;
    rec[3] = (double)V.hdr->n;
}

__global__ void pb_clear_kernel(double* rec, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rec[i] = 0.0;
}

// ||x - x*||_inf <= ||x - x*||_2 <= ||r||_2 / lambda_min(A), and lambda_min(A) >= lambda_min of the H x W Dirichlet Laplacian
// (A is a principal submatrix of it) = 4 sin^2(pi / (2 (H + 1))) + 4 sin^2(pi / (2 (W + 1))).  Stopping at ||r||_2 <= a quarter of
// DELTA = 1e-3 times that bound keeps the solution within DELTA of the exact one with room for the drift of the recursive residual.
static double pb_tolerance(int H, int W) {
    const double pi = 3.14159265358979323846;
    const double sh = sin(pi / (2.0 * (H + 1))), sw = sin(pi / (2.0 * (W + 1)));
    return 0.25e-3 * (4.0 * sh * sh + 4.0 * sw * sw);
}

extern "C" int64_t dgx_poisson_frame_unknowns(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (H < 3 || W < 3) ? (int64_t)H * W : 2 * (int64_t)H + 2 * (int64_t)W - 4;
}

extern "C" int64_t dgx_poisson_work_bytes(int H, int W, int64_t max_unknowns) {
    if (H <= 0 || W <= 0 || max_unknowns < 0) return 0;
    const int64_t HW = (int64_t)H * W;
    return (int64_t)pb_layout(H, W, max_unknowns < HW ? max_unknowns : HW).total;
}

// CG on an SPD matrix reduces the energy norm of the error by 2 ((sqrt(k) - 1) / (sqrt(k) + 1))^i, k the condition number.  Here
// lambda_max < 8, and among all pixel sets of a given size the disc has the smallest lambda_min (Faber-Krahn), about 18.2 / |F|
// for the footprint F (the frame's rows are strictly dominant and do not lower it): sqrt(k) <= 0.66 sqrt|F|.  Going from
// |r0| <= 4 * 255 sqrt|U| to the stopping tolerance is a reduction by at most e^-38: i <= 0.33 sqrt|F| * 38.5 = 12.7 sqrt|F|.
extern "C" int dgx_poisson_max_iter(int H, int W, int64_t max_unknowns) {
    const int64_t HW = (int64_t)H * W;
    if (max_unknowns > HW) max_unknowns = HW;
    int64_t f = max_unknowns - dgx_poisson_frame_unknowns(H, W);
    if (f < 0) f = 0;
    return 100 + 16 * (int)ceil(sqrt((double)f));
}

int64_t pb_capacity(int H, int W, const void* work, size_t work_bytes) {
    if (!work || ((uintptr_t)work & 15)) return -1;
    const int64_t HW = (int64_t)H * W, fr = dgx_poisson_frame_unknowns(H, W);
    if (pb_layout(H, W, fr).total > work_bytes) return -1;
    int64_t lo = fr, hi = HW;                                // the largest n in [fr, HW] whose layout fits
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (pb_layout(H, W, mid).total <= work_bytes) lo = mid; else hi = mid - 1;
    }
    return lo;
}

int pb_clear_report(void* work, hipStream_t st) {
    const int n = PB_REPORT_RECORDS * PB_REPORT_DOUBLES;
    hipLaunchKernelGGL(pb_clear_kernel, dim3(1), dim3(n), 0, st, (double*)work, n);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

int pb_enqueue(uint8_t* image, int H, int W, const uint8_t* src_rgba, const int32_t* ddesc, PbDesc hd, void* work, int64_t nmax,
               int max_iter, int record, hipStream_t st) {
    const PbLayout L = pb_layout(H, W, nmax);
    const PbView V = pb_view(work, L, nmax);
    if (max_iter < 0) max_iter = dgx_poisson_max_iter(H, W, nmax);
    const double tol = pb_tolerance(H, W);
    hipLaunchKernelGGL(pb_count_kernel, dim3(L.nsb), dim3(PB_T), 0, st, V, H, W, src_rgba, ddesc, hd);
    hipLaunchKernelGGL(pb_scan_kernel, dim3(1), dim3(PB_T), 0, st, V);
    hipLaunchKernelGGL(pb_index_kernel, dim3(L.nsb), dim3(PB_T), 0, st, V, H, W, src_rgba, ddesc, hd);
    const dim3 grid(L.nbmax, 3);
    hipLaunchKernelGGL(pb_setup_kernel, grid, dim3(PB_T), 0, st, V, (const uint8_t*)image, H, W, src_rgba, ddesc, hd);
    for (int it = 0; it < max_iter; ++it) {                  // a fixed number of launches: nothing is read back
        hipLaunchKernelGGL(pb_cg_dir_kernel, grid, dim3(PB_T), 0, st, V, it, tol);
        hipLaunchKernelGGL(pb_cg_step_kernel, grid, dim3(PB_T), 0, st, V, it);
    }
    hipLaunchKernelGGL(pb_finish_kernel, grid, dim3(PB_T), 0, st, V, image, H, W, max_iter, tol);
    hipLaunchKernelGGL(pb_report_kernel, dim3(1), dim3(1), 0, st, V, (double*)work + (int64_t)record * PB_REPORT_DOUBLES);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_poisson_blend(uint8_t* image, const uint8_t* src_rgba, const int32_t* desc_host, int H, int W, void* work,
                                 size_t work_bytes, int max_iter, void* stream) {
    if (!image || !src_rgba || !desc_host || H <= 0 || W <= 0) return DGX_ERR_BAD_ARG;
    const PbDesc hd = {desc_host[0], desc_host[1], desc_host[2], desc_host[3], desc_host[4]};
    if (hd.off < 0 || hd.h < 0 || hd.w < 0) return DGX_ERR_BAD_ARG;
    if (H < 3 || W < 3) return DGX_ERR_UNSUPPORTED;
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    // |U| <= pixels of the paste's rectangle inside the image + the frame
    const int64_t y1 = (int64_t)hd.y0 + hd.h, x1 = (int64_t)hd.x0 + hd.w;
    const int64_t ch = (y1 < H ? y1 : H) - (hd.y0 > 0 ? hd.y0 : 0), cw = (x1 < W ? x1 : W) - (hd.x0 > 0 ? hd.x0 : 0);
    int64_t need = dgx_poisson_frame_unknowns(H, W) + (ch > 0 && cw > 0 ? ch * cw : 0);
    if (need > (int64_t)H * W) need = (int64_t)H * W;
    const int64_t cap = pb_capacity(H, W, work, work_bytes);
    if (cap < need || max_iter > dgx_poisson_max_iter(H, W, (int64_t)H * W)) return DGX_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int rc = pb_clear_report(work, st);
    if (rc != DGX_OK) return rc;
    return pb_enqueue(image, H, W, src_rgba, nullptr, hd, work, need, max_iter, 0, st);
}
