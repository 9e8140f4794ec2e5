// Pillow-exact 8-bit bilinear resize (INPUT.DEVICE_RESIZE) for gfx950: a table of J independent jobs in ONE launch.  A job resamples one
// interleaved source (3 or 4 channels) exactly as Pillow's Resample.c does for 8 bits per channel -- horizontal pass first, ROUNDED TO
// BYTES, then the vertical pass on those bytes -- but only for a crop window of the scaled image, optionally mirrored, and writes the
// window planar (C, ch, cw) into `image` or as interleaved RGBA (ch, cw, 4) into `flat`.
//   one pass:  out = clamp((2^21 + sum_t src[xmin + t] * k[t]) >> 22, 0, 255), int32, arithmetic shift, every channel alike
//   RGBA with a size change ('premultiply' flag):  c' = ((c * a + 128 >> 8) + c * a + 128) >> 8 on load, and on store
//       c = c' when a is 0 or 255, else min(255 * c' / a, 255)  (Pillow's RGBA -> RGBa -> RGBA round trip)
// The coefficient tables come from the host (data/resize_tables.py, float64 like Pillow's doubles) and hold ONLY the window's rows and
// columns: per axis and job `bounds` (L, 2) = (xmin, n) followed by `k` (L, ksize), int32.  An axis whose size does not change carries
// the identity taps (n = 1, k = 2^22), which reproduce the byte exactly: (2^21 + s * 2^22) >> 22 == s.  No floating point here.
// A workgroup of 4 waves owns a tile of 64 x 16 output pixels; a lane owns 4 consecutive columns of one row.  The source rows the tile's
// vertical taps span are taken RS_CHUNK at a time: the workgroup runs the horizontal pass for the tile's 64 columns of those rows into
// LDS (one packed dword per pixel, 8 KB), then every lane adds the chunk's share of its vertical taps into its 16 int32 accumulators --
// a 10x (or any) downscale only takes more chunks, never more LDS.  The planar store packs a lane's 4 columns of one channel into one
// dword (16 lanes = 64 contiguous bytes of a row) where the address is 4-byte aligned, the interleaved store is one dword per pixel.
// No atomics; every byte of every job's window is written exactly once and nothing else.  Every number the kernel indexes with has
// been checked on the HOST copy of the tables before the launch (rs_validate); nothing is launched for a table that fails.
// Bytes that must move: the window's source footprint in, C * ch * cw (or 4 * ch * cw) out, the tables in.
#include "dgx_common.h"

#define RS_TILE_W 64
#define RS_TILE_H 16
#define RS_CHUNK 32         // source rows per horizontal-pass chunk: RS_CHUNK * RS_TILE_W dwords of LDS
#define RS_JOB_WORDS 13
#define RS_FLIP 1
#define RS_INTERLEAVED 2
#define RS_PREMUL 4
#define RS_HALF (1u << 21)
enum { RS_SRC_OFF, RS_SRC_H, RS_SRC_W, RS_C, RS_CH, RS_CW, RS_FLAGS, RS_DST_OFF, RS_H_OFF, RS_H_KS, RS_V_OFF, RS_V_KS, RS_TILE0 };

// The empty asm hides the clamped value from the instruction selector: it otherwise fuses shift, clamp and the packing of two channels
// into v_ashr_pk_u8_i32, whose 16-bit result it then ORs with the other channels WITHOUT clearing the upper half of the register -- the
// hardware leaves the register's old upper bits there (measured: the coefficient 2^22 a lane had just loaded came out as bit 6 of the
// third channel).
__device__ __forceinline__ uint32_t rs_clip(uint32_t acc) {
    int v = min(max((int)acc >> 22, 0), 255);
    asm volatile("" : "+v"(v));
    return (uint32_t)v;
}

__device__ __forceinline__ uint32_t rs_pack(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
    return rs_clip(a0) | (rs_clip(a1) << 8) | (rs_clip(a2) << 16) | (rs_clip(a3) << 24);
}

__device__ __forceinline__ uint32_t rs_premultiply(uint32_t p) {
    const uint32_t a = p >> 24;
    uint32_t out = p & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t t = ((p >> (8 * c)) & 255u) * a + 128u;
        out |= (((t >> 8) + t) >> 8) << (8 * c);
    }
    return out;
}

__device__ __forceinline__ uint32_t rs_unpremultiply(uint32_t p) {
    const uint32_t a = p >> 24;
    if (a == 0u || a == 255u) return p;
    uint32_t out = p & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) out |= min(255u * ((p >> (8 * c)) & 255u) / a, 255u) << (8 * c);
    return out;
}

__global__ __launch_bounds__(256) void rs_resize_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ jobs, int J,
                                                        const int32_t* __restrict__ tab, uint8_t* __restrict__ image,
                                                        uint8_t* __restrict__ flat) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[RS_CHUNK * RS_TILE_W];
    const int tid = threadIdx.x, b = (int)blockIdx.x;
    int lo = 0, hi = J - 1;                                 // the job of this workgroup: the last one whose first tile is <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid * RS_JOB_WORDS + RS_TILE0] <= b) lo = mid; else hi = mid - 1;
    }
    const int32_t* jb = jobs + lo * RS_JOB_WORDS;
    const int src_w = jb[RS_SRC_W], C = jb[RS_C], ch = jb[RS_CH], cw = jb[RS_CW], flags = jb[RS_FLAGS];
    const int hks = jb[RS_H_KS], vks = jb[RS_V_KS];
    const int32_t* hb = tab + jb[RS_H_OFF];
    const int32_t* hk = hb + 2 * (int64_t)cw;
    const int32_t* vb = tab + jb[RS_V_OFF];
    const int32_t* vk = vb + 2 * (int64_t)ch;
    const uint8_t* sbase = src + jb[RS_SRC_OFF];
    const bool premul = (flags & RS_PREMUL) != 0;
    const int tiles_x = (cw + RS_TILE_W - 1) / RS_TILE_W;
    const int t = b - jb[RS_TILE0];
    const int x0 = (t % tiles_x) * RS_TILE_W, y0 = (t / tiles_x) * RS_TILE_H;

    const int r = y0 + (tid >> 4), lx = (tid & 15) * 4, cx = x0 + lx;      // this lane's output row and first column in the window
    const bool row_ok = r < ch;
    const int vmin = row_ok ? vb[2 * r] : 0, vn = row_ok ? vb[2 * r + 1] : 0;
    int y_lo = INT32_MAX, y_hi = 0;                         // the source rows the tile's vertical taps span (workgroup-uniform)
    for (int i = 0; i < RS_TILE_H && y0 + i < ch; ++i) {
        const int s = vb[2 * (y0 + i)], n = vb[2 * (y0 + i) + 1];
        if (n > 0) {
            y_lo = min(y_lo, s);
            y_hi = max(y_hi, s + n);
        }
    }
    uint32_t acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[q][c] = RS_HALF;

    for (int yc = y_lo; yc < y_hi; yc += RS_CHUNK) {        // workgroup-uniform trip count: every wave meets the barriers
        const int nr = min(RS_CHUNK, y_hi - yc);
        __syncthreads();                                    // the previous chunk has been read
        for (int i = tid; i < nr * RS_TILE_W; i += 256) {   // horizontal pass: a wave = one source row, 64 adjacent output columns
            const int x = x0 + (i & (RS_TILE_W - 1));
            if (x >= cw) continue;
            const int xmin = hb[2 * x], n = hb[2 * x + 1];
            const int32_t* k = hk + (int64_t)x * hks;
            const uint8_t* sp = sbase + ((int64_t)(yc + (i >> 6)) * src_w + xmin) * C;
            uint32_t a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF, a3 = RS_HALF;
            if (C == 4) {
                for (int s = 0; s < n; ++s) {
                    uint32_t p = reinterpret_cast<const uint32_t*>(sp)[s];      // 4-byte aligned: the host checked base and offset
                    if (premul) p = rs_premultiply(p);
                    const uint32_t kk = (uint32_t)k[s];
                    a0 += (p & 255u) * kk;
                    a1 += ((p >> 8) & 255u) * kk;
                    a2 += ((p >> 16) & 255u) * kk;
                    a3 += (p >> 24) * kk;
                }
            } else {
                for (int s = 0; s < n; ++s) {
                    const uint32_t kk = (uint32_t)k[s];
                    a0 += sp[3 * s] * kk;
                    a1 += sp[3 * s + 1] * kk;
                    a2 += sp[3 * s + 2] * kk;
                }
            }
            rows[i] = rs_pack(a0, a1, a2, a3);
        }
        __syncthreads();
        if (row_ok) {                                       // vertical pass: this chunk's share of the lane's taps
            const int s0 = max(vmin, yc), s1 = min(vmin + vn, yc + nr);
            for (int y = s0; y < s1; ++y) {
                const uint32_t kk = (uint32_t)vk[(int64_t)r * vks + (y - vmin)];
                const u32x4 p4 = *reinterpret_cast<const u32x4*>(&rows[(y - yc) * RS_TILE_W + lx]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[q][c] += ((p4[q] >> (8 * c)) & 255u) * kk;
            }
        }
    }

    const int ncols = min(4, cw - cx);
    if (!row_ok || ncols <= 0) return;
    uint32_t px[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        px[q] = rs_pack(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
        if (premul) px[q] = rs_unpremultiply(px[q]);
    }
    const bool flip = (flags & RS_FLIP) != 0;
    if (flags & RS_INTERLEAVED) {
        uint8_t* row = flat + jb[RS_DST_OFF] + (int64_t)r * cw * 4;
        const bool vec = (reinterpret_cast<uintptr_t>(row) & 3u) == 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q >= ncols) break;
            uint8_t* d = row + (int64_t)(flip ? cw - 1 - (cx + q) : cx + q) * 4;
            if (vec) {
                *reinterpret_cast<uint32_t*>(d) = px[q];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) d[c] = (uint8_t)(px[q] >> (8 * c));
            }
        }
        return;
    }
    for (int c = 0; c < C; ++c) {
        uint8_t* row = image + jb[RS_DST_OFF] + ((int64_t)c * ch + r) * cw;
        const uint32_t b0 = (px[0] >> (8 * c)) & 255u, b1 = (px[1] >> (8 * c)) & 255u, b2 = (px[2] >> (8 * c)) & 255u,
                       b3 = (px[3] >> (8 * c)) & 255u;
        const int xd = flip ? cw - 1 - (cx + 3) : cx;          // with 4 columns: the lowest of their addresses
        if (ncols == 4 && (reinterpret_cast<uintptr_t>(row + xd) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(row + xd) = flip ? (b3 | (b2 << 8) | (b1 << 16) | (b0 << 24)) : (b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
        } else {
            const uint32_t bq[4] = {b0, b1, b2, b3};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < ncols) row[flip ? cw - 1 - (cx + q) : cx + q] = (uint8_t)bq[q];
        }
    }
}

// One axis table of a job on the host copy: `len` rows of (xmin, n) then len * ks coefficients, inside tab; every row inside the source.
static bool rs_axis_ok(const int32_t* tab, int64_t tab_words, int64_t off, int len, int ks, int in_size) {
    if (ks < 1 || off < 0 || off + (int64_t)len * (2 + (int64_t)ks) > tab_words) return false;
    const int32_t* bnd = tab + off;
    for (int i = 0; i < len; ++i) {
        const int64_t xmin = bnd[2 * i], n = bnd[2 * i + 1];
        if (xmin < 0 || n < 0 || n > ks || xmin + n > in_size) return false;
    }
    return true;
}

// The whole job table on its host copy; *tiles = number of workgroups.  false: something would index outside its buffer.
static bool rs_validate(const int32_t* jobs, int J, const int32_t* tab, int64_t tab_words, int64_t src_bytes, int64_t image_bytes,
                        int64_t flat_bytes, bool src_aligned, int64_t* tiles) {
    int64_t total = 0;
    for (int j = 0; j < J; ++j) {
        const int32_t* jb = jobs + (int64_t)j * RS_JOB_WORDS;
        const int64_t sh = jb[RS_SRC_H], sw = jb[RS_SRC_W], C = jb[RS_C], ch = jb[RS_CH], cw = jb[RS_CW];
        const int flags = jb[RS_FLAGS];
        if (sh < 1 || sw < 1 || ch < 1 || cw < 1 || (C != 3 && C != 4) || flags < 0 || flags > 7) return false;
        if ((flags & (RS_INTERLEAVED | RS_PREMUL)) && C != 4) return false;
        if (jb[RS_SRC_OFF] < 0 || jb[RS_SRC_OFF] + sh * sw * C > src_bytes) return false;
        if (C == 4 && (!src_aligned || (jb[RS_SRC_OFF] & 3))) return false;        // the kernel loads RGBA pixels as dwords
        const int64_t out_bytes = (flags & RS_INTERLEAVED) ? 4 * ch * cw : C * ch * cw;
        if (jb[RS_DST_OFF] < 0 || jb[RS_DST_OFF] + out_bytes > ((flags & RS_INTERLEAVED) ? flat_bytes : image_bytes)) return false;
        if (!rs_axis_ok(tab, tab_words, jb[RS_H_OFF], (int)cw, jb[RS_H_KS], (int)sw)) return false;
        if (!rs_axis_ok(tab, tab_words, jb[RS_V_OFF], (int)ch, jb[RS_V_KS], (int)sh)) return false;
        if (jb[RS_TILE0] != total) return false;
        total += ((cw + RS_TILE_W - 1) / RS_TILE_W) * ((ch + RS_TILE_H - 1) / RS_TILE_H);
        if (total >= ((int64_t)1 << 31)) return false;
    }
    *tiles = total;
    return true;
}

extern "C" int dgx_resize_bilinear_u8(const uint8_t* src, int64_t src_bytes, const int32_t* jobs, const int32_t* tab,
                                      const int32_t* host_jobs, const int32_t* host_tab, int J, int64_t tab_words, uint8_t* image,
                                      int64_t image_bytes, uint8_t* flat, int64_t flat_bytes, void* stream) {
    if (J < 0 || src_bytes < 0 || tab_words < 0 || image_bytes < 0 || flat_bytes < 0) return DGX_ERR_BAD_ARG;
    if (J == 0) return DGX_OK;
    if (!src || !jobs || !tab || !host_jobs || !host_tab || (image_bytes > 0 && !image) || (flat_bytes > 0 && !flat)) return DGX_ERR_BAD_ARG;
    if (src_bytes >= ((int64_t)1 << 31) || tab_words >= ((int64_t)1 << 31) || image_bytes >= ((int64_t)1 << 31) ||
        flat_bytes >= ((int64_t)1 << 31))
        return DGX_ERR_UNSUPPORTED;                        // offsets are int32
    int64_t tiles = 0;
    if (!rs_validate(host_jobs, J, host_tab, tab_words, src_bytes, image_bytes, flat_bytes, (reinterpret_cast<uintptr_t>(src) & 3u) == 0,
                     &tiles))
        return DGX_ERR_BAD_ARG;
    hipLaunchKernelGGL(rs_resize_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, src, jobs, J, tab, image, flat);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
