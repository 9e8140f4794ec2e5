// Ground-truth polygon fill (INPUT.DEVICE_RASTER) for gfx950: the (N, H, W) byte masks of one sample from the sorted crossing lists of its
// polygons, byte for byte divergen_amd/data/build.py:polygons_to_bitmask (pycocotools' rleFrPoly + rleMerge, decoded).
//   pixel (y, x) of ONE polygon = parity of the number of its crossings at column-major flat positions <= x * H + y (inclusive prefix, in
//   flat order: parity carries from the bottom of a column into the top of the next, and an odd total leaves the rest of the canvas set);
//   an instance = OR of its polygons.
// One launch per sample.  A workgroup of 4 waves owns a tile of 256 columns x 64 rows of one instance's plane; a wave owns 16 of those
// rows; a lane owns 4 consecutive columns, i.e. one dword of each row: a wave-instruction stores 256 contiguous bytes of a row.  The
// workgroup first copies the polygon's list into LDS with one coalesced pass (up to 4096 crossings; a longer list stays in global
// memory): the searches below are chains of dependent loads, a dozen deep, and from global memory their latency WAS the kernel's time.
// Per polygon and column the lane finds its carry-in with ONE binary search of x * H + y0 in the list and then walks the handful
// of crossings of that column down its 16 rows.  A polygon is confined to the columns [c0, c1] of its first and last crossing: a wave
// left of c0 skips it, a wave right of c1 takes the parity of the whole list, neither searches.  Every byte of the tile is written
// (zeros where nothing is set): the output buffer need not be cleared.  Integer arithmetic only, no atomics: the result is
// a pure function of the inputs.  The crossing positions are only ever COMPARED, never used as addresses.
// Bytes that must move: N * H * W written + 4 * len(pos) read.
#include "dgx_common.h"

#define PR_ROWS 16      // rows per wave
#define PR_COLS 4       // columns per lane: one dword of a row
#define PR_WAVES 4      // waves per workgroup, stacked in y
#define PR_TILE_W (64 * PR_COLS)
#define PR_TILE_H (PR_WAVES * PR_ROWS)
#define PR_LDS_MAX 4096 // crossings of one polygon staged in LDS (16 KB); a longer list is searched in global memory

// number of entries of p[0 .. n) that are < t (p ascending)
__device__ __forceinline__ int pr_count_below(const int32_t* __restrict__ p, int n, int32_t t) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One polygon (its n crossings at pp, global memory or the workgroup's LDS copy) into the lane's 16 rows x 4 columns
__device__ __forceinline__ void pr_polygon(const int32_t* pp, int n, int H, int W, int x0, int y0, int ny, int xw0, int xw1,
                                           uint32_t (&acc)[PR_ROWS]) {
    const int c0 = pp[0] / H, c1 = pp[n - 1] / H;
    const uint32_t tail = (uint32_t)(n & 1);               // an odd list: everything after its last crossing is set
    if (xw1 < c0) return;                                  // workgroup-uniform
    if (xw0 > c1) {                                        // workgroup-uniform
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) acc[r] |= tail * 0x01010101u;
        return;
    }
#pragma unroll
    for (int c = 0; c < PR_COLS; ++c) {
        const int x = x0 + c;
        if (x >= W || x < c0) continue;
        if (x > c1) {
#pragma unroll
            for (int r = 0; r < PR_ROWS; ++r) acc[r] |= tail << (8 * c);
            continue;
        }
        int32_t t = x * H + y0;                            // < H * W < 2^31
        int i = pr_count_below(pp, n, t);
        int32_t nxt = i < n ? pp[i] : INT32_MAX;
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) {
            if (r < ny) {
                while (nxt <= t) {                         // the crossings at this pixel (t < INT32_MAX ends it)
                    ++i;
                    nxt = i < n ? pp[i] : INT32_MAX;
                }
                acc[r] |= (uint32_t)(i & 1) << (8 * c);
                ++t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void pr_fill_kernel(const int32_t* __restrict__ pos, const int64_t* __restrict__ poly_off,
                                                      const int64_t* __restrict__ inst_off, int H, int W, int tiles_x, int tiles_y,
                                                      int vec, uint8_t* __restrict__ masks) {
    __shared__ int32_t staged[PR_LDS_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t b = blockIdx.x;
    const int tx = (int)(b % tiles_x);
    b /= tiles_x;
    const int ty = (int)(b % tiles_y);
    const int64_t inst = b / tiles_y;
    const int y0 = (ty * PR_WAVES + wave) * PR_ROWS;
    const int ny = max(0, min(PR_ROWS, H - y0));           // 0: a wave below the canvas only helps to stage (it meets every barrier)
    const int x0 = tx * PR_TILE_W + lane * PR_COLS;
    const int xw0 = tx * PR_TILE_W, xw1 = min(W, xw0 + PR_TILE_W) - 1;      // the workgroup's columns
    uint32_t acc[PR_ROWS];
#pragma unroll
    for (int r = 0; r < PR_ROWS; ++r) acc[r] = 0u;

    const int64_t p_end = inst_off[inst + 1];
    for (int64_t p = inst_off[inst]; p < p_end; ++p) {     // workgroup-uniform trip count and branches: the barriers are met by all
        const int64_t s = poly_off[p];
        const int n = (int)(poly_off[p + 1] - s);
        if (n <= 0) continue;
        if (n <= PR_LDS_MAX) {
            __syncthreads();                               // the previous polygon has been read
            for (int k = threadIdx.x; k < n; k += 64 * PR_WAVES) staged[k] = pos[s + k];
            __syncthreads();
            pr_polygon(staged, n, H, W, x0, y0, ny, xw0, xw1, acc);
        } else {
            pr_polygon(pos + s, n, H, W, x0, y0, ny, xw0, xw1, acc);
        }
    }

    uint8_t* plane = masks + inst * ((int64_t)H * W);
#pragma unroll
    for (int r = 0; r < PR_ROWS; ++r) {
        if (r < ny) {
            uint8_t* row = plane + (int64_t)(y0 + r) * W;
            if (vec) {                                     // W % 4 == 0 and a 4-byte aligned base: x0 < W has all four columns
                if (x0 < W) *reinterpret_cast<uint32_t*>(row + x0) = acc[r];
            } else {
#pragma unroll
                for (int c = 0; c < PR_COLS; ++c)
                    if (x0 + c < W) row[x0 + c] = (uint8_t)(acc[r] >> (8 * c));
            }
        }
    }
}

// offsets of cnt + 1 entries: start at 0, never decrease, end at `last`
static bool pr_offsets_ok(const int64_t* off, int64_t cnt, int64_t last) {
    if (off[0] != 0 || off[cnt] != last) return false;
    for (int64_t i = 0; i < cnt; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

extern "C" int dgx_polygons_to_bitmask(const int32_t* pos, int64_t n_pos, const int64_t* poly_off, const int64_t* inst_off,
                                       const int64_t* host_poly_off, const int64_t* host_inst_off, int N, int P, int H, int W,
                                       uint8_t* masks, void* stream) {
    if (N < 0 || P < 0 || H <= 0 || W <= 0 || n_pos < 0) return DGX_ERR_BAD_ARG;
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    if (N == 0) return DGX_OK;
    if (!masks || !poly_off || !inst_off || !host_poly_off || !host_inst_off || (n_pos > 0 && !pos)) return DGX_ERR_BAD_ARG;
    if (n_pos >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    if (!pr_offsets_ok(host_inst_off, N, P) || !pr_offsets_ok(host_poly_off, P, n_pos)) return DGX_ERR_BAD_ARG;
    const int tiles_x = (W + PR_TILE_W - 1) / PR_TILE_W, tiles_y = (H + PR_TILE_H - 1) / PR_TILE_H;
    const int64_t blocks = (int64_t)N * tiles_x * tiles_y;
    if (blocks >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    const int vec = (W % 4 == 0) && (((uintptr_t)masks & 3u) == 0);
    hipLaunchKernelGGL(pr_fill_kernel, dim3((unsigned)blocks), dim3(64 * PR_WAVES), 0, (hipStream_t)stream, pos, poly_off, inst_off, H, W,
                       tiles_x, tiles_y, vec, masks);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
