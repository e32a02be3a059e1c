// The two launches of a tiled forward's run (include/pfnl_hip.h TILES; the geometry: tile_geom.h; the rule: pfnl_amd/tiles.py).
//   launch_tile_gather   in [B][T][H][W][3] -> tiles [count][T][th][tw][3]: tile k = first + j reads rows oy .. oy + th - 1, pixels ox .. ox + tw - 1
//   launch_tile_scatter  y [count][s th][s tw][3] -> out [B][s H][s W][3]: tile k writes the rectangle it owns, rows s ay .. s by - 1, pixels s ax .. s bx - 1
// Both are row copies: a row of a tile and the row of the frame it maps to are contiguous runs of floats, so a wave takes one row and its
// lanes consecutive words of it - consecutive addresses on both sides, no LDS, no arithmetic on the values (bits are copied).  A workgroup
// is 4 waves = 4 consecutive rows of one image of the grid's y (gather: a frame of a tile; scatter: a tile).  The word is 16, 8 or 4
// bytes: W, tw and every origin are even, so every row starts a multiple of 8 bytes from its base pointer, and a multiple of 16 where the
// origins and the row lengths are multiples of 4 pixels (scatter: times the scale).  The launchers OR every byte offset the kernel will
// form into the two base addresses and read the word off the result - a base pointer one float off 16 bytes takes the 4-byte kernel.
// The owned ranges partition the frame (tile_geom.h), so the scatter stores every output element once, by one thread: no atomics, no
// memset, nothing outside the destination touched.  Rows past a tile's owned rows leave at once (at most 2 pad of th).
#include "common.h"
#include "tile_geom.h"

namespace pfnl {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int TILE_ROWS = 4;                   // rows (waves) per workgroup

template <typename V>
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int floats) {
    const V* const s = reinterpret_cast<const V*>(src);
    V* const d = reinterpret_cast<V*>(dst);
    const int words = floats / (int)(sizeof(V) / sizeof(float));
#pragma unroll 4
    for (int w = threadIdx.x; w < words; w += 64) d[w] = s[w];
}

// grid (row groups of a tile, (tile of the run) * T + frame from img0 on)
template <typename V>
__global__ __launch_bounds__(64 * TILE_ROWS) void tile_gather_kernel(const float* __restrict__ in, float* __restrict__ tiles, TileGrid g, int T,
                                                                     int first, int img0) {
    const int th = g.y.extent, tw = g.x.extent;
    const int r = blockIdx.x * TILE_ROWS + threadIdx.y;
    if (r >= th) return;
    const int img = img0 + blockIdx.y, j = img / T, f = img - j * T;
    const TilePos p = tile_pos(g, first + j);
    const float* const s = in + ((((size_t)p.b * T + f) * g.y.n + p.oy + r) * g.x.n + p.ox) * 3;
    float* const d = tiles + ((size_t)img * th + r) * tw * 3;
    copy_row<V>(s, d, tw * 3);
}

// grid (row groups of a tile's result, tile of the run from j0 on)
template <typename V>
__global__ __launch_bounds__(64 * TILE_ROWS) void tile_scatter_kernel(const float* __restrict__ y, float* __restrict__ out, TileGrid g, int sc,
                                                                      int first, int j0) {
    const int j = j0 + blockIdx.y;
    const TilePos p = tile_pos(g, first + j);
    const int r = blockIdx.x * TILE_ROWS + threadIdx.y;
    if (r >= sc * (p.by - p.ay)) return;
    const size_t sth = (size_t)sc * g.y.extent, stw = (size_t)sc * g.x.extent, sH = (size_t)sc * g.y.n, sW = (size_t)sc * g.x.n;
    const float* const s = y + ((j * sth + (size_t)sc * (p.ay - p.oy) + r) * stw + (size_t)sc * (p.ax - p.ox)) * 3;
    float* const d = out + ((p.b * sH + (size_t)sc * p.ay + r) * sW + (size_t)sc * p.ax) * 3;
    copy_row<V>(s, d, sc * (p.bx - p.ax) * 3);
}

// the bytes of the widest word (16, 8 or 4) that divides every address in `bits` (the OR of the base addresses and all byte offsets)
int word_bytes(uintptr_t bits) { return !(bits & 15) ? 16 : !(bits & 7) ? 8 : 4; }

constexpr int GRID_Y = 65535;

}  // namespace

hipError_t launch_tile_gather(const float* in, float* tiles, const TileGrid& g, int T, int first, int count, hipStream_t s) {
    if (!in || !tiles || T < 1 || first < 0 || count < 1) return hipErrorInvalidValue;
    const int th = g.y.extent, tw = g.x.extent;
    uintptr_t bits = reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(tiles) | (uintptr_t)g.x.n * 12 | (uintptr_t)tw * 12;
    for (int ix = 0; ix < g.x.count; ++ix) bits |= (uintptr_t)tile_origin(g.x, ix) * 12;
    const int wb = word_bytes(bits);
    const long long imgs = (long long)count * T;
    const unsigned gx = (unsigned)((th + TILE_ROWS - 1) / TILE_ROWS);
    for (long long i0 = 0; i0 < imgs; i0 += GRID_Y) {
        if (i0 > 0x7fffffffLL) return hipErrorInvalidValue;
        const dim3 grid(gx, (unsigned)(imgs - i0 < GRID_Y ? imgs - i0 : GRID_Y)), block(64, TILE_ROWS);
        if (wb == 16) hipLaunchKernelGGL(tile_gather_kernel<f32x4>, grid, block, 0, s, in, tiles, g, T, first, (int)i0);
        else if (wb == 8) hipLaunchKernelGGL(tile_gather_kernel<f32x2>, grid, block, 0, s, in, tiles, g, T, first, (int)i0);
        else hipLaunchKernelGGL(tile_gather_kernel<float>, grid, block, 0, s, in, tiles, g, T, first, (int)i0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_tile_scatter(const float* y, float* out, const TileGrid& g, int scale, int first, int count, hipStream_t s) {
    if (!y || !out || scale < 1 || first < 0 || count < 1) return hipErrorInvalidValue;
    const int th = g.y.extent, tw = g.x.extent;
    if ((long long)scale * th > 0x7fffffffLL - TILE_ROWS) return hipErrorInvalidValue;
    const uintptr_t px = (uintptr_t)scale * 12;                                     // bytes of `scale` pixels: an LR pixel's width in a result row
    uintptr_t bits = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out) | (uintptr_t)g.x.n * px | (uintptr_t)tw * px;
    for (int ix = 0; ix < g.x.count; ++ix) {
        const int ox = tile_origin(g.x, ix), ax = tile_own_first(g.x, ix), bx = tile_own_end(g.x, ix);
        bits |= (uintptr_t)ax * px | (uintptr_t)(ax - ox) * px | (uintptr_t)(bx - ax) * px;
    }
    const int wb = word_bytes(bits);
    const unsigned gx = (unsigned)((scale * th + TILE_ROWS - 1) / TILE_ROWS);
    for (int j0 = 0; j0 < count; j0 += GRID_Y) {
        const dim3 grid(gx, (unsigned)(count - j0 < GRID_Y ? count - j0 : GRID_Y)), block(64, TILE_ROWS);
        if (wb == 16) hipLaunchKernelGGL(tile_scatter_kernel<f32x4>, grid, block, 0, s, y, out, g, scale, first, j0);
        else if (wb == 8) hipLaunchKernelGGL(tile_scatter_kernel<f32x2>, grid, block, 0, s, y, out, g, scale, first, j0);
        else hipLaunchKernelGGL(tile_scatter_kernel<float>, grid, block, 0, s, y, out, g, scale, first, j0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pfnl
