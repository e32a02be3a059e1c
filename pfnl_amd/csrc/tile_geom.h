// THE GEOMETRY OF A TILING (include/pfnl_hip.h TILES; the rule: pfnl_amd/tiles.py): the tiles of one axis, the grid of a frame, the tile
// a number names, and the one check every entry that takes a pfnl_tiling makes before it touches the device or its session.  No HIP types
// and no HIP runtime calls: a plain C++ program can include this file and walk the rule (tests/test_tiles_host.py does); under hipcc the
// same functions are callable from the kernels of tiles.hip, which is the only reason for the qualifier below.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pfnl_hip.h"

#ifdef __HIPCC__
#define PFNL_TILE_FN __host__ __device__ inline
#else
#define PFNL_TILE_FN inline
#endif

namespace pfnl {

// one axis of length n under tile extent t and margin p (tile_axis_refused has passed them)
struct TileAxis {
    int n, extent, pad, step, count;   // extent: t, or n where the axis is not split (count 1; step is then n)
};

// nullptr, or what is wrong with (n, t, p), in words that name the argument
inline const char* tile_axis_refused(int n, int t, int p) {
    if (n <= 0 || (n & 1)) return "tile: the axis length n must be positive and even";
    if (t < 0 || (t & 1)) return "tile: the tile extent must be even and not negative";
    if (p < 0) return "tile: pad must not be negative";
    if (t != 0 && t < n && 2 * (long long)p >= t) return "tile: 2 * pad must be smaller than the tile extent where the axis is split";
    return nullptr;
}

inline TileAxis tile_axis(int n, int t, int p) {
    if (t == 0 || t >= n) return TileAxis{n, n, p, n, 1};
    const int step = t - 2 * p;
    return TileAxis{n, t, p, step, (n - 2 * p + step - 1) / step};
}

// tile i of the axis: its origin and the range [first, end) it owns.  (i + 1) * step < n for every i + 1 < count.
PFNL_TILE_FN int tile_origin(const TileAxis& a, int i) {
    const int o = i * a.step, last = a.n - a.extent;
    return o < last ? o : last;
}
PFNL_TILE_FN int tile_own_first(const TileAxis& a, int i) { return i == 0 ? 0 : tile_origin(a, i) + a.pad; }
PFNL_TILE_FN int tile_own_end(const TileAxis& a, int i) { return i + 1 == a.count ? a.n : tile_origin(a, i + 1) + a.pad; }

struct TileGrid {
    TileAxis y, x;           // rows of tiles over H, columns over W; a tile is y.extent x x.extent
};

// tile k of a call, k = (b * ny + iy) * nx + ix
struct TilePos {
    int b;
    int oy, ox;              // its origin in the frame
    int ay, by, ax, bx;      // the rectangle it owns, in the frame
};

PFNL_TILE_FN TilePos tile_pos(const TileGrid& g, int k) {
    const int ix = k % g.x.count, row = k / g.x.count, iy = row % g.y.count;
    return TilePos{row / g.y.count,           tile_origin(g.y, iy),  tile_origin(g.x, ix), tile_own_first(g.y, iy),
                   tile_own_end(g.y, iy),     tile_own_first(g.x, ix), tile_own_end(g.x, ix)};
}

// nullptr: `t` tiles a frame of H x W; else what is wrong with it
inline const char* tiling_refused(int H, int W, const pfnl_tiling& t) {
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) return "tile: H and W must be positive and even";
    if (t.batch < 0) return "tile: batch must not be negative";
    if (const char* why = tile_axis_refused(H, t.tile_h, t.pad)) return why;
    if (const char* why = tile_axis_refused(W, t.tile_w, t.pad)) return why;
    if ((long long)tile_axis(H, t.tile_h, t.pad).count * tile_axis(W, t.tile_w, t.pad).count > INT_MAX)
        return "tile: the tile count overflows a 32-bit integer";
    return nullptr;
}

// (tiling_refused has passed)
inline TileGrid tile_grid(int H, int W, const pfnl_tiling& t) { return TileGrid{tile_axis(H, t.tile_h, t.pad), tile_axis(W, t.tile_w, t.pad)}; }

// the tiles of B clips, or 0 where the count overflows a 32-bit integer
inline int tile_total(const TileGrid& g, int B) {
    const long long total = (long long)B * g.y.count * g.x.count;
    return total > INT_MAX ? 0 : (int)total;
}

// the tiles of a full run: batch == 0 or more than there are: all of them
inline int tile_run(int total, int batch) { return batch == 0 || batch > total ? total : batch; }

}  // namespace pfnl
