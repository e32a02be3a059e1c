// THE GEOMETRY OF A SURFACE (include/pfnl_hip.h SURFACES): the planes a pixel format has, the rows and the bytes per row of each for a frame
// of H x W, and the one check every entry that takes a pfnl_surface makes before it touches the device or its session.  No HIP types and
// no HIP runtime calls: a plain C++ program can include this file and walk the rule (tests/test_surface_host.py does).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pfnl_hip.h"
#include "pack_geom.h"

namespace pfnl {

struct SurfacePlane {
    int rows;
    size_t row_bytes;        // the bytes of a row that hold samples; the pitch is at least this
};

struct SurfaceGeom {
    int planes;              // 1 (RGB24 / RGB10), 2 (NV12 / P010) or 3 (I420 / I010); 0: no such format
    int sample_bytes;        // 1, or 2 for the 10-bit formats
    SurfacePlane plane[3];
    int align;               // every plane pointer and pitch is a multiple of this: sample_bytes, or a packing's own (pack_geom.h)
};

// H and W are the frame's (even for the 4:2:0 formats: the entries check that with their own geometry).  chroma: PFNL_CHROMA_*, the
// subsampling of a YUV format's chroma planes - H rows at 4:2:2, H rows of twice the samples at 4:4:4; an RGB format ignores it.
// pack: PFNL_PACK_*; a packing replaces the planes by ONE plane of H rows of pack_row_bytes, where fmt's family and depth, the chroma
// format and W agree with it (pack_refused), and fmt then says no more than that family and depth.
inline SurfaceGeom surface_geom(int fmt, int H, int W, int chroma = PFNL_CHROMA_420, int pack = PFNL_PACK_NONE) {
    SurfaceGeom g{};
    if (fmt < PFNL_PIX_RGB24 || fmt > PFNL_PIX_I010 || H < 1 || W < 1 || chroma < PFNL_CHROMA_420 || chroma > PFNL_CHROMA_444) return g;
    if (pack != PFNL_PACK_NONE) {
        const bool yuv = fmt != PFNL_PIX_RGB24 && fmt != PFNL_PIX_RGB10;
        if (pack_refused(pack, yuv, fmt >= PFNL_PIX_RGB10 ? 10 : 8, chroma, W)) return g;
        g.planes = 1;
        g.sample_bytes = fmt >= PFNL_PIX_RGB10 ? 2 : 1;
        g.plane[0] = {H, pack_row_bytes(pack, W)};
        g.align = PACK_TABLE[pack].align;
        return g;
    }
    const int ch = chroma == PFNL_CHROMA_420 ? H / 2 : H;               // rows of a chroma plane,
    const size_t cw = chroma == PFNL_CHROMA_444 ? (size_t)W : (size_t)W / 2;   // and samples in a row of one
    const size_t b = fmt >= PFNL_PIX_RGB10 ? 2 : 1, w = (size_t)W;
    g.sample_bytes = g.align = (int)b;
    if (fmt == PFNL_PIX_RGB24 || fmt == PFNL_PIX_RGB10) {
        g.planes = 1;
        g.plane[0] = {H, 3 * w * b};
    } else if (fmt == PFNL_PIX_NV12 || fmt == PFNL_PIX_P010) {
        g.planes = 2;
        g.plane[0] = {H, w * b};
        g.plane[1] = {ch, 2 * cw * b};               // Cb and Cr interleaved: W / 2 pairs (4:4:4: W)
    } else {
        g.planes = 3;
        g.plane[0] = {H, w * b};
        g.plane[1] = g.plane[2] = {ch, cw * b};
    }
    return g;
}

// nullptr: `sf` describes a frame of H x W in `fmt`; else what is wrong with it, in words that name the plane or the pitch.  Entries past
// the format's planes are not looked at.
inline const char* surface_refused(const pfnl_surface* sf, int fmt, int H, int W, int chroma = PFNL_CHROMA_420, int pack = PFNL_PACK_NONE) {
    if (!sf) return "NULL argument";
    const SurfaceGeom g = surface_geom(fmt, H, W, chroma, pack);
    if (!g.planes) return "surface: no plane layout for this format and size";
    for (int k = 0; k < g.planes; ++k) {
        if (!sf->plane[k]) return "surface: a plane the format needs is NULL";
        if (sf->pitch[k] < g.plane[k].row_bytes) return "surface: a pitch is smaller than the bytes of a row of its plane";
        if (g.sample_bytes == 2 && ((reinterpret_cast<uintptr_t>(sf->plane[k]) | sf->pitch[k]) & 1))
            return "surface: 16-bit samples need an even plane pointer and an even pitch";
        if (g.align == 4 && ((reinterpret_cast<uintptr_t>(sf->plane[k]) | sf->pitch[k]) & 3))
            return "surface: a packing of 32-bit words (x2rgb10, x2bgr10, v210) needs a plane pointer and a pitch that are multiples of 4";
    }
    return nullptr;
}

}  // namespace pfnl
