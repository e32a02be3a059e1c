// THE TWO ROUTES OF A STREAMING SESSION.  The output route (include/pfnl_hip.h pfnl_stream_format / pfnl_stream_resize): what a batch goes
// through between the fp32 result and pop - stage 0 quantise -> stage 1 resize (or a placement on a canvas: pfnl_stream_place) -> stage 2
// RGB -> YUV at the session's output subsampling (pfnl_stream_chroma_format; 4:2:0 unless it says otherwise), at 1 or 2 bytes per sample -,
// the bytes of a frame behind each stage, which stage pop reads, the one check of a (formats, size) setting that needs no session, and the
// one check of a placement's rectangles.  The input route (pfnl_stream_format / _input_depth / _chroma_format / _packing): what a pushed
// frame is - its surface format and geometry, the pitches and bytes of the tight frame, the staging frame a host push needs, the ring
// frame - and which decode takes it into its ring slot.  No HIP types and no HIP runtime calls: a plain C++ program can include this file
// and walk the rules (tests/test_route_host.py, tests/test_input_route_host.py and tests/test_place_host.py do).
#pragma once
#include "surface_geom.h"

namespace pfnl {

inline bool is_10bit(int fmt) { return fmt == PFNL_PIX_RGB10 || fmt == PFNL_PIX_P010 || fmt == PFNL_PIX_I010; }
inline bool is_420(int fmt) { return fmt == PFNL_PIX_NV12 || fmt == PFNL_PIX_I420 || fmt == PFNL_PIX_P010 || fmt == PFNL_PIX_I010; }
inline bool is_yuv(int fmt) { return is_420(fmt); }   // the YUV layouts: 4:2:0 by name, at any subsampling with PFNL_CHROMA_*
inline bool is_chroma(int chroma) { return chroma >= PFNL_CHROMA_420 && chroma <= PFNL_CHROMA_444; }

constexpr int ROUTE_STAGES = 3;   // 0 quantise (always) | 1 resize (a size is set) | 2 RGB -> YUV (a YUV out_fmt) or -> a packing (pack_geom.h)

struct OutRoute {
    bool runs[ROUTE_STAGES];
    int sample_bytes;                  // 1, or 2 for RGB10 / P010 / I010; 0: no such format, and no stage runs
    size_t stage_bytes[ROUTE_STAGES];  // one frame as the stage writes it; 0 where it does not run
    int last;                          // the last stage that runs: pop reads its slot
    int out_h, out_w;                  // the delivered frame,
    size_t frame_bytes;                // and its bytes = stage_bytes[last]
};

// the packed frame is its planes one behind the other: rows of row_bytes, nothing between
inline size_t packed_bytes(const SurfaceGeom& g) {
    size_t n = 0;
    for (int k = 0; k < g.planes; ++k) n += g.plane[k].rows * g.plane[k].row_bytes;
    return n;
}

// sH x sW: the network's raster; oH = oW = 0: no resampling; chroma: the subsampling of a YUV out_fmt; pack: the output side's packing,
// which is stage 2 for an RGB out_fmt too and delivers the tightly packed frame (pack_frame_bytes).  Sizes are what route_refused has let
// through.
inline OutRoute out_route(int out_fmt, int sH, int sW, int oH, int oW, int chroma = PFNL_CHROMA_420, int pack = PFNL_PACK_NONE) {
    OutRoute r{};
    r.out_h = oH ? oH : sH;
    r.out_w = oW ? oW : sW;
    const SurfaceGeom g = surface_geom(out_fmt, r.out_h, r.out_w, chroma, pack);
    if (!g.planes) return r;
    const int rgb = is_10bit(out_fmt) ? PFNL_PIX_RGB10 : PFNL_PIX_RGB24;
    const SurfaceGeom writes[ROUTE_STAGES] = {surface_geom(rgb, sH, sW), surface_geom(rgb, r.out_h, r.out_w), g};
    r.sample_bytes = g.sample_bytes;
    r.runs[0] = true, r.runs[1] = oH != 0, r.runs[2] = is_yuv(out_fmt) || pack != PFNL_PACK_NONE;
    for (int k = 0; k < ROUTE_STAGES; ++k)
        if (r.runs[k]) r.last = k, r.stage_bytes[k] = packed_bytes(writes[k]);
    if (pack != PFNL_PACK_NONE) r.stage_bytes[2] = pack_frame_bytes(pack, r.out_h, r.out_w);
    r.frame_bytes = r.stage_bytes[r.last];
    return r;
}

// THE INPUT ROUTE: a frame of H x W as it is pushed under (in_fmt, in_depth, in_chroma, in_pack) and the decode that makes it a ring frame.
enum InDecode {
    IN_DECODE_NONE = 0,   // no such setting: surface_geom or pack_refused refuses it, and every size is 0
    IN_DECODE_COPY,       // planar RGB: the ring's own layout
    IN_DECODE_420,        // NV12 / I420 (P010 / I010) at 4:2:0: yuv.hip
    IN_DECODE_CHROMA,     // the same layouts at 4:2:2 / 4:4:4: yuv_chroma.hip
    IN_DECODE_PACK,       // one plane of interleaved samples: packed.hip
};

struct InRoute {
    int kind;             // InDecode
    int fmt;              // the pushed surface's format: in_fmt names the layout, the depth the sample (RGB10 / P010 / I010 at 10 bits)
    SurfaceGeom geom;     // ... and its planes (surface_geom)
    size_t pitch[3];      // the pitch of each plane in a tight frame: its row bytes; a packing's pack_tight_pitch (v210's is above them)
    size_t frame_bytes;   // the tight frame: its planes one behind the other at those pitches
    size_t staging_bytes; // what a host push stages on the device ahead of the decode: the tight frame; 0 for planar RGB, copied as it is
    size_t ring_bytes;    // the frame as the ring holds it: H W 3 samples
    int sample_bytes;     // 1, or 2 at a depth of 10
};

inline InRoute in_route(int in_fmt, int in_depth, int in_chroma, int in_pack, int H, int W) {
    InRoute r{};
    if (in_fmt < PFNL_PIX_RGB24 || in_fmt > PFNL_PIX_I420 || (in_depth != 8 && in_depth != 10)) return r;
    const int fmt = in_depth != 10 ? in_fmt : (in_fmt == PFNL_PIX_NV12 ? PFNL_PIX_P010 : (in_fmt == PFNL_PIX_I420 ? PFNL_PIX_I010 : PFNL_PIX_RGB10));
    const SurfaceGeom g = surface_geom(fmt, H, W, in_chroma, in_pack);
    if (!g.planes) return r;
    const bool packed = in_pack != PFNL_PACK_NONE;
    r.fmt = fmt;
    r.geom = g;
    r.sample_bytes = g.sample_bytes;
    for (int k = 0; k < g.planes; ++k) {
        r.pitch[k] = packed ? pack_tight_pitch(in_pack, W) : g.plane[k].row_bytes;
        r.frame_bytes += g.plane[k].rows * r.pitch[k];
    }
    r.kind = packed ? IN_DECODE_PACK : (in_fmt == PFNL_PIX_RGB24 ? IN_DECODE_COPY : (in_chroma == PFNL_CHROMA_420 ? IN_DECODE_420 : IN_DECODE_CHROMA));
    r.staging_bytes = r.kind == IN_DECODE_COPY ? 0 : r.frame_bytes;
    r.ring_bytes = (size_t)H * W * 3 * g.sample_bytes;
    return r;
}

// nullptr: a session may take in_fmt -> out_fmt and deliver out_h x out_w; else why not.  Both setters ask this before they look at
// the session's state, each with the other's current setting.  chroma: the subsampling of a YUV out_fmt - the size is even along the axes
// it halves: both at 4:2:0, the width at 4:2:2, none at 4:4:4.  pack: the output side's packing, which must agree with out_fmt's family and
// depth, the chroma format and the output width (pack_refused).
inline const char* route_refused(int in_fmt, int out_fmt, int out_h, int out_w, int chroma = PFNL_CHROMA_420, int pack = PFNL_PACK_NONE) {
    if (!is_chroma(chroma)) return "chroma format: PFNL_CHROMA_420, PFNL_CHROMA_422 or PFNL_CHROMA_444";
    if (is_10bit(in_fmt))
        return "format: 10-bit input is set with pfnl_stream_input_depth; in_fmt names the layout: PFNL_PIX_RGB24, PFNL_PIX_NV12 or PFNL_PIX_I420";
    if (in_fmt < PFNL_PIX_RGB24 || in_fmt > PFNL_PIX_I420 || out_fmt < PFNL_PIX_RGB24 || out_fmt > PFNL_PIX_I010)
        return "format: PFNL_PIX_RGB24, PFNL_PIX_NV12 or PFNL_PIX_I420, and as out_fmt PFNL_PIX_RGB10, PFNL_PIX_P010 or PFNL_PIX_I010";
    if (in_fmt != PFNL_PIX_RGB24 && out_fmt == PFNL_PIX_RGB10)
        return "format: PFNL_PIX_RGB10 is delivered for RGB24 input only (a YUV in_fmt pairs with a YUV out_fmt or RGB24)";
    if (is_yuv(out_fmt) && chroma == PFNL_CHROMA_420 && ((out_h | out_w) & 1))
        return "a YUV output format needs an even output size (pfnl_stream_format, pfnl_stream_resize)";
    if (is_yuv(out_fmt) && chroma == PFNL_CHROMA_422 && (out_w & 1))
        return "a 4:2:2 output needs an even output width (pfnl_stream_chroma_format, pfnl_stream_resize)";
    if (pack != PFNL_PACK_NONE) return pack_refused(pack, is_yuv(out_fmt), is_10bit(out_fmt) ? 10 : 8, chroma, out_w);
    return nullptr;
}

// A PLACEMENT (include/pfnl_hip.h pfnl_stream_place, pfnl_op_resize_place_u8 / _u10; the rule: pfnl_amd/fit.py check_rects): nullptr where
// `src` is a rectangle of the raster sH x sW, `dst` one of the canvas oH x oW and the resampler takes src -> dst on both axes; else why
// not, in words that name src or dst.  The session and the op hooks ask this before any HIP call and before any change to a session.
constexpr int PLACE_MAX_SIZE = 16384;   // a side of raster and canvas (RESIZE_MAX_SIZE: pfnl_resize_taps' limit)

inline const char* place_refused(int sH, int sW, int oH, int oW, const pfnl_rect& src, const pfnl_rect& dst) {
    if (sH < 1 || sW < 1 || sH > PLACE_MAX_SIZE || sW > PLACE_MAX_SIZE) return "place: the raster src lies in must be 1 .. 16384 a side";
    if (oH < 1 || oW < 1 || oH > PLACE_MAX_SIZE || oW > PLACE_MAX_SIZE) return "place: the canvas dst lies in must be 1 .. 16384 a side";
    const auto inside = [](const pfnl_rect& r, int H, int W) {   // (64 bits: y + h of two int32 cannot wrap)
        return r.h >= 1 && r.w >= 1 && r.y >= 0 && r.x >= 0 && (long long)r.y + r.h <= H && (long long)r.x + r.w <= W;
    };
    if (!inside(src, sH, sW)) return "place: src must have h, w >= 1 and lie inside the raster";
    if (!inside(dst, oH, oW)) return "place: dst must have h, w >= 1 and lie inside the canvas";
    const auto takes = [](int n_in, int n_out) { return n_out >= (n_in + 3) / 4 && n_out <= 2 * n_in; };
    if (!takes(src.h, dst.h)) return "place: src.h -> dst.h: the output must lie between a quarter and twice the input";
    if (!takes(src.w, dst.w)) return "place: src.w -> dst.w: the output must lie between a quarter and twice the input";
    return nullptr;
}

}  // namespace pfnl
