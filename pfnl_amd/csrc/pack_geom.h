// THE PACKED FORMATS (include/pfnl_hip.h PACKED FORMATS; the host rule: pfnl_amd/packed.py): one plane whose samples are interleaved within
// a pixel or a pixel group.  The table - the pixels and bytes of a unit, the family, depth and subsampling a side must have - the bytes of a
// row, the row of a tightly packed frame, and the one check of a packing against a side.  No HIP types and no HIP runtime calls: a plain
// C++ program can include this file and walk the rule (tests/test_packed_host.py does).
#pragma once
#include <stddef.h>

#include "../../include/pfnl_hip.h"

namespace pfnl {

struct PackInfo {
    bool yuv;                // the family of the side: YUV at 4:2:2, else RGB
    int bits;                // 8 or 10: the depth of the side
    int unit_px, unit_bytes; // a unit: the pixels it holds and its bytes
    int align;               // plane pointer, pitch and frame stride are multiples of this
};

// PFNL_PACK_BGR24 .. PFNL_PACK_V210, indexed by the enum's value (entry 0, PFNL_PACK_NONE, is no layout)
constexpr PackInfo PACK_TABLE[PFNL_PACK_V210 + 1] = {
    {false, 0, 1, 0, 1},     // none
    {false, 8, 1, 3, 1},     // bgr24    B G R
    {false, 8, 1, 4, 1},     // rgba     R G B A
    {false, 8, 1, 4, 1},     // bgra     B G R A
    {true, 8, 2, 4, 1},      // yuyv422  Y0 Cb Y1 Cr
    {true, 8, 2, 4, 1},      // uyvy422  Cb Y0 Cr Y1
    {false, 10, 1, 4, 4},    // x2rgb10  one uint32: R 29..20, G 19..10, B 9..0
    {false, 10, 1, 4, 4},    // x2bgr10  one uint32: B 29..20, G 19..10, R 9..0
    {true, 10, 2, 8, 2},     // y210     four uint16 Y0 Cb Y1 Cr, each value << 6
    {true, 10, 6, 16, 4},    // v210     four uint32 of three 10-bit samples
};

inline bool is_packing(int pack) { return pack > PFNL_PACK_NONE && pack <= PFNL_PACK_V210; }

// the bytes of a row that hold samples; 0: no such packing, or a width its unit does not divide
inline size_t pack_row_bytes(int pack, int W) {
    if (!is_packing(pack) || W < 1 || W % PACK_TABLE[pack].unit_px) return 0;
    return (size_t)(W / PACK_TABLE[pack].unit_px) * PACK_TABLE[pack].unit_bytes;
}

// the row of a tightly packed frame: v210's own rule rounds the width up to 48 pixels (128 bytes), for any W >= 1 (1280 -> 3456: also
// where pack_refused takes no frame of that width); every other packing's is its row bytes
inline size_t pack_tight_pitch(int pack, int W) {
    if (pack == PFNL_PACK_V210 && W >= 1) return (size_t)((W + 47) / 48) * 128;
    return pack_row_bytes(pack, W);
}

// the bytes of a tightly packed frame; 0 where there is no such frame
inline size_t pack_frame_bytes(int pack, int H, int W) { return H < 1 || !pack_row_bytes(pack, W) ? 0 : (size_t)H * pack_tight_pitch(pack, W); }

// nullptr: a side of this family, depth (8 | 10) and subsampling (PFNL_CHROMA_*) may carry `pack` at a width of W; else what disagrees.
// PFNL_PACK_NONE agrees with every side.
inline const char* pack_refused(int pack, bool family_is_yuv, int bits, int chroma, int W) {
    if (pack == PFNL_PACK_NONE) return nullptr;
    if (!is_packing(pack)) return "packing: PFNL_PACK_NONE .. PFNL_PACK_V210";
    const PackInfo& p = PACK_TABLE[pack];
    if (p.yuv != family_is_yuv)
        return p.yuv ? "packing: a YUV packing (yuyv422, uyvy422, y210, v210) needs a YUV family on its side, not RGB"
                     : "packing: an RGB packing (bgr24, rgba, bgra, x2rgb10, x2bgr10) needs an RGB family on its side, not YUV";
    if (p.bits != bits)
        return p.bits == 8 ? "packing: an 8-bit packing (bgr24, rgba, bgra, yuyv422, uyvy422) needs a depth of 8 bits on its side"
                           : "packing: a 10-bit packing (x2rgb10, x2bgr10, y210, v210) needs a depth of 10 bits on its side";
    if (p.yuv && chroma != PFNL_CHROMA_422) return "packing: a YUV packing needs the chroma format PFNL_CHROMA_422 on its side";
    if (W < 1) return "packing: the width must be at least 1";
    if (pack == PFNL_PACK_V210 && W % 6) return "packing: v210 needs a width that is a multiple of 6";
    if (p.yuv && (W & 1)) return "packing: a 4:2:2 packing needs an even width";
    return nullptr;
}

}  // namespace pfnl
