// PACKED FORMATS <-> packed RGB (include/pfnl_hip.h PACKED FORMATS; the table: pack_geom.h): bgr24 / rgba / bgra, yuyv422 / uyvy422 and, with
// uint16 samples on the RGB side, x2rgb10 / x2bgr10, y210 and v210.  One plane whose samples are interleaved within a pixel or a pixel group.
// The arithmetic is the 4:2:2 rule of yuv_chroma.hip - the same coefficient table, the same sample primitives (sample_depth.h), the same
// taps and roundings - behind another LAYOUT, stated once on the host in pfnl_amd/packed.py: unpack, then pfnl_amd/yuv.py / depth10.py with
// chroma = "422".  An RGB packing is a permutation of samples and no arithmetic at all.
// There is no vertical coupling, so a lane owns ONE row by the pixels of one 16-byte word of the packed side (4: rgba / bgra / x2* / y210,
// 8: yuyv / uyvy, 6: v210; bgr24: 16 pixels = three words), or - where the plane, its pitch or the frame stride do not put rows on 16 bytes,
// and for the tail of a row that is no whole number of such strips - by ONE UNIT (a pixel, a pixel pair, a v210 group).  The packed side is
// handled as the 32-bit words of the strip, loaded and stored as wide as the strip's address allows (16 bytes, 4 bytes, single bytes); the
// RGB side moves in the widest words its address allows, else sample by sample.  No form is chosen from a flag alone: every access reads
// its width off its own address.  Edges are index clamps inside the one kernel, and the neighbouring chroma sample (decode) or RGB column
// (co-sited encode) comes from memory.
#include "pack_geom.h"
#include "sample_depth.h"

namespace pfnl {

namespace {

__device__ __forceinline__ size_t lane_index() { return (size_t)blockIdx.x * 256 + threadIdx.x; }

// NB bytes at p -> the words w[0 .. ceil(NB / 4)), little-endian; a last partial word is zero above its bytes
template <int NB>
__device__ __forceinline__ void load_packed(const uint8_t* __restrict__ p, unsigned* w) {
    constexpr int ND = (NB + 3) / 4;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if constexpr (NB % 16 == 0) {
        if (a % 16 == 0) {
#pragma unroll
            for (int k = 0; k < ND; k += 4) {
                const u32x4 q = *reinterpret_cast<const u32x4*>(p + 4 * k);
                w[k] = q.x, w[k + 1] = q.y, w[k + 2] = q.z, w[k + 3] = q.w;
            }
            return;
        }
    }
    if constexpr (NB % 4 == 0) {
        if (a % 4 == 0) {
#pragma unroll
            for (int k = 0; k < ND; ++k) w[k] = *reinterpret_cast<const unsigned*>(p + 4 * k);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) w[k] = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) w[j / 4] |= (unsigned)p[j] << (8 * (j % 4));
}

template <int NB>
__device__ __forceinline__ void store_packed(uint8_t* __restrict__ p, const unsigned* w) {
    constexpr int ND = (NB + 3) / 4;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if constexpr (NB % 16 == 0) {
        if (a % 16 == 0) {
#pragma unroll
            for (int k = 0; k < ND; k += 4) *reinterpret_cast<u32x4*>(p + 4 * k) = u32x4{w[k], w[k + 1], w[k + 2], w[k + 3]};
            return;
        }
    }
    if constexpr (NB % 4 == 0) {
        if (a % 4 == 0) {
#pragma unroll
            for (int k = 0; k < ND; ++k) *reinterpret_cast<unsigned*>(p + 4 * k) = w[k];
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) p[j] = (uint8_t)(w[j / 4] >> (8 * (j % 4)));
}

// N samples of the RGB side, in words where p sits on the word N samples allow
template <typename T, int N>
__device__ __forceinline__ void load_rgb(const T* __restrict__ p, int* v) {
    if (reinterpret_cast<uintptr_t>(p) % word_of<T, N>() == 0)
        load_samples<T, N, true>(p, v);
    else
        load_samples<T, N, false>(p, v);
}

template <typename T, int N>
__device__ __forceinline__ void store_rgb(T* __restrict__ p, const int* v) {
    if (reinterpret_cast<uintptr_t>(p) % word_of<T, N>() == 0)
        store_samples<T, N, true>(p, v);
    else
        store_samples<T, N, false>(p, v);
}

__device__ __forceinline__ int byte_of(const unsigned* w, int j) { return (int)((w[j / 4] >> (8 * (j % 4))) & 255u); }

// ---- the packings: T the sample of the RGB side; a unit's pixels and bytes; the pixels of a strip of 16-byte words; N pixels <-> words ----
struct PackBgr24 {
    typedef uint8_t T;
    static constexpr bool YUV = false;
    static constexpr int UNIT_PX = 1, UNIT_BYTES = 3, WIDE_PX = 16;
    template <int N>
    static __device__ __forceinline__ void unpack(const unsigned* w, int* px) {
#pragma unroll
        for (int p = 0; p < N; ++p) px[3 * p] = byte_of(w, 3 * p + 2), px[3 * p + 1] = byte_of(w, 3 * p + 1), px[3 * p + 2] = byte_of(w, 3 * p);
    }
    template <int N>
    static __device__ __forceinline__ void pack(unsigned* w, const int* px) {
#pragma unroll
        for (int k = 0; k < (3 * N + 3) / 4; ++k) w[k] = 0;
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) w[(3 * p + ch) / 4] |= (unsigned)(px[3 * p + 2 - ch] & 255) << (8 * ((3 * p + ch) % 4));
    }
};

template <int RPOS, int BPOS>                                // the bytes of R and B in the pixel's word; G is byte 1, alpha byte 3
struct PackRgba {
    typedef uint8_t T;
    static constexpr bool YUV = false;
    static constexpr int UNIT_PX = 1, UNIT_BYTES = 4, WIDE_PX = 4;
    template <int N>
    static __device__ __forceinline__ void unpack(const unsigned* w, int* px) {
#pragma unroll
        for (int p = 0; p < N; ++p)
            px[3 * p] = (int)((w[p] >> (8 * RPOS)) & 255u), px[3 * p + 1] = (int)((w[p] >> 8) & 255u), px[3 * p + 2] = (int)((w[p] >> (8 * BPOS)) & 255u);
    }
    template <int N>
    static __device__ __forceinline__ void pack(unsigned* w, const int* px) {
#pragma unroll
        for (int p = 0; p < N; ++p)
            w[p] = ((unsigned)(px[3 * p] & 255) << (8 * RPOS)) | ((unsigned)(px[3 * p + 1] & 255) << 8) | ((unsigned)(px[3 * p + 2] & 255) << (8 * BPOS)) |
                   0xFF000000u;
    }
};

template <int RSH, int BSH>                                  // the bit of R and of B in the pixel's word; G is at 10, the spare bits 31..30
struct PackX2 {
    typedef uint16_t T;
    static constexpr bool YUV = false;
    static constexpr int UNIT_PX = 1, UNIT_BYTES = 4, WIDE_PX = 4;
    template <int N>
    static __device__ __forceinline__ void unpack(const unsigned* w, int* px) {
#pragma unroll
        for (int p = 0; p < N; ++p)
            px[3 * p] = (int)((w[p] >> RSH) & 1023u), px[3 * p + 1] = (int)((w[p] >> 10) & 1023u), px[3 * p + 2] = (int)((w[p] >> BSH) & 1023u);
    }
    template <int N>
    static __device__ __forceinline__ void pack(unsigned* w, const int* px) {
#pragma unroll
        for (int p = 0; p < N; ++p)
            w[p] = ((unsigned)(px[3 * p] & 1023) << RSH) | ((unsigned)(px[3 * p + 1] & 1023) << 10) | ((unsigned)(px[3 * p + 2] & 1023) << BSH) |
                   0xC0000000u;
    }
};

template <int YPOS>                                          // the byte of Y0 in a pair's word: 0 yuyv (Y0 Cb Y1 Cr) | 1 uyvy (Cb Y0 Cr Y1)
struct PackYuyv {
    typedef uint8_t T;
    static constexpr bool YUV = true;
    static constexpr int UNIT_PX = 2, UNIT_BYTES = 4, WIDE_PX = 8, CPOS = 1 - YPOS;
    template <int N>
    static __device__ __forceinline__ void unpack(const unsigned* w, int* y, int* cb, int* cr) {
#pragma unroll
        for (int q = 0; q < N / 2; ++q) {
            y[2 * q] = (int)((w[q] >> (8 * YPOS)) & 255u), y[2 * q + 1] = (int)((w[q] >> (8 * YPOS + 16)) & 255u);
            cb[q] = (int)((w[q] >> (8 * CPOS)) & 255u), cr[q] = (int)((w[q] >> (8 * CPOS + 16)) & 255u);
        }
    }
    template <int N>
    static __device__ __forceinline__ void pack(unsigned* w, const int* y, const int* cb, const int* cr) {
#pragma unroll
        for (int q = 0; q < N / 2; ++q)
            w[q] = ((unsigned)y[2 * q] << (8 * YPOS)) | ((unsigned)y[2 * q + 1] << (8 * YPOS + 16)) | ((unsigned)cb[q] << (8 * CPOS)) |
                   ((unsigned)cr[q] << (8 * CPOS + 16));
    }
    // chroma sample i of the row
    static __device__ __forceinline__ void chroma_at(const uint8_t* __restrict__ row, int i, int* cb, int* cr) {
        *cb = row[4 * (size_t)i + CPOS], *cr = row[4 * (size_t)i + CPOS + 2];
    }
};

struct PackY210 {                                                      // four uint16 Y0 Cb Y1 Cr, the value in the upper ten bits (the low six ignored)
    typedef uint16_t T;
    static constexpr bool YUV = true;
    static constexpr int UNIT_PX = 2, UNIT_BYTES = 8, WIDE_PX = 4;
    template <int N>
    static __device__ __forceinline__ void unpack(const unsigned* w, int* y, int* cb, int* cr) {
#pragma unroll
        for (int q = 0; q < N / 2; ++q) {
            y[2 * q] = (int)((w[2 * q] & 0xFFFFu) >> 6), cb[q] = (int)(w[2 * q] >> 22);
            y[2 * q + 1] = (int)((w[2 * q + 1] & 0xFFFFu) >> 6), cr[q] = (int)(w[2 * q + 1] >> 22);
        }
    }
    template <int N>
    static __device__ __forceinline__ void pack(unsigned* w, const int* y, const int* cb, const int* cr) {
#pragma unroll
        for (int q = 0; q < N / 2; ++q) {
            w[2 * q] = ((unsigned)y[2 * q] << 6) | ((unsigned)cb[q] << 22);
            w[2 * q + 1] = ((unsigned)y[2 * q + 1] << 6) | ((unsigned)cr[q] << 22);
        }
    }
    static __device__ __forceinline__ void chroma_at(const uint8_t* __restrict__ row, int i, int* cb, int* cr) {
        const uint16_t* const r = reinterpret_cast<const uint16_t*>(row) + 4 * (size_t)i;   // (the launcher has seen an even row address)
        *cb = r[1] >> 6, *cr = r[3] >> 6;
    }
};

struct PackV210 {   // four uint32 of three 10-bit samples at bits 9..0, 19..10, 29..20: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
    typedef uint16_t T;
    static constexpr bool YUV = true;
    static constexpr int UNIT_PX = 6, UNIT_BYTES = 16, WIDE_PX = 6;
    static __device__ __forceinline__ int field(unsigned w, int k) { return (int)((w >> (10 * k)) & 1023u); }
    template <int N>
    static __device__ __forceinline__ void unpack(const unsigned* w, int* y, int* cb, int* cr) {
        static_assert(N == 6, "one group");
        cb[0] = field(w[0], 0), y[0] = field(w[0], 1), cr[0] = field(w[0], 2);
        y[1] = field(w[1], 0), cb[1] = field(w[1], 1), y[2] = field(w[1], 2);
        cr[1] = field(w[2], 0), y[3] = field(w[2], 1), cb[2] = field(w[2], 2);
        y[4] = field(w[3], 0), cr[2] = field(w[3], 1), y[5] = field(w[3], 2);
    }
    template <int N>
    static __device__ __forceinline__ void pack(unsigned* w, const int* y, const int* cb, const int* cr) {
        static_assert(N == 6, "one group");
        const auto word = [](int a, int b, int c) { return (unsigned)a | ((unsigned)b << 10) | ((unsigned)c << 20); };   // (bits 31..30: 0)
        w[0] = word(cb[0], y[0], cr[0]);
        w[1] = word(y[1], cb[1], y[2]);
        w[2] = word(cr[1], y[3], cb[2]);
        w[3] = word(y[4], cr[2], y[5]);
    }
    static __device__ __forceinline__ void chroma_at(const uint8_t* __restrict__ row, int i, int* cb, int* cr) {
        const int g = i / 3, k = i - 3 * g;                            // pair k of group g: Cb in word k at field k; Cr in word 0 | 2 | 3 at field 2 | 0 | 1
        const unsigned* const w = reinterpret_cast<const unsigned*>(row + 16 * (size_t)g);   // (the launcher has seen a row address on 4 bytes)
        *cb = field(w[k], k);
        *cr = field(w[k == 0 ? 0 : k + 1], k == 0 ? 2 : k - 1);
    }
};

typedef PackRgba<0, 2> PackRGBA;
typedef PackRgba<2, 0> PackBGRA;
typedef PackX2<20, 0> PackX2RGB10;
typedef PackX2<0, 20> PackX2BGR10;
typedef PackYuyv<0> PackYUYV;
typedef PackYuyv<1> PackUYVY;

// The N pixels x0 .. x0 + N - 1 of one row, packed -> RGB.  YUV: the N / 2 chroma samples i0 .. of the strip and the one to their right
// (clamped onto the last); MID (chroma midway between two luma columns) reads the one to their left as well (clamped onto 0).  The taps
// and the conversion are yuv_chroma.hip's at 4:2:2.
template <class PK, bool MID, int N>
__device__ __forceinline__ void decode_strip(const uint8_t* __restrict__ prow, typename PK::T* __restrict__ rrow, int x0, int W, const YuvCoef& c) {
    typedef typename PK::T T;
    constexpr int NB = N / PK::UNIT_PX * PK::UNIT_BYTES, LEVELS = Depth<T>::LEVELS;
    unsigned w[(NB + 3) / 4];
    load_packed<NB>(prow + (size_t)(x0 / PK::UNIT_PX) * PK::UNIT_BYTES, w);
    int out[3 * N];
    if constexpr (!PK::YUV) {
        PK::template unpack<N>(w, out);
    } else {
        constexpr int NC = N / 2, L = MID ? 1 : 0;
        int luma[N], cb[L + NC + 1], cr[L + NC + 1];                   // [L + q]: sample i0 + q
        PK::template unpack<N>(w, luma, cb + L, cr + L);
        const int cw = W >> 1, i0 = x0 >> 1;
        const int ie = i0 + NC < cw ? i0 + NC : cw - 1;
        PK::chroma_at(prow, ie, &cb[L + NC], &cr[L + NC]);
        if constexpr (MID) {
            const int il = i0 > 0 ? i0 - 1 : 0;
            PK::chroma_at(prow, il, &cb[0], &cr[0]);
        }
#pragma unroll
        for (int px = 0; px < N; ++px) {
            int u, v;
            if constexpr (MID) {                                       // near sample [1 + q], far [q] | [2 + q]
                const int q = px >> 1, far = px & 1 ? q + 2 : q;
                u = (3 * cb[q + 1] + cb[far] + 2) >> 2;
                v = (3 * cr[q + 1] + cr[far] + 2) >> 2;
            } else {
                const int q = px >> 1, e = px & 1 ? q + 1 : q;
                u = (cb[q] + cb[e] + 1) >> 1;
                v = (cr[q] + cr[e] + 1) >> 1;
            }
            u -= Depth<T>::CHROMA, v -= Depth<T>::CHROMA;
            const int yy = c.dy * (luma[px] - c.y0) + (1 << 13);
            out[3 * px] = shift_clip<14, LEVELS>(yy + c.drv * v);
            out[3 * px + 1] = shift_clip<14, LEVELS>(yy + c.dgu * u + c.dgv * v);
            out[3 * px + 2] = shift_clip<14, LEVELS>(yy + c.dbu * u);
        }
    }
    store_rgb<T, 3 * N>(rrow + (size_t)x0 * 3, out);
}

// The N pixels x0 .. of one row, RGB -> packed.  YUV: N luma samples and N / 2 samples of each chroma from the unrounded numerators; co-sited:
// 1-2-1 over the columns 2i - 1, 2i, 2i + 1 - only the column left of the strip is not its own, and at x = 0 it clamps onto column 0 - and
// 16 bits of shift; midway: the box over 2i, 2i + 1, 15 bits (yuv_chroma.hip at 4:2:2).
template <class PK, bool MID, int N>
__device__ __forceinline__ void encode_strip(const typename PK::T* __restrict__ rrow, uint8_t* __restrict__ prow, int x0, const YuvCoef& c) {
    typedef typename PK::T T;
    constexpr int NB = N / PK::UNIT_PX * PK::UNIT_BYTES, LEVELS = Depth<T>::LEVELS;
    constexpr int L = PK::YUV && !MID ? 1 : 0;                         // RGB columns read left of the strip
    int px[3 * (N + L)];                                               // [L + p]: column x0 + p
    if constexpr (L) {
        const size_t xl = x0 > 0 ? x0 - 1 : 0;
        px[0] = rrow[3 * xl], px[1] = rrow[3 * xl + 1], px[2] = rrow[3 * xl + 2];
    }
    load_rgb<T, 3 * N>(rrow + (size_t)x0 * 3, px + 3 * L);
    unsigned w[(NB + 3) / 4];
    if constexpr (!PK::YUV) {
        PK::template pack<N>(w, px);
    } else {
        constexpr int NC = N / 2, CS = 14 + (MID ? 1 : 2);
        constexpr int BIAS = (1 << (CS - 1)) + (Depth<T>::CHROMA << CS);   // the rounding and the chroma offset
        int luma[N], nb[N + L], nr[N + L], ob[NC], orr[NC];
#pragma unroll
        for (int p = 0; p < N + L; ++p) {
            const int r = px[3 * p], gg = px[3 * p + 1], b = px[3 * p + 2];
            nb[p] = c.cbr * r + c.cbg * gg + c.cbb * b;
            nr[p] = c.crr * r + c.crg * gg + c.crb * b;
            if (p >= L) luma[p - L] = shift_clip<14, LEVELS>(c.yr * r + c.yg * gg + c.yb * b + (c.y0 << 14) + (1 << 13));
        }
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            if constexpr (MID) {
                ob[q] = shift_clip<CS, LEVELS>(nb[2 * q] + nb[2 * q + 1] + BIAS);
                orr[q] = shift_clip<CS, LEVELS>(nr[2 * q] + nr[2 * q + 1] + BIAS);
            } else {
                ob[q] = shift_clip<CS, LEVELS>(nb[2 * q] + 2 * nb[2 * q + 1] + nb[2 * q + 2] + BIAS);
                orr[q] = shift_clip<CS, LEVELS>(nr[2 * q] + 2 * nr[2 * q + 1] + nr[2 * q + 2] + BIAS);
            }
        }
        PK::template pack<N>(w, luma, ob, orr);
    }
    store_packed<NB>(prow + (size_t)(x0 / PK::UNIT_PX) * PK::UNIT_BYTES, w);
}

// a row as the launch deals it out: `wide` strips of WIDE_PX pixels first (0 in a narrow launch), then the rest unit by unit
template <class PK>
__device__ __forceinline__ int wide_strips(int W, int wide) {
    return PK::WIDE_PX > PK::UNIT_PX && wide ? W / PK::WIDE_PX : 0;
}

}  // namespace

// plane: n frames `stride` bytes apart, rows `pitch` bytes apart -> rgb [n][H][W][3].  Lane (f, y, item) converts one strip of row y.
template <class PK, bool MID>
__global__ __launch_bounds__(256) void packed_to_rgb_kernel(const uint8_t* __restrict__ plane, size_t pitch, size_t stride,
                                                            typename PK::T* __restrict__ rgb, int n, int H, int W, int wide, YuvCoef c) {
    constexpr int GP = PK::WIDE_PX, UP = PK::UNIT_PX;
    const int nw = wide_strips<PK>(W, wide), per = nw + (W - nw * GP) / UP;
    const size_t total = (size_t)n * H * per;
    for (size_t t = lane_index(); t < total; t += (size_t)gridDim.x * 256) {
        const int item = (int)(t % per);
        const size_t fy = t / per;
        const int y = (int)(fy % H);
        const size_t f = fy / H;
        const uint8_t* const prow = plane + f * stride + (size_t)y * pitch;
        typename PK::T* const rrow = rgb + (f * H + y) * (size_t)W * 3;
        if constexpr (GP > UP) {
            if (item < nw) {
                decode_strip<PK, MID, GP>(prow, rrow, item * GP, W, c);
                continue;
            }
        }
        decode_strip<PK, MID, UP>(prow, rrow, nw * GP + (item - nw) * UP, W, c);
    }
}

// rgb [n][H][W][3] -> plane.  Only the bytes of a row that hold samples are written.
template <class PK, bool MID>
__global__ __launch_bounds__(256) void rgb_to_packed_kernel(const typename PK::T* __restrict__ rgb, uint8_t* __restrict__ plane, size_t pitch,
                                                            size_t stride, int n, int H, int W, int wide, YuvCoef c) {
    constexpr int GP = PK::WIDE_PX, UP = PK::UNIT_PX;
    const int nw = wide_strips<PK>(W, wide), per = nw + (W - nw * GP) / UP;
    const size_t total = (size_t)n * H * per;
    for (size_t t = lane_index(); t < total; t += (size_t)gridDim.x * 256) {
        const int item = (int)(t % per);
        const size_t fy = t / per;
        const int y = (int)(fy % H);
        const size_t f = fy / H;
        uint8_t* const prow = plane + f * stride + (size_t)y * pitch;
        const typename PK::T* const rrow = rgb + (f * H + y) * (size_t)W * 3;
        if constexpr (GP > UP) {
            if (item < nw) {
                encode_strip<PK, MID, GP>(rrow, prow, item * GP, c);
                continue;
            }
        }
        encode_strip<PK, MID, UP>(rrow, prow, nw * GP + (item - nw) * UP, c);
    }
}

namespace {

int strip_blocks(size_t items) {
    const size_t blocks = (items + 255) / 256;
    return (int)(blocks < 8192 ? blocks : 8192);
}

// What both launchers check: the table's refusals, the pitch and the frame stride against the row, the packing's alignment.  *wide: rows
// and frames sit on 16 bytes, so the launch deals out strips of 16-byte words (and the row's tail by units)
bool plane_ok(const void* plane, size_t pitch, size_t stride, int pack, const void* rgb, int n, int H, int W, int siting, int* wide) {
    const size_t row = pack_row_bytes(pack, W);
    if (!plane || !rgb || n < 1 || H < 1 || !row || pitch < row || siting < 0 || siting > 2) return false;
    if (n > 1 && stride < (size_t)(H - 1) * pitch + row) return false;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(plane) | pitch | (n > 1 ? stride : 0);
    if (bits % PACK_TABLE[pack].align || reinterpret_cast<uintptr_t>(rgb) % (PACK_TABLE[pack].bits == 10 ? 2 : 1)) return false;
    *wide = bits % 16 == 0;
    return true;
}

template <class PK>
size_t strips(int n, int H, int W, int wide) {
    const int nw = PK::WIDE_PX > PK::UNIT_PX && wide ? W / PK::WIDE_PX : 0;
    return (size_t)n * H * (nw + (W - nw * PK::WIDE_PX) / PK::UNIT_PX);
}

template <class PK>
hipError_t decode_as(const void* plane, size_t pitch, size_t stride, void* rgb, const YuvCoef& c, int n, int H, int W, int siting, int wide,
                     hipStream_t s) {
    const dim3 grid(strip_blocks(strips<PK>(n, H, W, wide))), block(256);
    const uint8_t* const from = static_cast<const uint8_t*>(plane);
    typename PK::T* const to = static_cast<typename PK::T*>(rgb);
    if (PK::YUV && siting == 1)                                        // (yuv.py AXES: centre alone is midway across)
        hipLaunchKernelGGL((packed_to_rgb_kernel<PK, PK::YUV>), grid, block, 0, s, from, pitch, stride, to, n, H, W, wide, c);
    else
        hipLaunchKernelGGL((packed_to_rgb_kernel<PK, false>), grid, block, 0, s, from, pitch, stride, to, n, H, W, wide, c);
    return hipGetLastError();
}

template <class PK>
hipError_t encode_as(const void* rgb, void* plane, size_t pitch, size_t stride, const YuvCoef& c, int n, int H, int W, int siting, int wide,
                     hipStream_t s) {
    const dim3 grid(strip_blocks(strips<PK>(n, H, W, wide))), block(256);
    const typename PK::T* const from = static_cast<const typename PK::T*>(rgb);
    uint8_t* const to = static_cast<uint8_t*>(plane);
    if (PK::YUV && siting == 1)
        hipLaunchKernelGGL((rgb_to_packed_kernel<PK, PK::YUV>), grid, block, 0, s, from, to, pitch, stride, n, H, W, wide, c);
    else
        hipLaunchKernelGGL((rgb_to_packed_kernel<PK, false>), grid, block, 0, s, from, to, pitch, stride, n, H, W, wide, c);
    return hipGetLastError();
}

// CALL<the packing's trait>(...) for the runtime's packing
#define PFNL_PACK_DISPATCH(CALL, ...)                                  \
    switch (pack) {                                                    \
        case PFNL_PACK_BGR24: return CALL<PackBgr24>(__VA_ARGS__);     \
        case PFNL_PACK_RGBA: return CALL<PackRGBA>(__VA_ARGS__);       \
        case PFNL_PACK_BGRA: return CALL<PackBGRA>(__VA_ARGS__);       \
        case PFNL_PACK_YUYV: return CALL<PackYUYV>(__VA_ARGS__);       \
        case PFNL_PACK_UYVY: return CALL<PackUYVY>(__VA_ARGS__);       \
        case PFNL_PACK_X2RGB10: return CALL<PackX2RGB10>(__VA_ARGS__); \
        case PFNL_PACK_X2BGR10: return CALL<PackX2BGR10>(__VA_ARGS__); \
        case PFNL_PACK_Y210: return CALL<PackY210>(__VA_ARGS__);       \
        case PFNL_PACK_V210: return CALL<PackV210>(__VA_ARGS__);       \
        default: return hipErrorInvalidValue;                          \
    }

}  // namespace

hipError_t launch_packed_to_rgb(const void* plane, size_t pitch, size_t frame_stride, int pack, void* rgb, const YuvCoef& c, int n, int H, int W,
                                int siting, hipStream_t s) {
    int wide = 0;
    if (!plane_ok(plane, pitch, frame_stride, pack, rgb, n, H, W, siting, &wide)) return hipErrorInvalidValue;
    PFNL_PACK_DISPATCH(decode_as, plane, pitch, frame_stride, rgb, c, n, H, W, siting, wide, s)
}

hipError_t launch_rgb_to_packed(const void* rgb, void* plane, size_t pitch, size_t frame_stride, int pack, const YuvCoef& c, int n, int H, int W,
                                int siting, hipStream_t s) {
    int wide = 0;
    if (!plane_ok(plane, pitch, frame_stride, pack, rgb, n, H, W, siting, &wide)) return hipErrorInvalidValue;
    PFNL_PACK_DISPATCH(encode_as, rgb, plane, pitch, frame_stride, c, n, H, W, siting, wide, s)
}

#undef PFNL_PACK_DISPATCH

}  // namespace pfnl
