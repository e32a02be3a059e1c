// YUV 4:2:0 <-> packed RGB: the two edges of the streaming session (include/pfnl_hip.h, pfnl_stream_format, pfnl_stream_input_depth) - the
// decode of NV12 / I420 or, with uint16 samples, P010 / I010 input, and the encode to NV12 / I420 or, with uint16 samples 0 .. 1023, to
// P010 / I010.  The arithmetic is integer and stated once on the
// host, pfnl_amd/yuv.py (10 bits: pfnl_amd/depth10.py): 14 fractional bits, coefficients rounded once, chroma sited left (on the even luma
// columns, midway between two luma rows) unless the caller names another siting - centre or top left (include/pfnl_hip.h SITING), a template
// parameter of both kernels; the kernels give its samples.
// Both kernels move bytes - 1.5 samples per pixel on one side, 3 on the other.  A lane owns a strip of two luma rows by P pixels, so that the
// chroma samples it reads (or forms) serve both rows.  8 bits: P = 16 reads and writes 16-byte words (8-byte ones for I420's half-width
// planes), P = 4 4-byte words (2-byte ones), P = 2 single bytes; 10 bits: P = 8 reads three 16-byte words per row and writes one per luma
// row and one of interleaved chroma (I010's half-width planes take 8 bytes each), P = 2 single samples.  So any even H, W and any pointer
// a sample can sit at (the decode mirrors it: one 16-byte word of luma per row and one of interleaved chroma in, three of RGB per row out).
// Edges are index clamps inside the one kernel.  Each kernel is one body over the sample type (sample_depth.h); the decode takes a caller's
// 16-bit samples as values10 does (depth10.py): P010 >> 6, anything else clamped onto 1023.
// The decode reads its planes by pointer and row pitch, so a decoder's surface (include/pfnl_hip.h SURFACES) and a packed frame are one kernel.
#include <cmath>

#include "sample_depth.h"

namespace pfnl {

bool yuv_coefficients(int bits, int matrix, int full_range, YuvCoef* c) {
    if (!c || (bits != 8 && bits != 10) || matrix < 0 || matrix > 1 || full_range < 0 || full_range > 1) return false;
    const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double top = (double)((1 << bits) - 1);                      // 219 / 255, 224 / 255 | 876 / 1023, 896 / 1023
    const double ys = full_range ? 1.0 : (219 << (bits - 8)) / top, cs = full_range ? 1.0 : (224 << (bits - 8)) / top;
    const auto rnd = [](double x) { return (int)std::floor(x * 16384.0 + 0.5); };
    *c = YuvCoef{};
    c->y0 = full_range ? 0 : 16 << (bits - 8);
    c->yr = rnd(ys * kr);
    c->yb = rnd(ys * kb);
    c->yg = rnd(ys) - c->yr - c->yb;
    c->cbr = rnd(-cs * kr / (2.0 * (1.0 - kb)));
    c->cbb = rnd(cs / 2.0);
    c->cbg = -c->cbr - c->cbb;
    c->crr = rnd(cs / 2.0);
    c->crb = rnd(-cs * kb / (2.0 * (1.0 - kr)));
    c->crg = -c->crr - c->crb;
    c->dy = rnd(1.0 / ys);
    c->drv = rnd(2.0 * (1.0 - kr) / cs);
    c->dbu = rnd(2.0 * (1.0 - kb) / cs);
    c->dgu = rnd(-2.0 * kb * (1.0 - kb) / (kg * cs));
    c->dgv = rnd(-2.0 * kr * (1.0 - kr) / (kg * cs));
    return true;
}

// planes of n frames -> rgb [n][H][W][3].  A frame is its planes by pointer and row pitch (common.h YuvPlanes): W, and W / 2 for I420's
// chroma, in a tightly packed frame, whatever the decoder chose in a surface; frame f lies f * src.frame bytes behind the first.
// Strip k of 0 .. H/2 is the luma rows 2k - 1 and 2k: exactly the two rows that lie between the
// chroma rows k - 1 and k, each three quarters its near row and one quarter the other (yuv.py upsample); row -1 and row H do not exist,
// and there the missing chroma row clamps onto the present one.  Per row and plane a lane reads P/2 samples and the one to their right.
// S is the chroma siting (include/pfnl_hip.h SITING; yuv.py AXES).  S = 0, left, is the body above.  S = 1, centre: the same strips, and
// horizontally the 3 : 1 rule as well - an even pixel's far sample is the one to its LEFT, so a lane also reads the sample left of its
// strip (clamped at 0): P/2 + 2 per row and plane.  S = 2, top left: chroma row k lies ON luma row 2k, so strip k of 0 .. H/2 - 1 is the
// rows 2k (row k alone) and 2k + 1 (half row k, half row min(k + 1, H/2 - 1)); horizontally as left.
template <typename T, int P, bool NV12, int S>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(YuvPlanes src, T* __restrict__ rgb, int n, int H, int W, YuvCoef c) {
    constexpr bool WORDS = P > 2;
    constexpr int LEVELS = Depth<T>::LEVELS, SH = sizeof(T) == 2 && NV12 ? 6 : 0;   // (P010: the value sits in the upper ten bits)
    const auto row_of = [](const uint8_t* plane, size_t row, size_t pitch) { return reinterpret_cast<const T*>(plane + row * pitch); };
    constexpr int HP = P / 2, L = S == 1 ? 1 : 0;                      // L: samples read left of the strip
    const int gw = W / P, strips = S == 2 ? H / 2 : H / 2 + 1, hh = H >> 1, hw = W >> 1;
    const size_t total = (size_t)n * strips * gw;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int g = (int)(t % gw);
        const size_t fk = t / gw;
        const int k = (int)(fk % strips);
        const size_t f = fk / strips;
        const uint8_t* __restrict__ const fy = src.y + f * src.frame;
        const uint8_t* __restrict__ const fb = src.cb + f * src.frame;   // (NV12: Cb and Cr interleaved)
        const int x0 = g * P, i0 = x0 >> 1;
        const int ie = i0 + HP < hw ? i0 + HP : hw - 1;
        const int il = i0 > 0 ? i0 - 1 : 0;                            // (S = 1 alone reads it)
        const int jrow[2] = {S == 2 ? k : (k > 0 ? k - 1 : 0), S == 2 ? (k + 1 < hh ? k + 1 : hh - 1) : (k < hh ? k : hh - 1)};
        int cb[2][HP + 1 + L], cr[2][HP + 1 + L];                      // [L + q]: sample i0 + q; [0] of S = 1: sample il
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if constexpr (NV12) {
                const T* const p = row_of(fb, jrow[a], src.pitch_cb);
                int pair[P], e[2];
                load_values<T, P, WORDS, SH>(p + x0, pair);
                load_values<T, 2, WORDS, SH>(p + 2 * ie, e);
#pragma unroll
                for (int q = 0; q < HP; ++q) cb[a][L + q] = pair[2 * q], cr[a][L + q] = pair[2 * q + 1];
                cb[a][L + HP] = e[0], cr[a][L + HP] = e[1];
                if constexpr (L) {
                    load_values<T, 2, WORDS, SH>(p + 2 * il, e);
                    cb[a][0] = e[0], cr[a][0] = e[1];
                }
            } else {
                const T* const pb = row_of(fb, jrow[a], src.pitch_cb);
                const T* const pr = row_of(src.cr + f * src.frame, jrow[a], src.pitch_cr);
                load_values<T, HP, WORDS>(pb + i0, cb[a] + L);
                load_values<T, HP, WORDS>(pr + i0, cr[a] + L);
                load_values<T, 1, false>(pb + ie, &cb[a][L + HP]);
                load_values<T, 1, false>(pr + ie, &cr[a][L + HP]);
                if constexpr (L) {
                    load_values<T, 1, false>(pb + il, &cb[a][0]);
                    load_values<T, 1, false>(pr + il, &cr[a][0]);
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {                                  // a = 0: row 2k - 1, near chroma row k - 1; a = 1: row 2k, near row k
            const int y = S == 2 ? 2 * k + a : 2 * k - 1 + a;          // (S = 2: row 2k + a, on chroma row k | between rows k and k + 1)
            if (y < 0 || y >= H) continue;
            int luma[P], out[3 * P];
            load_values<T, P, WORDS, SH>(row_of(fy, y, src.pitch_y) + x0, luma);
#pragma unroll
            for (int px = 0; px < P; ++px) {
                const int q = px >> 1;
                int u, v;
                if constexpr (S == 0) {
                    if (px & 1) {
                        u = (3 * cb[a][q] + cb[1 - a][q] + 3 * cb[a][q + 1] + cb[1 - a][q + 1] + 4) >> 3;
                        v = (3 * cr[a][q] + cr[1 - a][q] + 3 * cr[a][q + 1] + cr[1 - a][q + 1] + 4) >> 3;
                    } else {
                        u = (6 * cb[a][q] + 2 * cb[1 - a][q] + 4) >> 3;
                        v = (6 * cr[a][q] + 2 * cr[1 - a][q] + 4) >> 3;
                    }
                } else if constexpr (S == 1) {                         // 3 : 1 on both axes: near sample [q + 1], far [q + 2] | [q]
                    const int far = px & 1 ? q + 2 : q;
                    u = (3 * (3 * cb[a][q + 1] + cb[a][far]) + 3 * cb[1 - a][q + 1] + cb[1 - a][far] + 8) >> 4;
                    v = (3 * (3 * cr[a][q + 1] + cr[a][far]) + 3 * cr[1 - a][q + 1] + cr[1 - a][far] + 8) >> 4;
                } else {                                               // both axes: the sample itself | the mean of it and the next
                    const int e = px & 1 ? q + 1 : q;
                    if (a) {
                        u = (cb[0][q] + cb[1][q] + cb[0][e] + cb[1][e] + 2) >> 2;
                        v = (cr[0][q] + cr[1][q] + cr[0][e] + cr[1][e] + 2) >> 2;
                    } else {
                        u = (cb[0][q] + cb[0][e] + 1) >> 1;
                        v = (cr[0][q] + cr[0][e] + 1) >> 1;
                    }
                }
                u -= Depth<T>::CHROMA, v -= Depth<T>::CHROMA;
                const int yy = c.dy * (luma[px] - c.y0) + (1 << 13);
                out[3 * px] = shift_clip<14, LEVELS>(yy + c.drv * v);
                out[3 * px + 1] = shift_clip<14, LEVELS>(yy + c.dgu * u + c.dgv * v);
                out[3 * px + 2] = shift_clip<14, LEVELS>(yy + c.dbu * u);
            }
            store_samples<T, 3 * P, WORDS>(rgb + ((f * H + y) * W + x0) * 3, out);
        }
    }
}

// rgb [n][H][W][3] -> yuv [n][H*W*3/2] samples of T: NV12 / P010 (SEMIPLANAR; P010's samples << 6) or I420 / I010.  A lane takes the luma
// rows 2j, 2j + 1 by P pixels: 2 P luma samples and P/2 samples of each chroma plane - the unrounded numerators of both rows added per
// column, then 1-2-1 across columns 2i - 1, 2i, 2i + 1 (yuv.py downsample, depth10.py downsample10).  Only the column left of the strip is
// not its own (2i + 1 <= W - 1 always); at x = 0 it clamps onto column 0.
// S is the chroma siting (yuv.py encode_filter).  S = 0, left, is the body above: weights that sum to 8, 17 bits of shift.  S = 1, centre:
// the box over the strip's own 2 x 2 pixels, no neighbour column, 16 bits.  S = 2, top left: 1-2-1 over the rows 2j - 1, 2j, 2j + 1 as well -
// the lane reads row 2j - 1 (row 0 where j = 0) for its chroma numerators only, the luma of that row belongs to the strip above - 18 bits.
template <typename T, int P, bool SEMIPLANAR, int S>
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const T* __restrict__ rgb, T* __restrict__ yuv, int n, int H, int W, YuvCoef c) {
    constexpr bool WORDS = P > 2;
    constexpr int HP = P / 2, LEVELS = Depth<T>::LEVELS, SH = sizeof(T) == 2 && SEMIPLANAR ? 6 : 0;
    constexpr int A0 = S == 2 ? -1 : 0, P0 = S == 1 ? 1 : 0;           // the first row read, relative to 2j; the first column used of [0 .. P]
    constexpr int CS = S == 0 ? 17 : (S == 1 ? 16 : 18);               // 14 + k (yuv.py downsample)
    const int gw = W / P, hh = H >> 1, hw = W >> 1;
    const size_t plane = (size_t)H * W, total = (size_t)n * hh * gw;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int g = (int)(t % gw);
        const size_t fj = t / gw;
        const int j = (int)(fj % hh);
        const size_t f = fj / hh;
        T* const fr = yuv + f * (plane + plane / 2);
        const int x0 = g * P, xl = x0 > 0 ? x0 - 1 : 0;
        int nb[P + 1], nr[P + 1];                                      // per column, both rows: [0] the column left of the strip
#pragma unroll
        for (int a = A0; a < 2; ++a) {
            const int y = S == 2 && 2 * j + a < 0 ? 0 : 2 * j + a;
            const T* const row = rgb + (f * H + y) * (size_t)W * 3;
            int px[3 * P + 3], luma[P];
            if constexpr (S != 1) px[0] = row[3 * (size_t)xl], px[1] = row[3 * (size_t)xl + 1], px[2] = row[3 * (size_t)xl + 2];
            load_samples<T, 3 * P, WORDS>(row + (size_t)x0 * 3, px + 3);
#pragma unroll
            for (int p = P0; p <= P; ++p) {
                const int r = px[3 * p], gg = px[3 * p + 1], b = px[3 * p + 2];
                int vb = c.cbr * r + c.cbg * gg + c.cbb * b, vr = c.crr * r + c.crg * gg + c.crb * b;
                if constexpr (S == 2)
                    if (a == 0) vb *= 2, vr *= 2;                      // (1-2-1 down the rows as well)
                nb[p] = a > A0 ? nb[p] + vb : vb;
                nr[p] = a > A0 ? nr[p] + vr : vr;
                if (p && a >= 0) luma[p - 1] = shift_clip<14, LEVELS>(c.yr * r + c.yg * gg + c.yb * b + (c.y0 << 14) + (1 << 13));
            }
            if (a >= 0) store_samples<T, P, WORDS, SH>(fr + (size_t)y * W + x0, luma);
        }
        int ob[HP], orr[HP];
#pragma unroll
        for (int q = 0; q < HP; ++q) {                                 // the chroma offset + (S' >> 17 | 16 | 18)
            if constexpr (S == 1) {
                ob[q] = shift_clip<CS, LEVELS>(nb[2 * q + 1] + nb[2 * q + 2] + (1 << (CS - 1)) + (Depth<T>::CHROMA << CS));
                orr[q] = shift_clip<CS, LEVELS>(nr[2 * q + 1] + nr[2 * q + 2] + (1 << (CS - 1)) + (Depth<T>::CHROMA << CS));
            } else {
                ob[q] = shift_clip<CS, LEVELS>(nb[2 * q] + 2 * nb[2 * q + 1] + nb[2 * q + 2] + (1 << (CS - 1)) + (Depth<T>::CHROMA << CS));
                orr[q] = shift_clip<CS, LEVELS>(nr[2 * q] + 2 * nr[2 * q + 1] + nr[2 * q + 2] + (1 << (CS - 1)) + (Depth<T>::CHROMA << CS));
            }
        }
        if constexpr (SEMIPLANAR) {
            int pair[P];
#pragma unroll
            for (int q = 0; q < HP; ++q) pair[2 * q] = ob[q], pair[2 * q + 1] = orr[q];
            store_samples<T, P, WORDS, SH>(fr + plane + (size_t)j * W + x0, pair);
        } else {
            T* const pb = fr + plane + (size_t)j * hw + (x0 >> 1);
            store_samples<T, HP, WORDS, SH>(pb, ob);
            store_samples<T, HP, WORDS, SH>(pb + (size_t)hh * hw, orr);
        }
    }
}

namespace {

// The strip width the encode runs with.  8 bits: 16-byte words, 4-byte words, bytes.  10 bits: W % 8 == 0 puts every row of every plane,
// every strip of 8 pixels in it and every frame on a 16-byte boundary (I010's chroma: 8); single samples otherwise.
template <typename T>
int strip_width(uintptr_t align, int W) {
    if constexpr (sizeof(T) == 1)
        return W % 16 == 0 && align % 16 == 0 ? 16 : (W % 4 == 0 && align % 4 == 0 ? 4 : 2);
    else
        return W % 8 == 0 && align % 16 == 0 ? 8 : 2;
}

int strip_blocks(size_t items) {
    const size_t blocks = (items + 255) / 256;
    return (int)(blocks < 8192 ? blocks : 8192);
}

bool yuv_geometry_ok(const void* a, const void* b, int n, int H, int W) { return a && b && n >= 1 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1); }

// The strip width the decode runs with.  Every word is read or written at plane + row * pitch (+ f * frame) + a multiple of its size, so
// the planes, their pitches, the frame stride and rgb (rows of 3 W samples) all have to be multiples of it: 16 | 4 for the full-width planes
// and rgb, half of that for I420's / I010's chroma planes, whose words are half as wide.  A tightly packed frame gives what strip_width
// gives.  16-bit samples: 8 pixels in 16-byte words, or single samples; 0: a plane or a pitch that no 16-bit sample can sit at.
template <typename T>
int decode_strip_width(const YuvPlanes& p, const void* rgb, bool nv12, int W) {
    const auto bits = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
    const uintptr_t full = bits(p.y) | p.pitch_y | p.frame | bits(rgb) | (nv12 ? bits(p.cb) | p.pitch_cb : 0);
    const uintptr_t half = nv12 ? 0 : bits(p.cb) | bits(p.cr) | p.pitch_cb | p.pitch_cr;
    if constexpr (sizeof(T) == 1) {
        if (W % 16 == 0 && full % 16 == 0 && half % 8 == 0) return 16;
        if (W % 4 == 0 && full % 4 == 0 && half % 2 == 0) return 4;
        return 2;
    } else {
        if ((full | half) % 2) return 0;
        return W % 8 == 0 && full % 16 == 0 && half % 8 == 0 ? 8 : 2;
    }
}

template <typename T>
hipError_t launch_decode(const YuvPlanes& src, T* rgb, bool nv12, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s) {
    if (!yuv_geometry_ok(src.y, rgb, n, H, W) || !src.cb || (!nv12 && !src.cr) || siting < 0 || siting > 2) return hipErrorInvalidValue;
    const size_t row = (size_t)W * sizeof(T);                          // bytes of a luma row
    if (src.pitch_y < row || src.pitch_cb < (nv12 ? row : row / 2) || (!nv12 && src.pitch_cr < row / 2)) return hipErrorInvalidValue;
    const int P = decode_strip_width<T>(src, rgb, nv12, W);
    if (!P) return hipErrorInvalidValue;
    const dim3 grid(strip_blocks((size_t)n * (siting == 2 ? H / 2 : H / 2 + 1) * (W / P))), block(256);
#define PFNL_YUV_LAUNCH_S(P_, S_)                                                                                  \
    if (nv12)                                                                                                      \
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<T, P_, true, S_>), grid, block, 0, s, src, rgb, n, H, W, c);      \
    else                                                                                                           \
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<T, P_, false, S_>), grid, block, 0, s, src, rgb, n, H, W, c)
#define PFNL_YUV_LAUNCH(P_)                                                                                        \
    if (siting == 0) {                                                                                             \
        PFNL_YUV_LAUNCH_S(P_, 0);                                                                                  \
    } else if (siting == 1) {                                                                                      \
        PFNL_YUV_LAUNCH_S(P_, 1);                                                                                  \
    } else {                                                                                                       \
        PFNL_YUV_LAUNCH_S(P_, 2);                                                                                  \
    }
    if constexpr (sizeof(T) == 1) {
        if (P == 16) {
            PFNL_YUV_LAUNCH(16);
        } else if (P == 4) {
            PFNL_YUV_LAUNCH(4);
        } else {
            PFNL_YUV_LAUNCH(2);
        }
    } else {
        if (P == 8) {
            PFNL_YUV_LAUNCH(8);
        } else {
            PFNL_YUV_LAUNCH(2);
        }
    }
#undef PFNL_YUV_LAUNCH
#undef PFNL_YUV_LAUNCH_S
    return hipGetLastError();
}

// the packed frames as planes: the same kernel, the same strip width as ever
template <typename T>
hipError_t launch_decode_packed(const T* yuv, T* rgb, bool nv12, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s) {
    if (!yuv_geometry_ok(yuv, rgb, n, H, W)) return hipErrorInvalidValue;
    const size_t plane = (size_t)H * W * sizeof(T), row = (size_t)W * sizeof(T);
    const uint8_t* const at = reinterpret_cast<const uint8_t*>(yuv);
    const YuvPlanes src{at, at + plane, nv12 ? nullptr : at + plane + plane / 4, row, nv12 ? row : row / 2, nv12 ? 0 : row / 2, plane + plane / 2};
    return launch_decode<T>(src, rgb, nv12, c, n, H, W, siting, s);
}

}  // namespace

hipError_t launch_yuv420_planes_to_rgb_u8(const YuvPlanes& src, uint8_t* rgb, bool nv12, const YuvCoef& c, int n, int H, int W, int siting,
                                          hipStream_t s) {
    return launch_decode<uint8_t>(src, rgb, nv12, c, n, H, W, siting, s);
}

hipError_t launch_yuv420_planes_to_rgb_u10(const YuvPlanes& src, uint16_t* rgb, bool p010, const YuvCoef& c, int n, int H, int W, int siting,
                                           hipStream_t s) {
    return launch_decode<uint16_t>(src, rgb, p010, c, n, H, W, siting, s);
}

hipError_t launch_yuv420_to_rgb_u8(const uint8_t* yuv, uint8_t* rgb, bool nv12, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s) {
    return launch_decode_packed<uint8_t>(yuv, rgb, nv12, c, n, H, W, siting, s);
}

hipError_t launch_yuv420_to_rgb(const uint16_t* yuv, uint16_t* rgb, bool p010, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s) {
    return launch_decode_packed<uint16_t>(yuv, rgb, p010, c, n, H, W, siting, s);
}

namespace {

template <typename T>
hipError_t launch_encode(const T* rgb, T* yuv, bool semiplanar, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s) {
    const uintptr_t align = reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(yuv);
    if (!yuv_geometry_ok(rgb, yuv, n, H, W) || align % sizeof(T) || siting < 0 || siting > 2) return hipErrorInvalidValue;
    const int P = strip_width<T>(align, W);
    const dim3 grid(strip_blocks((size_t)n * (H / 2) * (W / P))), block(256);
#define PFNL_YUV_LAUNCH_S(P_, S_)                                                                                  \
    if (semiplanar)                                                                                                \
        hipLaunchKernelGGL((rgb_to_yuv420_kernel<T, P_, true, S_>), grid, block, 0, s, rgb, yuv, n, H, W, c);      \
    else                                                                                                           \
        hipLaunchKernelGGL((rgb_to_yuv420_kernel<T, P_, false, S_>), grid, block, 0, s, rgb, yuv, n, H, W, c)
#define PFNL_YUV_LAUNCH(P_)                                                                                        \
    if (siting == 0) {                                                                                             \
        PFNL_YUV_LAUNCH_S(P_, 0);                                                                                  \
    } else if (siting == 1) {                                                                                      \
        PFNL_YUV_LAUNCH_S(P_, 1);                                                                                  \
    } else {                                                                                                       \
        PFNL_YUV_LAUNCH_S(P_, 2);                                                                                  \
    }
    if constexpr (sizeof(T) == 1) {
        if (P == 16) {
            PFNL_YUV_LAUNCH(16);
        } else if (P == 4) {
            PFNL_YUV_LAUNCH(4);
        } else {
            PFNL_YUV_LAUNCH(2);
        }
    } else {
        if (P == 8) {
            PFNL_YUV_LAUNCH(8);
        } else {
            PFNL_YUV_LAUNCH(2);
        }
    }
#undef PFNL_YUV_LAUNCH
#undef PFNL_YUV_LAUNCH_S
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rgb_to_yuv420(const uint8_t* rgb, uint8_t* yuv, bool nv12, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s) {
    return launch_encode<uint8_t>(rgb, yuv, nv12, c, n, H, W, siting, s);
}

hipError_t launch_rgb_to_yuv420(const uint16_t* rgb, uint16_t* yuv, bool p010, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s) {
    return launch_encode<uint16_t>(rgb, yuv, p010, c, n, H, W, siting, s);
}

}  // namespace pfnl
