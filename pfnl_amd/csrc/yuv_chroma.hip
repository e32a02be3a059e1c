// YUV 4:2:2 / 4:4:4 <-> packed RGB (include/pfnl_hip.h CHROMA FORMAT): the decode of NV16 / I422 / NV24 / I444 or, with uint16 samples, of
// P210 / P410 / yuv422p10le / yuv444p10le, and the encode to them.  The 4:2:0 pair lives in yuv.hip and is not touched; the coefficient
// table, the sample primitives (sample_depth.h) and the plane descriptor (common.h YuvPlanes) are shared with it.  The arithmetic is integer
// and stated once on the host, pfnl_amd/yuv.py (10 bits: pfnl_amd/depth10.py) with chroma = "422" | "444": an axis that is not subsampled
// takes no filter, so at 4:2:2 only the horizontal half of a siting is read (co-sited: left and top left; midway: centre) and 4:4:4 is a
// conversion per pixel.
// There is no vertical coupling, so a lane owns ONE luma row by P pixels.  Both kernels move bytes - 2 (4:2:2) or 3 (4:4:4) samples per pixel
// on one side, 3 on the other.  8 bits: P = 16 reads and writes 16-byte words (8-byte ones for I422's half-width planes), P = 4 4-byte words
// (2-byte ones), then single bytes (P = 2 at 4:2:2, P = 1 at 4:4:4, which any W reaches).  10 bits: P = 8 in 16-byte words (I422's planes: 8),
// or single samples.  The form is read off the addresses.  Edges are index clamps inside the one kernel.
#include "sample_depth.h"

namespace pfnl {

namespace {

constexpr int C422 = PFNL_CHROMA_422, C444 = PFNL_CHROMA_444;

__device__ __forceinline__ size_t lane_index() { return (size_t)blockIdx.x * 256 + threadIdx.x; }

}  // namespace

// planes of n frames -> rgb [n][H][W][3].  Lane (f, y, g) converts the pixels g P .. g P + P - 1 of luma row y.  CH = 4:2:2: it reads the
// P/2 samples i0 .. i0 + P/2 - 1 of each chroma plane's row y and the one to their right (clamped onto the last); MID (chroma midway
// between two luma columns) reads the one to their left as well (clamped onto 0).  Co-sited: an even pixel takes its sample, an odd one
// the mean of it and the next, (a + b + 1) >> 1 - which is (2 a + 2 b + 2) >> 2.  Midway: (3 near + far + 2) >> 2, far = the sample to the
// left on even and to the right on odd pixels.  CH = 4:4:4: P samples per plane, each its pixel's.
template <typename T, int P, bool SEMI, int CH, bool MID>
__global__ __launch_bounds__(256) void yuv_row_to_rgb_kernel(YuvPlanes src, T* __restrict__ rgb, int n, int H, int W, YuvCoef c) {
    constexpr bool WORDS = P > 2, SUB = CH == C422;
    constexpr int LEVELS = Depth<T>::LEVELS, SH = sizeof(T) == 2 && SEMI ? 6 : 0;   // (P210 / P410: the value sits in the upper ten bits)
    constexpr int NC = SUB ? P / 2 : P, L = SUB && MID ? 1 : 0, R = SUB ? 1 : 0;    // chroma samples of the strip; read left, right of it
    static_assert(!MID || SUB, "4:4:4 has no siting");
    const auto row_of = [](const uint8_t* plane, size_t row, size_t pitch) { return reinterpret_cast<const T*>(plane + row * pitch); };
    const int gw = W / P, cw = SUB ? W >> 1 : W;
    const size_t total = (size_t)n * H * gw;
    for (size_t t = lane_index(); t < total; t += (size_t)gridDim.x * 256) {
        const int g = (int)(t % gw);
        const size_t fy = t / gw;
        const int y = (int)(fy % H);
        const size_t f = fy / H;
        const int x0 = g * P, i0 = SUB ? x0 >> 1 : x0;
        const int ie = i0 + NC < cw ? i0 + NC : cw - 1;                // (4:2:2 alone reads it)
        const int il = i0 > 0 ? i0 - 1 : 0;                            // (4:2:2 midway alone)
        int cb[L + NC + R], cr[L + NC + R];                            // [L + q]: sample i0 + q
        if constexpr (SEMI) {
            const T* const p = row_of(src.cb + f * src.frame, y, src.pitch_cb);   // Cb and Cr interleaved
            int pair[2 * NC], e[2];
#pragma unroll
            for (int k = 0; k < 2 * NC; k += P) load_values<T, P, WORDS, SH>(p + 2 * (size_t)i0 + k, pair + k);
#pragma unroll
            for (int q = 0; q < NC; ++q) cb[L + q] = pair[2 * q], cr[L + q] = pair[2 * q + 1];
            if constexpr (R) {
                load_values<T, 2, WORDS, SH>(p + 2 * (size_t)ie, e);
                cb[L + NC] = e[0], cr[L + NC] = e[1];
            }
            if constexpr (L) {
                load_values<T, 2, WORDS, SH>(p + 2 * (size_t)il, e);
                cb[0] = e[0], cr[0] = e[1];
            }
        } else {
            const T* const pb = row_of(src.cb + f * src.frame, y, src.pitch_cb);
            const T* const pr = row_of(src.cr + f * src.frame, y, src.pitch_cr);
            load_values<T, NC, WORDS>(pb + i0, cb + L);
            load_values<T, NC, WORDS>(pr + i0, cr + L);
            if constexpr (R) {
                load_values<T, 1, false>(pb + ie, &cb[L + NC]);
                load_values<T, 1, false>(pr + ie, &cr[L + NC]);
            }
            if constexpr (L) {
                load_values<T, 1, false>(pb + il, &cb[0]);
                load_values<T, 1, false>(pr + il, &cr[0]);
            }
        }
        int luma[P], out[3 * P];
        load_values<T, P, WORDS, SH>(row_of(src.y + f * src.frame, y, src.pitch_y) + x0, luma);
#pragma unroll
        for (int px = 0; px < P; ++px) {
            int u, v;
            if constexpr (!SUB) {
                u = cb[px], v = cr[px];
            } else if constexpr (MID) {                                // near sample [1 + q], far [q] | [2 + q]
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
        store_samples<T, 3 * P, WORDS>(rgb + ((f * H + y) * W + x0) * 3, out);
    }
}

// rgb [n][H][W][3] -> yuv [n][2 H W | 3 H W] samples of T, tightly packed: Y [H][W], then CbCr [H][cw][2] (SEMI; 16-bit samples << 6) or
// Cb [H][cw], Cr [H][cw]; cw = W / 2 at 4:2:2 and W at 4:4:4.  Lane (f, y, g) takes P pixels of row y: P luma samples and P/2 | P samples of
// each chroma plane from the unrounded numerators (yuv.py encode_filter along the one axis).  4:2:2 co-sited: 1-2-1 over the columns
// 2i - 1, 2i, 2i + 1 - only the column left of the strip is not its own, and at x = 0 it clamps onto column 0 - and 16 bits of shift; midway:
// the box over 2i, 2i + 1, 15 bits.  4:4:4: the numerator itself, 14 bits.
template <typename T, int P, bool SEMI, int CH, bool MID>
__global__ __launch_bounds__(256) void rgb_to_yuv_row_kernel(const T* __restrict__ rgb, T* __restrict__ yuv, int n, int H, int W, YuvCoef c) {
    constexpr bool WORDS = P > 2, SUB = CH == C422;
    constexpr int LEVELS = Depth<T>::LEVELS, SH = sizeof(T) == 2 && SEMI ? 6 : 0;
    constexpr int NC = SUB ? P / 2 : P, L = SUB && !MID ? 1 : 0;       // L: RGB columns read left of the strip
    constexpr int CS = 14 + (SUB ? (MID ? 1 : 2) : 0);                 // 14 + k (yuv.py downsample)
    static_assert(!MID || SUB, "4:4:4 has no siting");
    const int gw = W / P, cw = SUB ? W >> 1 : W;
    const size_t plane = (size_t)H * W, cplane = (size_t)H * cw, total = (size_t)n * H * gw;
    for (size_t t = lane_index(); t < total; t += (size_t)gridDim.x * 256) {
        const int g = (int)(t % gw);
        const size_t fy = t / gw;
        const int y = (int)(fy % H);
        const size_t f = fy / H;
        T* const fr = yuv + f * (plane + 2 * cplane);
        const int x0 = g * P, i0 = SUB ? x0 >> 1 : x0;
        const T* const row = rgb + (f * H + y) * (size_t)W * 3;
        int px[3 * (P + L)], luma[P], nb[P + L], nr[P + L];            // [L + p]: column x0 + p
        if constexpr (L) {
            const size_t xl = x0 > 0 ? x0 - 1 : 0;
            px[0] = row[3 * xl], px[1] = row[3 * xl + 1], px[2] = row[3 * xl + 2];
        }
        load_samples<T, 3 * P, WORDS>(row + (size_t)x0 * 3, px + 3 * L);
#pragma unroll
        for (int p = 0; p < P + L; ++p) {
            const int r = px[3 * p], gg = px[3 * p + 1], b = px[3 * p + 2];
            nb[p] = c.cbr * r + c.cbg * gg + c.cbb * b;
            nr[p] = c.crr * r + c.crg * gg + c.crb * b;
            if (p >= L) luma[p - L] = shift_clip<14, LEVELS>(c.yr * r + c.yg * gg + c.yb * b + (c.y0 << 14) + (1 << 13));
        }
        store_samples<T, P, WORDS, SH>(fr + (size_t)y * W + x0, luma);
        constexpr int BIAS = (1 << (CS - 1)) + (Depth<T>::CHROMA << CS);   // the rounding and the chroma offset + (S' >> CS)
        int ob[NC], orr[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            if constexpr (!SUB) {
                ob[q] = shift_clip<CS, LEVELS>(nb[q] + BIAS);
                orr[q] = shift_clip<CS, LEVELS>(nr[q] + BIAS);
            } else if constexpr (MID) {
                ob[q] = shift_clip<CS, LEVELS>(nb[2 * q] + nb[2 * q + 1] + BIAS);
                orr[q] = shift_clip<CS, LEVELS>(nr[2 * q] + nr[2 * q + 1] + BIAS);
            } else {
                ob[q] = shift_clip<CS, LEVELS>(nb[2 * q] + 2 * nb[2 * q + 1] + nb[2 * q + 2] + BIAS);
                orr[q] = shift_clip<CS, LEVELS>(nr[2 * q] + 2 * nr[2 * q + 1] + nr[2 * q + 2] + BIAS);
            }
        }
        if constexpr (SEMI) {
            int pair[2 * NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) pair[2 * q] = ob[q], pair[2 * q + 1] = orr[q];
            T* const to = fr + plane + ((size_t)y * cw + i0) * 2;
#pragma unroll
            for (int k = 0; k < 2 * NC; k += P) store_samples<T, P, WORDS, SH>(to + k, pair + k);
        } else {
            T* const pb = fr + plane + (size_t)y * cw + i0;
            store_samples<T, NC, WORDS>(pb, ob);
            store_samples<T, NC, WORDS>(pb + cplane, orr);
        }
    }
}

namespace {

int row_blocks(size_t items) {
    const size_t blocks = (items + 255) / 256;
    return (int)(blocks < 8192 ? blocks : 8192);
}

bool size_ok(int chroma, int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1) return false;
    return chroma == C444 || (chroma == C422 && W >= 2 && !(W & 1));
}

// The strip width of either kernel from what its words need.  `full`: every address bit of what is read or written in words as wide as the
// luma strip - pointers, pitches, frame strides; `half`: the same for I422's chroma planes, whose words are half as wide (0 where there
// are none).  8 bits: 16-byte words, 4-byte words, then single samples; 16 bits: 8 pixels in 16-byte words, or single samples.
template <typename T>
int strip_of(uintptr_t full, uintptr_t half, int chroma, int W) {
    const int single = chroma == C422 ? 2 : 1;
    if constexpr (sizeof(T) == 1) {
        if (W % 16 == 0 && full % 16 == 0 && half % 8 == 0) return 16;
        if (W % 4 == 0 && full % 4 == 0 && half % 2 == 0) return 4;
        return single;
    } else {
        return W % 8 == 0 && full % 16 == 0 && half % 8 == 0 ? 8 : single;
    }
}

// KERNEL<T, P, semiplanar, chroma, midway> for the runtime's P, layout, subsampling and horizontal siting
#define PFNL_ROW_LAUNCH_P(KERNEL, P4, P1, ...)                                                                     \
    if (chroma == C422) {                                                                                          \
        if (semi && mid) hipLaunchKernelGGL((KERNEL<T, P4, true, C422, true>), grid, block, 0, s, __VA_ARGS__);     \
        else if (semi) hipLaunchKernelGGL((KERNEL<T, P4, true, C422, false>), grid, block, 0, s, __VA_ARGS__);      \
        else if (mid) hipLaunchKernelGGL((KERNEL<T, P4, false, C422, true>), grid, block, 0, s, __VA_ARGS__);       \
        else hipLaunchKernelGGL((KERNEL<T, P4, false, C422, false>), grid, block, 0, s, __VA_ARGS__);               \
    } else {                                                                                                       \
        if (semi) hipLaunchKernelGGL((KERNEL<T, P1, true, C444, false>), grid, block, 0, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL((KERNEL<T, P1, false, C444, false>), grid, block, 0, s, __VA_ARGS__);               \
    }
#define PFNL_ROW_LAUNCH(KERNEL, ...)                                                                               \
    if constexpr (sizeof(T) == 1) {                                                                                \
        if (P == 16) {                                                                                             \
            PFNL_ROW_LAUNCH_P(KERNEL, 16, 16, __VA_ARGS__)                                                         \
        } else if (P == 4) {                                                                                       \
            PFNL_ROW_LAUNCH_P(KERNEL, 4, 4, __VA_ARGS__)                                                           \
        } else {                                                                                                   \
            PFNL_ROW_LAUNCH_P(KERNEL, 2, 1, __VA_ARGS__)                                                           \
        }                                                                                                          \
    } else {                                                                                                       \
        if (P == 8) {                                                                                              \
            PFNL_ROW_LAUNCH_P(KERNEL, 8, 8, __VA_ARGS__)                                                           \
        } else {                                                                                                   \
            PFNL_ROW_LAUNCH_P(KERNEL, 2, 1, __VA_ARGS__)                                                           \
        }                                                                                                          \
    }

template <typename T>
hipError_t launch_decode(const YuvPlanes& src, T* rgb, bool semi, const YuvCoef& c, int n, int H, int W, int chroma, int siting, hipStream_t s) {
    if (!src.y || !src.cb || (!semi && !src.cr) || !rgb || !size_ok(chroma, n, H, W) || siting < 0 || siting > 2) return hipErrorInvalidValue;
    const size_t row = (size_t)W * sizeof(T), crow = chroma == C422 ? row / 2 : row;   // bytes of a luma row, of a row of one chroma plane
    if (src.pitch_y < row || src.pitch_cb < (semi ? 2 * crow : crow) || (!semi && src.pitch_cr < crow)) return hipErrorInvalidValue;
    const auto bits = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
    const uintptr_t chroma_bits = semi ? bits(src.cb) | src.pitch_cb : bits(src.cb) | bits(src.cr) | src.pitch_cb | src.pitch_cr;
    const bool narrow = !semi && chroma == C422;                       // planes of half the width: words half as wide
    const uintptr_t full = bits(src.y) | src.pitch_y | src.frame | bits(rgb) | (narrow ? 0 : chroma_bits), half = narrow ? chroma_bits : 0;
    if ((full | half) % sizeof(T)) return hipErrorInvalidValue;        // no 16-bit sample sits at an odd address
    const int P = strip_of<T>(full, half, chroma, W);
    const bool mid = chroma == C422 && siting == 1;                    // (yuv.py AXES: centre alone is midway across)
    const dim3 grid(row_blocks((size_t)n * H * (W / P))), block(256);
    PFNL_ROW_LAUNCH(yuv_row_to_rgb_kernel, src, rgb, n, H, W, c)
    return hipGetLastError();
}

template <typename T>
hipError_t launch_decode_packed(const T* yuv, T* rgb, bool semi, const YuvCoef& c, int n, int H, int W, int chroma, int siting, hipStream_t s) {
    if (!yuv || !size_ok(chroma, n, H, W)) return hipErrorInvalidValue;
    const size_t row = (size_t)W * sizeof(T), plane = (size_t)H * row, crow = chroma == C422 ? row / 2 : row, cplane = (size_t)H * crow;
    const uint8_t* const at = reinterpret_cast<const uint8_t*>(yuv);
    const YuvPlanes src{at, at + plane, semi ? nullptr : at + plane + cplane, row, semi ? 2 * crow : crow, semi ? 0 : crow, plane + 2 * cplane};
    return launch_decode<T>(src, rgb, semi, c, n, H, W, chroma, siting, s);
}

template <typename T>
hipError_t launch_encode(const T* rgb, T* yuv, bool semi, const YuvCoef& c, int n, int H, int W, int chroma, int siting, hipStream_t s) {
    const uintptr_t align = reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(yuv);
    if (!rgb || !yuv || !size_ok(chroma, n, H, W) || align % sizeof(T) || siting < 0 || siting > 2) return hipErrorInvalidValue;
    // W % P == 0 puts every row of every plane, every strip in it and every frame on the boundary its words need: rows of W, W / 2 (words
    // half as wide) or 2 W samples behind planes of H W, H W / 2 samples
    const int P = strip_of<T>(align, 0, chroma, W);
    const bool mid = chroma == C422 && siting == 1;
    const dim3 grid(row_blocks((size_t)n * H * (W / P))), block(256);
    PFNL_ROW_LAUNCH(rgb_to_yuv_row_kernel, rgb, yuv, n, H, W, c)
    return hipGetLastError();
}

#undef PFNL_ROW_LAUNCH
#undef PFNL_ROW_LAUNCH_P

}  // namespace

hipError_t launch_yuv_planes_to_rgb_chroma(const YuvPlanes& src, uint8_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma,
                                           int siting, hipStream_t s) {
    return launch_decode<uint8_t>(src, rgb, semiplanar, c, n, H, W, chroma, siting, s);
}

hipError_t launch_yuv_planes_to_rgb_chroma(const YuvPlanes& src, uint16_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma,
                                           int siting, hipStream_t s) {
    return launch_decode<uint16_t>(src, rgb, semiplanar, c, n, H, W, chroma, siting, s);
}

hipError_t launch_yuv_to_rgb_chroma(const uint8_t* yuv, uint8_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s) {
    return launch_decode_packed<uint8_t>(yuv, rgb, semiplanar, c, n, H, W, chroma, siting, s);
}

hipError_t launch_yuv_to_rgb_chroma(const uint16_t* yuv, uint16_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s) {
    return launch_decode_packed<uint16_t>(yuv, rgb, semiplanar, c, n, H, W, chroma, siting, s);
}

hipError_t launch_rgb_to_yuv_chroma(const uint8_t* rgb, uint8_t* yuv, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s) {
    return launch_encode<uint8_t>(rgb, yuv, semiplanar, c, n, H, W, chroma, siting, s);
}

hipError_t launch_rgb_to_yuv_chroma(const uint16_t* rgb, uint16_t* yuv, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s) {
    return launch_encode<uint16_t>(rgb, yuv, semiplanar, c, n, H, W, chroma, siting, s);
}

}  // namespace pfnl
