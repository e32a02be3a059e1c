// A rectangle of the SR frame on a canvas: crop, letterbox and aspect fit at stage 1 of the streaming session's output route
// (include/pfnl_hip.h PLACEMENT, pfnl_stream_place).  The rule is stated once on the host, pfnl_amd/fit.py place (10 bits:
// pfnl_amd/depth10.py place10): the canvas is the fill colour, with the resize of resize.hip / depth10.hip of the source rectangle alone
// written at the destination rectangle.  The tables are resize_plan(src.h, src.w, dst.h, dst.w), unchanged, and so is the fixed point.
// One launch writes every sample of the canvas once.  Across, the canvas is cut into tiles of RESIZE_TW pixels from its left edge, so that
// a tile's rows start on 16-byte boundaries wherever the canvas's do; down, the tiling is anchored at dst: ceil(dst.y / RESIZE_TH) tile
// rows of bar, then the tile rows of the resampled picture exactly as resize_plan walked them (its max_rows sizes the LDS), then the bar
// below.  A workgroup whose tile holds picture forms the horizontal pass of the input rows its vertical taps name into the int16 LDS tile -
// taps index inside src: the first sample is at src.(y, x), the row stride is the raster's, and the columns of the tile outside dst are
// zero - and runs the vertical pass from there; a sample outside dst is the fill colour instead, chosen per sample in registers, so a
// 16-byte word that straddles an edge of dst is still stored once.  A tile without picture reads no table and no input.
// The two depths share the body: 8 bits keep 6 fractional bits in the intermediate and round 20 away, 10 bits keep 4 and round 18 away.
#include <string>

#include "common.h"
#include "stream_route.h"

namespace pfnl {

static_assert(PLACE_MAX_SIZE == RESIZE_MAX_SIZE, "place_refused and resize_axis hold one limit");

bool place_plan(int sH, int sW, int cH, int cW, const pfnl_rect* src, const pfnl_rect* dst, PlacePlan* p, std::string* why) {
    PlacePlan q;
    q.sH = sH, q.sW = sW, q.cH = cH, q.cW = cW;
    q.src = src ? *src : pfnl_rect{0, 0, sH, sW};
    q.dst = dst ? *dst : pfnl_rect{0, 0, cH, cW};
    if (src || dst)                                                    // (neither: a plain resize, and resize_plan's own words)
        if (const char* no = place_refused(sH, sW, cH, cW, q.src, q.dst)) {
            *why = no;
            return false;
        }
    if (!resize_plan(q.src.h, q.src.w, q.dst.h, q.dst.w, &q.r, why)) return false;
    q.whole = q.src.y == 0 && q.src.x == 0 && q.src.h == sH && q.src.w == sW && q.dst.y == 0 && q.dst.x == 0 && q.dst.h == cH && q.dst.w == cW;
    *p = std::move(q);
    return true;
}

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int TW3 = RESIZE_TW * 3;                                     // int16 per row of the intermediate tile

struct PlaceArgs {
    const int32_t *hfirst, *hcount, *vfirst, *vcount;                  // of src.w -> dst.w and src.h -> dst.h
    const int16_t *hcoef, *vcoef;
    int ht, vt;
    int sH, sW, cH, cW;                                                // the raster; the canvas
    int sy, sx;                                                        // src's corner (its size is in the tables)
    int dy, dx, dh, dw;                                                // dst
    int top, mid;                                                      // tile rows above dst; of dst
    unsigned f0, f1, f2;                                               // the fill colour, in sample values
};

template <typename T>
struct Depth;
template <>
struct Depth<uint8_t> {
    static constexpr int HS = 8, VS = 20, LEVELS = 256;                // (+2^7) >> 8, then clip((+2^19) >> 20, 0, 255)
};
template <>
struct Depth<uint16_t> {
    static constexpr int HS = 10, VS = 18, LEVELS = 1024;              // (+2^9) >> 10, then clip((+2^17) >> 18, 0, 1023)
};

// the second pass's rounding and clip, the clamp ahead of the shift (round_clip_u8 of resize.hip, shift_clip_u10 of depth10.hip)
template <typename T>
__device__ __forceinline__ unsigned round_clip(int v) {
    constexpr int S = Depth<T>::VS, TOP = (Depth<T>::LEVELS << S) - 1;
    v += 1 << (S - 1);
    v = v < 0 ? 0 : v;
    v = v > TOP ? TOP : v;
    return (unsigned)(v >> S);
}

// one tile of one frame: grid (tiles across the canvas, tile rows, frames); hrow: the launch's rows x TW3 int16
template <typename T, bool WORDS>
__device__ __forceinline__ void place_tile(const T* __restrict__ in, T* __restrict__ out, const PlaceArgs& a, int16_t* hrow) {
    constexpr int PER = 16 / (int)sizeof(T), SPW = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);   // samples per 16 bytes, per 4; bits of one
    const int cx0 = blockIdx.x * RESIZE_TW, by = blockIdx.y;
    const int tw = a.cW - cx0 < RESIZE_TW ? a.cW - cx0 : RESIZE_TW;
    // the tile's canvas rows cy0 .. cy0 + th - 1: bar above dst | picture rows py0 .. of dst | bar below
    int cy0, end, py0 = -1;
    if (by < a.top) {
        cy0 = by * RESIZE_TH, end = a.dy;
    } else if (by < a.top + a.mid) {
        py0 = (by - a.top) * RESIZE_TH, cy0 = a.dy + py0, end = a.dy + a.dh;
    } else {
        cy0 = a.dy + a.dh + (by - a.top - a.mid) * RESIZE_TH, end = a.cH;
    }
    const int th = end - cy0 < RESIZE_TH ? end - cy0 : RESIZE_TH;
    // the tile's columns inside dst: xa <= x < xb, elements ea <= e < eb of a tile row (none where the tile holds no picture)
    const int xa = a.dx > cx0 ? a.dx - cx0 : 0, xb = a.dx + a.dw - cx0 < tw ? a.dx + a.dw - cx0 : tw;
    const bool picture = py0 >= 0 && xa < xb;                          // (the same for every lane of the workgroup)
    const int ea = picture ? 3 * xa : 0, eb = picture ? 3 * xb : 0;
    T* const fout = out + (((size_t)blockIdx.z * a.cH + cy0) * a.cW + cx0) * 3;
    int lo = 0;

    if (picture) {
        // horizontal pass: element e = 3 x + c of row lo + r of src; the columns outside dst are zero (only words that straddle read them)
        lo = a.vfirst[py0];                                            // the tile's rows of src: lo .. lo + rows - 1 (the runs never move back)
        const int rows = a.vfirst[py0 + th - 1] + a.vcount[py0 + th - 1] - lo;
        const T* const fin = in + (((size_t)blockIdx.z * a.sH + a.sy + lo) * a.sW + a.sx) * 3;
        for (int i = threadIdx.x; i < rows * TW3; i += 256) {
            const int r = i / TW3, e = i - r * TW3, x = e / 3, c = e - 3 * x;
            int v = 0;
            if (x >= xa && x < xb) {
                const int ox = cx0 + x - a.dx, cnt = a.hcount[ox];
                const int16_t* const cf = a.hcoef + (size_t)ox * a.ht;
                const T* const p = fin + ((size_t)r * a.sW + a.hfirst[ox]) * 3 + c;
                int acc = 1 << (Depth<T>::HS - 1);
                for (int k = 0; k < cnt; ++k) acc += (int)cf[k] * (int)p[3 * k];
                v = acc >> Depth<T>::HS;
            }
            hrow[i] = (int16_t)v;
        }
        __syncthreads();
    }

    // vertical pass, or the fill colour: element e of a tile row has channel e % 3 (a tile starts on a pixel)
    if constexpr (WORDS) {
        const int groups = tw * 3 / PER;                               // exact: cW is a multiple of PER, cx0 of 64
        for (int i = threadIdx.x; i < th * groups; i += 256) {
            const int y = i / groups, g = i - y * groups, e0 = PER * g;
            unsigned v[PER];
#pragma unroll
            for (int q = 0; q < PER; ++q) v[q] = 0;
            if (e0 < eb && e0 + PER > ea) {                            // the word holds picture
                const int oy = py0 + y, cnt = a.vcount[oy];
                const int16_t* const cf = a.vcoef + (size_t)oy * a.vt;
                const int16_t* src = hrow + (a.vfirst[oy] - lo) * TW3 + e0;
                int acc[PER];
#pragma unroll
                for (int q = 0; q < PER; ++q) acc[q] = 0;
                for (int k = 0; k < cnt; ++k, src += TW3) {
                    const int c = cf[k];
#pragma unroll
                    for (int h = 0; h < PER / 8; ++h) {
                        const u32x4 w4 = *reinterpret_cast<const u32x4*>(src + 8 * h);
                        const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            acc[8 * h + 2 * j] += c * (int)(int16_t)(w[j] & 0xffffu);
                            acc[8 * h + 2 * j + 1] += c * ((int)w[j] >> 16);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < PER; ++q) v[q] = round_clip<T>(acc[q]);
            }
            if (e0 < ea || e0 + PER > eb) {                            // the word holds bar: the fill colour, rotated to its first channel
                const int c0 = e0 % 3;
                const unsigned fr[3] = {c0 == 0 ? a.f0 : (c0 == 1 ? a.f1 : a.f2), c0 == 0 ? a.f1 : (c0 == 1 ? a.f2 : a.f0),
                                        c0 == 0 ? a.f2 : (c0 == 1 ? a.f0 : a.f1)};
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const int e = e0 + q;
                    v[q] = e >= ea && e < eb ? v[q] : fr[q % 3];
                }
            }
            unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < PER; ++q) o[q / SPW] |= v[q] << (BITS * (q % SPW));
            *reinterpret_cast<u32x4*>(fout + (size_t)y * a.cW * 3 + e0) = u32x4{o[0], o[1], o[2], o[3]};
        }
    } else {
        const int samples = tw * 3;
        for (int i = threadIdx.x; i < th * samples; i += 256) {
            const int y = i / samples, e = i - y * samples;
            unsigned v;
            if (e >= ea && e < eb) {
                const int oy = py0 + y, cnt = a.vcount[oy];
                const int16_t* const cf = a.vcoef + (size_t)oy * a.vt;
                const int16_t* src = hrow + (a.vfirst[oy] - lo) * TW3 + e;
                int acc = 0;
                for (int k = 0; k < cnt; ++k, src += TW3) acc += (int)cf[k] * (int)*src;
                v = round_clip<T>(acc);
            } else {
                const int c = e % 3;
                v = c == 0 ? a.f0 : (c == 1 ? a.f1 : a.f2);
            }
            fout[(size_t)y * a.cW * 3 + e] = (T)v;
        }
    }
}

}  // namespace

// in [n][sH][sW][3] -> out [n][cH][cW][3] uint8; LDS: the launch's rows x TW3 int16
template <bool WORDS>
__global__ __launch_bounds__(256) void resize_place_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, PlaceArgs a) {
    extern __shared__ __attribute__((aligned(16))) int16_t place_rows[];
    place_tile<uint8_t, WORDS>(in, out, a, place_rows);
}

// the same on uint16 samples 0 .. 1023
template <bool WORDS>
__global__ __launch_bounds__(256) void resize_place_u10_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, PlaceArgs a) {
    extern __shared__ __attribute__((aligned(16))) int16_t place_rows[];
    place_tile<uint16_t, WORDS>(in, out, a, place_rows);
}

namespace {

template <typename T>
hipError_t launch_place(const T* in, T* out, const PlacePlan& p, const int32_t* blob_dev, const T fill[3], int n, hipStream_t s) {
    const ResizePlan& r = p.r;
    if (!in || !out || !blob_dev || !fill || n < 1 || r.max_rows < 1 || p.cH < 1 || p.cW < 1) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % sizeof(T)) return hipErrorInvalidValue;
    if (r.H != p.src.h || r.W != p.src.w || r.oH != p.dst.h || r.oW != p.dst.w || place_refused(p.sH, p.sW, p.cH, p.cW, p.src, p.dst))
        return hipErrorInvalidValue;                                   // (the tables are those of these rectangles, and they lie inside)
    const size_t lds = (size_t)r.max_rows * TW3 * sizeof(int16_t);
    if (lds > 65536) return hipErrorInvalidValue;
    PlaceArgs a;
    a.hfirst = blob_dev;
    a.hcount = blob_dev + r.oW;
    a.vfirst = blob_dev + 2 * (size_t)r.oW;
    a.vcount = blob_dev + 2 * (size_t)r.oW + r.oH;
    a.hcoef = reinterpret_cast<const int16_t*>(blob_dev + 2 * (size_t)r.oW + 2 * (size_t)r.oH);
    a.vcoef = a.hcoef + 2 * (((size_t)r.oW * r.ht + 1) / 2);
    a.ht = r.ht, a.vt = r.vt;
    a.sH = p.sH, a.sW = p.sW, a.cH = p.cH, a.cW = p.cW;
    a.sy = p.src.y, a.sx = p.src.x;
    a.dy = p.dst.y, a.dx = p.dst.x, a.dh = p.dst.h, a.dw = p.dst.w;
    const auto tiles = [](int rows) { return (rows + RESIZE_TH - 1) / RESIZE_TH; };
    a.top = tiles(a.dy), a.mid = tiles(a.dh);
    a.f0 = fill[0], a.f1 = fill[1], a.f2 = fill[2];
    // 16 bytes of samples: a canvas row, a tile's 64 * 3 samples and its last tw * 3 divide into such words where cW is a multiple of 16 / 8,
    // and every word of every row and frame is then 16-byte aligned with the destination
    const bool words = p.cW % (16 / (int)sizeof(T)) == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const size_t fin = (size_t)p.sH * p.sW * 3, fout = (size_t)p.cH * p.cW * 3;
    for (int f0 = 0; f0 < n; f0 += 65535) {                            // (the grid's z)
        const int nf = n - f0 < 65535 ? n - f0 : 65535;
        const dim3 grid((p.cW + RESIZE_TW - 1) / RESIZE_TW, a.top + a.mid + tiles(a.cH - a.dy - a.dh), nf), block(256);
        if constexpr (sizeof(T) == 1) {
            if (words)
                hipLaunchKernelGGL(resize_place_u8_kernel<true>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, a);
            else
                hipLaunchKernelGGL(resize_place_u8_kernel<false>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, a);
        } else {
            if (words)
                hipLaunchKernelGGL(resize_place_u10_kernel<true>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, a);
            else
                hipLaunchKernelGGL(resize_place_u10_kernel<false>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, a);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_resize_place_u8(const uint8_t* in, uint8_t* out, const PlacePlan& p, const int32_t* blob_dev, const uint8_t fill[3], int n,
                                  hipStream_t s) {
    return launch_place<uint8_t>(in, out, p, blob_dev, fill, n, s);
}

hipError_t launch_resize_place_u10(const uint16_t* in, uint16_t* out, const PlacePlan& p, const int32_t* blob_dev, const uint16_t fill[3], int n,
                                   hipStream_t s) {
    if (fill && (fill[0] > 1023 || fill[1] > 1023 || fill[2] > 1023)) return hipErrorInvalidValue;
    return launch_place<uint16_t>(in, out, p, blob_dev, fill, n, s);
}

}  // namespace pfnl
