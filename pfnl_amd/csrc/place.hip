// The resampler at stage 1 of the streaming session's output route: the plain resize (pfnl_stream_resize) and a rectangle of the SR frame on
// a canvas - crop, letterbox and aspect fit - (include/pfnl_hip.h PLACEMENT, pfnl_stream_place), one kernel body for both and for both
// sample depths (sample_depth.h).  The rule is stated once on the host, pfnl_amd/resize.py resize and pfnl_amd/fit.py place (10 bits:
// pfnl_amd/depth10.py resize10, place10): the canvas is the fill colour, with the resize of the source rectangle alone written at the
// destination rectangle.  The tables are resize_plan(src.h, src.w, dst.h, dst.w) of resize.hip, and the kernel never evaluates the filter.
// One launch does both passes and writes every sample of the canvas once.  Across, the canvas is cut into tiles of RESIZE_TW pixels from
// its left edge, so that a tile's rows start on 16-byte boundaries wherever the canvas's do; down, the tiling is anchored at dst:
// ceil(dst.y / RESIZE_TH) tile rows of bar, then the tile rows of the resampled picture exactly as resize_plan walked them (its max_rows
// sizes the LDS), then the bar below.  A workgroup whose tile holds picture forms the horizontal pass of the input rows its vertical taps
// name - straight from the frame's samples, neighbouring lanes on neighbouring samples - into the int16 LDS tile of rows x TW x 3; taps
// index inside src: the first sample is at src.(y, x), the row stride is the raster's, and the columns of the tile outside dst are zero.
// It runs the vertical pass from there: a lane per 16 output bytes, read from LDS and stored as 16-byte words, where the destination's
// rows are 16-byte aligned; a lane per sample otherwise.  A sample outside dst is the fill colour instead, chosen per sample in
// registers, so a 16-byte word that straddles an edge of dst is still stored once.  A tile without picture reads no table and no input.
// A plan whose rectangles are the whole raster and the whole canvas runs the instantiation PLACED = false, which holds none of this
// rectangle logic: the per-element index work costs 16 % / 6 % on whole rectangles when it is left to run time.
// 8 bits keep 6 fractional bits in the intermediate and round 20 away, 10 bits keep 4 and round 18 away (Depth<T>); sum |c| <= 2^15 per
// table row keeps the intermediate inside int16 and the second sum inside int32 at either depth.
#include <string>

#include "sample_depth.h"
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

// the tables of resize_plan's blob on the device: hfirst [oW] | hcount [oW] | vfirst [oH] | vcount [oH] | hcoef | vcoef
void split_blob(const ResizePlan& r, const int32_t* blob_dev, PlaceArgs* a) {
    a->hfirst = blob_dev;
    a->hcount = blob_dev + r.oW;
    a->vfirst = blob_dev + 2 * (size_t)r.oW;
    a->vcount = blob_dev + 2 * (size_t)r.oW + r.oH;
    a->hcoef = reinterpret_cast<const int16_t*>(blob_dev + 2 * (size_t)r.oW + 2 * (size_t)r.oH);
    a->vcoef = a->hcoef + 2 * (((size_t)r.oW * r.ht + 1) / 2);
    a->ht = r.ht, a->vt = r.vt;
}

// the second pass's rounding and clip
template <typename T>
__device__ __forceinline__ unsigned round_clip(int v) {
    return (unsigned)shift_clip<Depth<T>::VS, Depth<T>::LEVELS>(v + (1 << (Depth<T>::VS - 1)));
}

}  // namespace

// in [n][sH][sW][3] -> out [n][cH][cW][3], samples of T; one tile of one frame per workgroup: grid (tiles across the canvas, tile rows,
// frames); LDS: the launch's rows x TW3 int16.  WORDS: a lane per 16 bytes of output, read from LDS and stored as one word; a lane per
// sample otherwise.  PLACED = false is the plain resize: src is the raster and dst the canvas, known when the kernel is compiled, so its
// code holds no rectangle - every tile is picture, all of it, and nothing is filled.
template <typename T, bool WORDS, bool PLACED>
__global__ __launch_bounds__(256) void resize_place_kernel(const T* __restrict__ in, T* __restrict__ out, PlaceArgs a) {
    extern __shared__ __attribute__((aligned(16))) int16_t hrow[];
    constexpr int PER = 16 / (int)sizeof(T);                           // samples per 16 bytes
    const int cx0 = blockIdx.x * RESIZE_TW, by = blockIdx.y;
    const int tw = a.cW - cx0 < RESIZE_TW ? a.cW - cx0 : RESIZE_TW;
    const int sy = PLACED ? a.sy : 0, sx = PLACED ? a.sx : 0, dx = PLACED ? a.dx : 0;
    // the tile's canvas rows cy0 .. cy0 + th - 1, of which picture rows py0 .. of dst; its columns inside dst: xa <= x < xb
    int cy0 = by * RESIZE_TH, end = a.cH, py0 = cy0, xa = 0, xb = tw;
    bool picture = true;
    if constexpr (PLACED) {                                            // bar above dst | picture | bar below
        py0 = -1;
        if (by < a.top) {
            end = a.dy;
        } else if (by < a.top + a.mid) {
            py0 = (by - a.top) * RESIZE_TH, cy0 = a.dy + py0, end = a.dy + a.dh;
        } else {
            cy0 = a.dy + a.dh + (by - a.top - a.mid) * RESIZE_TH;
        }
        xa = a.dx > cx0 ? a.dx - cx0 : 0, xb = a.dx + a.dw - cx0 < tw ? a.dx + a.dw - cx0 : tw;
        picture = py0 >= 0 && xa < xb;                                 // (the same for every lane of the workgroup)
    }
    const int th = end - cy0 < RESIZE_TH ? end - cy0 : RESIZE_TH;
    const int ea = picture ? 3 * xa : 0, eb = picture ? 3 * xb : 0;    // elements ea <= e < eb of a tile row (none where the tile holds no picture)
    T* const fout = out + (((size_t)blockIdx.z * a.cH + cy0) * a.cW + cx0) * 3;
    int lo = 0;

    if (picture) {
        // horizontal pass: element e = 3 x + c of row lo + r of src; the columns outside dst are zero (only words that straddle read them)
        lo = a.vfirst[py0];                                            // the tile's rows of src: lo .. lo + rows - 1 (the runs never move back)
        const int rows = a.vfirst[py0 + th - 1] + a.vcount[py0 + th - 1] - lo;
        const T* const fin = in + (((size_t)blockIdx.z * a.sH + sy + lo) * a.sW + sx) * 3;
        for (int i = threadIdx.x; i < rows * TW3; i += 256) {
            const int r = i / TW3, e = i - r * TW3, x = e / 3, c = e - 3 * x;
            int v = 0;
            if ((!PLACED || x >= xa) && x < xb) {
                const int ox = cx0 + x - dx, cnt = a.hcount[ox];
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
            int v[PER];
#pragma unroll
            for (int q = 0; q < PER; ++q) v[q] = 0;
            if (!PLACED || (e0 < eb && e0 + PER > ea)) {               // the word holds picture
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
                for (int q = 0; q < PER; ++q) v[q] = (int)round_clip<T>(acc[q]);
            }
            if constexpr (PLACED)
                if (e0 < ea || e0 + PER > eb) {                        // the word holds bar: the fill colour, rotated to its first channel
                    const int c0 = e0 % 3;
                    const unsigned fr[3] = {c0 == 0 ? a.f0 : (c0 == 1 ? a.f1 : a.f2), c0 == 0 ? a.f1 : (c0 == 1 ? a.f2 : a.f0),
                                            c0 == 0 ? a.f2 : (c0 == 1 ? a.f0 : a.f1)};
#pragma unroll
                    for (int q = 0; q < PER; ++q) {
                        const int e = e0 + q;
                        v[q] = e >= ea && e < eb ? v[q] : (int)fr[q % 3];
                    }
                }
            store_samples<T, PER, true>(fout + (size_t)y * a.cW * 3 + e0, v);
        }
    } else {
        const int samples = tw * 3;
        for (int i = threadIdx.x; i < th * samples; i += 256) {
            const int y = i / samples, e = i - y * samples;
            unsigned v;
            if (!PLACED || (e >= ea && e < eb)) {
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
            fout[y * a.cW * 3 + e] = (T)v;                             // (an int: y < RESIZE_TH, cW <= PLACE_MAX_SIZE)
        }
    }
}

namespace {

template <typename T>
hipError_t launch_place(const T* in, T* out, const PlacePlan& p, const int32_t* blob_dev, const T fill[3], int n, hipStream_t s) {
    const ResizePlan& r = p.r;
    if (!in || !out || !blob_dev || !fill || n < 1 || r.max_rows < 1 || p.cH < 1 || p.cW < 1) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % sizeof(T)) return hipErrorInvalidValue;
    if (fill[0] >= Depth<T>::LEVELS || fill[1] >= Depth<T>::LEVELS || fill[2] >= Depth<T>::LEVELS) return hipErrorInvalidValue;
    if (r.H != p.src.h || r.W != p.src.w || r.oH != p.dst.h || r.oW != p.dst.w || place_refused(p.sH, p.sW, p.cH, p.cW, p.src, p.dst))
        return hipErrorInvalidValue;                                   // (the tables are those of these rectangles, and they lie inside)
    const size_t lds = (size_t)r.max_rows * TW3 * sizeof(int16_t);
    if (lds > 65536) return hipErrorInvalidValue;
    PlaceArgs a;
    split_blob(r, blob_dev, &a);
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
        const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, lds, s, in + f0 * fin, out + f0 * fout, a); };
        if (p.whole)                                                   // the plain resize: the instantiation without rectangles
            words ? launch(resize_place_kernel<T, true, false>) : launch(resize_place_kernel<T, false, false>);
        else
            words ? launch(resize_place_kernel<T, true, true>) : launch(resize_place_kernel<T, false, true>);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_resize_place(const uint8_t* in, uint8_t* out, const PlacePlan& p, const int32_t* blob_dev, const uint8_t fill[3], int n,
                               hipStream_t s) {
    return launch_place<uint8_t>(in, out, p, blob_dev, fill, n, s);
}

hipError_t launch_resize_place(const uint16_t* in, uint16_t* out, const PlacePlan& p, const int32_t* blob_dev, const uint16_t fill[3], int n,
                               hipStream_t s) {
    return launch_place<uint16_t>(in, out, p, blob_dev, fill, n, s);
}

}  // namespace pfnl
