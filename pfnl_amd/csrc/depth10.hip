// SR frames at 10 bits: the streaming session's output edge with uint16 samples (include/pfnl_hip.h, pfnl_stream_format with PFNL_PIX_RGB10 /
// PFNL_PIX_P010 / PFNL_PIX_I010) - quantisation of the fp32 result to 0 .. 1023, resampling, RGB -> YUV 4:2:0.  The three are the 8-bit
// kernels (quantise_u8_kernel, resize.hip, yuv.hip) with the wider sample; the arithmetic is stated once on the host, pfnl_amd/depth10.py,
// and the kernels give its samples.  The tap tables are resize.hip's (resize_plan and its device blob, unchanged): only the split of the
// fixed point differs, 4 fractional bits in the int16 intermediate and 18 in the second sum.
// All three move bytes.  A lane of the conversion owns two luma rows by P pixels: P = 8 reads three 16-byte words per row and writes one per
// luma row and one of interleaved chroma (P010; I010's half-width planes take 8 bytes each), P = 2 single samples - any even H, W and any
// pointer a uint16 can sit at.  Edges are index clamps inside the one kernel.
#include <cmath>

#include "common.h"

namespace pfnl {

bool yuv10_coefficients(int matrix, int full_range, YuvCoef* c) {
    if (!c || matrix < 0 || matrix > 1 || full_range < 0 || full_range > 1) return false;
    const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722;
    const double ys = full_range ? 1.0 : 876.0 / 1023.0, cs = full_range ? 1.0 : 896.0 / 1023.0;
    const auto rnd = [](double x) { return (int)std::floor(x * 16384.0 + 0.5); };
    *c = YuvCoef{};                                                    // (no decode side: 10-bit input is not built)
    c->y0 = full_range ? 0 : 64;
    c->yr = rnd(ys * kr);
    c->yb = rnd(ys * kb);
    c->yg = rnd(ys) - c->yr - c->yb;
    c->cbr = rnd(-cs * kr / (2.0 * (1.0 - kb)));
    c->cbb = rnd(cs / 2.0);
    c->cbg = -c->cbr - c->cbb;
    c->crr = rnd(cs / 2.0);
    c->crb = rnd(-cs * kb / (2.0 * (1.0 - kr)));
    c->crg = -c->crr - c->crb;
    return true;
}

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// clip(v >> S, 0, 1023) with the clamp AHEAD of the shift (the same value: both are monotonic), as shift_clip_u8 of yuv.hip and for its
// reason: written as shift-then-clamp, results that are packed into one word invite the packed shift-and-clamp instructions of gfx950,
// which this compiler has assembled into wrong words (tools/GFX950_NOTES.md)
template <int S>
__device__ __forceinline__ int shift_clip_u10(int v) {
    v = v < 0 ? 0 : v;
    v = v > (1024 << S) - 1 ? (1024 << S) - 1 : v;
    return v >> S;
}

// the widest word, in bytes, that divides N samples: the strips are laid out so that a run of N samples is aligned to it in the wide form
template <int N>
constexpr int word_of() {
    return (2 * N) % 16 == 0 ? 16 : ((2 * N) % 8 == 0 ? 8 : ((2 * N) % 4 == 0 ? 4 : 2));
}

// N samples at p -> v[0 .. N), in words (WORDS) or sample by sample
template <int N, bool WORDS>
__device__ __forceinline__ void load_samples(const uint16_t* __restrict__ p, int* v) {
    constexpr int WB = WORDS ? word_of<N>() : 2;
    if constexpr (WB == 2) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = p[k];
    } else {
        unsigned w[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; k += WB / 4) {
            if constexpr (WB == 16) {
                const u32x4 q = *reinterpret_cast<const u32x4*>(p + 2 * k);
                w[k] = q.x, w[k + 1] = q.y, w[k + 2] = q.z, w[k + 3] = q.w;
            } else if constexpr (WB == 8) {
                const u32x2 q = *reinterpret_cast<const u32x2*>(p + 2 * k);
                w[k] = q.x, w[k + 1] = q.y;
            } else {
                w[k] = *reinterpret_cast<const unsigned*>(p + 2 * k);
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = (int)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    }
}

// v[0 .. N), each in [0, 1023] -> N samples at p, each v << SH (P010 keeps its values in the upper ten bits: the shift is part of the store)
template <int N, bool WORDS, int SH>
__device__ __forceinline__ void store_samples(uint16_t* __restrict__ p, const int* v) {
    constexpr int WB = WORDS ? word_of<N>() : 2;
    if constexpr (WB == 2) {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = (uint16_t)(v[k] << SH);
    } else {
        unsigned w[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) w[k] = ((unsigned)v[2 * k] << SH) | ((unsigned)v[2 * k + 1] << (16 + SH));
#pragma unroll
        for (int k = 0; k < N / 2; k += WB / 4) {
            if constexpr (WB == 16)
                *reinterpret_cast<u32x4*>(p + 2 * k) = u32x4{w[k], w[k + 1], w[k + 2], w[k + 3]};
            else if constexpr (WB == 8)
                *reinterpret_cast<u32x2*>(p + 2 * k) = u32x2{w[k], w[k + 1]};
            else
                *reinterpret_cast<unsigned*>(p + 2 * k) = w[k];
        }
    }
}

}  // namespace

// uint16(np.round(np.clip(sr * 1023, 0, 1023))): the float32 product; rintf = round half to even, like np.round; NaN -> 0 (fmaxf)
__global__ __launch_bounds__(256) void quantise_u10_kernel(const f32x4* __restrict__ sr, u32x2* __restrict__ out, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 v = sr[i];
        const uint32_t a = (uint32_t)rintf(fminf(fmaxf(v.x * 1023.0f, 0.f), 1023.f));
        const uint32_t b = (uint32_t)rintf(fminf(fmaxf(v.y * 1023.0f, 0.f), 1023.f));
        const uint32_t c = (uint32_t)rintf(fminf(fmaxf(v.z * 1023.0f, 0.f), 1023.f));
        const uint32_t d = (uint32_t)rintf(fminf(fmaxf(v.w * 1023.0f, 0.f), 1023.f));
        out[i] = u32x2{a | (b << 16), c | (d << 16)};
    }
}

hipError_t launch_quantise_u10(const float* sr, uint16_t* out, size_t n, hipStream_t s) {
    if (!sr || !out || !n || n % 4 || reinterpret_cast<uintptr_t>(sr) % 16 || reinterpret_cast<uintptr_t>(out) % 8) return hipErrorInvalidValue;
    const size_t n4 = n / 4;
    const int blocks = (int)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
    hipLaunchKernelGGL(quantise_u10_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const f32x4*>(sr), reinterpret_cast<u32x2*>(out), n4);
    return hipGetLastError();
}

// rgb [n][H][W][3] (values 0 .. 1023) -> yuv [n][H*W*3/2], P010 (SEMIPLANAR, samples << 6) or I010.  A lane takes the luma rows 2j, 2j + 1
// by P pixels: 2 P luma samples and P/2 samples of each chroma plane - the unrounded numerators of both rows added per column, then 1-2-1
// across columns 2i - 1, 2i, 2i + 1 (depth10.py downsample10).  Only the column left of the strip is not its own (2i + 1 <= W - 1 always);
// at x = 0 it clamps onto column 0.
template <int P, bool SEMIPLANAR>
__global__ __launch_bounds__(256) void rgb_to_yuv420_u10_kernel(const uint16_t* __restrict__ rgb, uint16_t* __restrict__ yuv, int n, int H,
                                                                int W, YuvCoef c) {
    constexpr bool WORDS = P > 2;
    constexpr int HP = P / 2, SH = SEMIPLANAR ? 6 : 0;
    const int gw = W / P, hh = H >> 1, hw = W >> 1;
    const size_t plane = (size_t)H * W, total = (size_t)n * hh * gw;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int g = (int)(t % gw);
        const size_t fj = t / gw;
        const int j = (int)(fj % hh);
        const size_t f = fj / hh;
        uint16_t* const fr = yuv + f * (plane + plane / 2);
        const int x0 = g * P, xl = x0 > 0 ? x0 - 1 : 0;
        int nb[P + 1], nr[P + 1];                                      // per column, both rows: [0] the column left of the strip
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int y = 2 * j + a;
            const uint16_t* const row = rgb + (f * H + y) * (size_t)W * 3;
            int px[3 * P + 3], luma[P];
            px[0] = row[3 * (size_t)xl], px[1] = row[3 * (size_t)xl + 1], px[2] = row[3 * (size_t)xl + 2];
            load_samples<3 * P, WORDS>(row + (size_t)x0 * 3, px + 3);
#pragma unroll
            for (int p = 0; p <= P; ++p) {
                const int r = px[3 * p], gg = px[3 * p + 1], b = px[3 * p + 2];
                const int vb = c.cbr * r + c.cbg * gg + c.cbb * b, vr = c.crr * r + c.crg * gg + c.crb * b;
                nb[p] = a ? nb[p] + vb : vb;
                nr[p] = a ? nr[p] + vr : vr;
                if (p) luma[p - 1] = shift_clip_u10<14>(c.yr * r + c.yg * gg + c.yb * b + (c.y0 << 14) + (1 << 13));
            }
            store_samples<P, WORDS, SH>(fr + (size_t)y * W + x0, luma);
        }
        int ob[HP], orr[HP];
#pragma unroll
        for (int q = 0; q < HP; ++q) {
            ob[q] = shift_clip_u10<17>(nb[2 * q] + 2 * nb[2 * q + 1] + nb[2 * q + 2] + (1 << 16) + (512 << 17));   // 512 + (S' >> 17)
            orr[q] = shift_clip_u10<17>(nr[2 * q] + 2 * nr[2 * q + 1] + nr[2 * q + 2] + (1 << 16) + (512 << 17));
        }
        if constexpr (SEMIPLANAR) {
            int pair[P];
#pragma unroll
            for (int q = 0; q < HP; ++q) pair[2 * q] = ob[q], pair[2 * q + 1] = orr[q];
            store_samples<P, WORDS, SH>(fr + plane + (size_t)j * W + x0, pair);
        } else {
            uint16_t* const pb = fr + plane + (size_t)j * hw + (x0 >> 1);
            store_samples<HP, WORDS, SH>(pb, ob);
            store_samples<HP, WORDS, SH>(pb + (size_t)hh * hw, orr);
        }
    }
}

hipError_t launch_rgb_to_yuv420_u10(const uint16_t* rgb, uint16_t* yuv, bool p010, const YuvCoef& c, int n, int H, int W, hipStream_t s) {
    const uintptr_t align = reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(yuv);
    if (!rgb || !yuv || n < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || align % 2) return hipErrorInvalidValue;
    // W % 8 == 0 puts every row of every plane, every strip of 8 pixels in it and every frame on a 16-byte boundary (I010's chroma: 8)
    const int P = W % 8 == 0 && align % 16 == 0 ? 8 : 2;
    const size_t blocks = ((size_t)n * (H / 2) * (W / P) + 255) / 256;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192)), block(256);
    if (P == 8) {
        if (p010)
            hipLaunchKernelGGL((rgb_to_yuv420_u10_kernel<8, true>), grid, block, 0, s, rgb, yuv, n, H, W, c);
        else
            hipLaunchKernelGGL((rgb_to_yuv420_u10_kernel<8, false>), grid, block, 0, s, rgb, yuv, n, H, W, c);
    } else {
        if (p010)
            hipLaunchKernelGGL((rgb_to_yuv420_u10_kernel<2, true>), grid, block, 0, s, rgb, yuv, n, H, W, c);
        else
            hipLaunchKernelGGL((rgb_to_yuv420_u10_kernel<2, false>), grid, block, 0, s, rgb, yuv, n, H, W, c);
    }
    return hipGetLastError();
}

namespace {

constexpr int TW3 = RESIZE_TW * 3;                                     // int16 per row of the intermediate tile

struct Resize10Tables {
    const int32_t *hfirst, *hcount, *vfirst, *vcount;
    const int16_t *hcoef, *vcoef;
    int ht, vt;
};

// clip((v + 2^17) >> 18, 0, 1023), the clamp ahead of the shift (shift_clip_u10)
__device__ __forceinline__ unsigned round_clip_u10(int v) { return (unsigned)shift_clip_u10<18>(v + (1 << 17)); }

}  // namespace

// in [n][H][W][3] -> out [n][oH][oW][3], values 0 .. 1023; grid (tiles across, tiles down, frames); LDS: the launch's rows x TW3 int16.
// resize_u8_kernel with 2-byte samples: the horizontal pass keeps 4 fractional bits (|h| <= 1023 * 2^15 >> 10 fits int16), the vertical
// pass rounds 18 away (|sum| <= 32736 * 2^15 < 2^31).  WORDS: a lane per 8 output samples, read from LDS and stored as one 16-byte word.
template <bool WORDS>
__global__ __launch_bounds__(256) void resize_u10_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, Resize10Tables t, int H,
                                                         int W, int oH, int oW) {
    extern __shared__ __attribute__((aligned(16))) int16_t hrow10[];
    const int ox0 = blockIdx.x * RESIZE_TW, oy0 = blockIdx.y * RESIZE_TH;
    const int tw = oW - ox0 < RESIZE_TW ? oW - ox0 : RESIZE_TW, th = oH - oy0 < RESIZE_TH ? oH - oy0 : RESIZE_TH;
    const int lo = t.vfirst[oy0];                                      // the tile's input rows: lo .. lo + rows - 1 (the runs never move back)
    const int rows = t.vfirst[oy0 + th - 1] + t.vcount[oy0 + th - 1] - lo;
    const uint16_t* const fin = in + (size_t)blockIdx.z * H * W * 3;
    uint16_t* const fout = out + ((size_t)blockIdx.z * oH * oW + ox0) * 3;

    // horizontal pass: element e = 3 x + c of input row lo + r; the columns right of the frame are zero (nothing reads them)
    for (int i = threadIdx.x; i < rows * TW3; i += 256) {
        const int r = i / TW3, e = i - r * TW3, x = e / 3, c = e - 3 * x;
        int v = 0;
        if (x < tw) {
            const int ox = ox0 + x, cnt = t.hcount[ox];
            const int16_t* const cf = t.hcoef + (size_t)ox * t.ht;
            const uint16_t* const p = fin + ((size_t)(lo + r) * W + t.hfirst[ox]) * 3 + c;
            int acc = 1 << 9;
            for (int k = 0; k < cnt; ++k) acc += (int)cf[k] * (int)p[3 * k];
            v = acc >> 10;
        }
        hrow10[i] = (int16_t)v;
    }
    __syncthreads();

    // vertical pass
    if constexpr (WORDS) {
        const int groups = tw * 3 / 8;                                 // exact: oW is a multiple of 8, ox0 of 64
        for (int i = threadIdx.x; i < th * groups; i += 256) {
            const int y = i / groups, g = i - y * groups, oy = oy0 + y, cnt = t.vcount[oy];
            const int16_t* const cf = t.vcoef + (size_t)oy * t.vt;
            const int16_t* src = hrow10 + (t.vfirst[oy] - lo) * TW3 + 8 * g;
            int acc[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = 0;
            for (int k = 0; k < cnt; ++k, src += TW3) {
                const int c = cf[k];
                const u32x4 a = *reinterpret_cast<const u32x4*>(src);
                const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[2 * q] += c * (int)(int16_t)(w[q] & 0xffffu);
                    acc[2 * q + 1] += c * ((int)w[q] >> 16);
                }
            }
            unsigned o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = round_clip_u10(acc[2 * q]) | (round_clip_u10(acc[2 * q + 1]) << 16);
            *reinterpret_cast<u32x4*>(fout + (size_t)oy * oW * 3 + 8 * g) = u32x4{o[0], o[1], o[2], o[3]};
        }
    } else {
        const int samples = tw * 3;
        for (int i = threadIdx.x; i < th * samples; i += 256) {
            const int y = i / samples, e = i - y * samples, oy = oy0 + y, cnt = t.vcount[oy];
            const int16_t* const cf = t.vcoef + (size_t)oy * t.vt;
            const int16_t* src = hrow10 + (t.vfirst[oy] - lo) * TW3 + e;
            int acc = 0;
            for (int k = 0; k < cnt; ++k, src += TW3) acc += (int)cf[k] * (int)*src;
            fout[(size_t)oy * oW * 3 + e] = (uint16_t)round_clip_u10(acc);
        }
    }
}

hipError_t launch_resize_u10(const uint16_t* in, uint16_t* out, const ResizePlan& p, const int32_t* blob_dev, int n, hipStream_t s) {
    if (!in || !out || !blob_dev || n < 1 || p.max_rows < 1) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 2) return hipErrorInvalidValue;
    const size_t lds = (size_t)p.max_rows * TW3 * sizeof(int16_t);
    if (lds > 65536) return hipErrorInvalidValue;
    Resize10Tables t;
    t.hfirst = blob_dev;
    t.hcount = blob_dev + p.oW;
    t.vfirst = blob_dev + 2 * (size_t)p.oW;
    t.vcount = blob_dev + 2 * (size_t)p.oW + p.oH;
    t.hcoef = reinterpret_cast<const int16_t*>(blob_dev + 2 * (size_t)p.oW + 2 * (size_t)p.oH);
    t.vcoef = t.hcoef + 2 * (((size_t)p.oW * p.ht + 1) / 2);
    t.ht = p.ht;
    t.vt = p.vt;
    // 8 samples are 16 bytes: a row of oW * 3 samples, a tile's 64 * 3 and its last tw * 3 divide into such groups where oW % 8 == 0, and
    // every group of every row and frame is then 16-byte aligned with the destination
    const bool words = p.oW % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const size_t fin = (size_t)p.H * p.W * 3, fout = (size_t)p.oH * p.oW * 3;
    for (int f0 = 0; f0 < n; f0 += 65535) {                            // (the grid's z)
        const int nf = n - f0 < 65535 ? n - f0 : 65535;
        const dim3 grid((p.oW + RESIZE_TW - 1) / RESIZE_TW, (p.oH + RESIZE_TH - 1) / RESIZE_TH, nf), block(256);
        if (words)
            hipLaunchKernelGGL(resize_u10_kernel<true>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, t, p.H, p.W, p.oH, p.oW);
        else
            hipLaunchKernelGGL(resize_u10_kernel<false>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, t, p.H, p.W, p.oH, p.oW);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pfnl
