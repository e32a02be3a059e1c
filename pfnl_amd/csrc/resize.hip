// uint8 RGB frames at a chosen raster: the last step of the streaming session's output edge (include/pfnl_hip.h, pfnl_stream_resize), behind
// the quantisation and ahead of the YUV conversion.  The rule is stated once on the host in integers, pfnl_amd/resize.py: a separable Keys
// cubic (a = -1/2) whose support widens by in / out when the raster shrinks, coefficients with 14 fractional bits that sum to 2^14 per row,
// horizontal pass first into an unclipped intermediate with 6 fractional bits, one rounding and one clip at the end.  resize_axis builds
// that module's tables with 128-bit integers (no floating point, no device); the kernel reads tables and never evaluates the filter.
// One launch does both passes.  A workgroup owns RESIZE_TH x RESIZE_TW output pixels: it forms the horizontal pass of the input rows its
// vertical taps name - straight from the frame's bytes, neighbouring lanes on neighbouring bytes - into an int16 LDS tile of rows x TW x 3,
// and runs the vertical pass from there: a lane per 16 output bytes, read from LDS and stored as 16-byte words, where the destination's
// rows are 16-byte aligned; a lane per byte otherwise.  sum |c| <= 2^15 per row (checked when the table is built) keeps the intermediate
// inside int16 and the second pass's sum inside int32.
#include <string>

#include "common.h"

namespace pfnl {

namespace {

typedef __int128 i128;

i128 floor_div(i128 a, i128 b) {                                       // b > 0
    const i128 q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

i128 keys_weight(long long u, long long d) {                           // the Keys kernel at u / d, times 2 d^3
    const i128 U = u, D = d;
    if (u <= d) return 3 * U * U * U - 5 * U * U * D + 2 * D * D * D;
    if (u < 2 * d) return -U * U * U + 5 * U * U * D - 8 * U * D * D + 4 * D * D * D;
    return 0;
}

}  // namespace

bool resize_axis(int n_in, int n_out, ResizeAxis* t, std::string* why) {
    if (n_in < 1 || n_out < 1 || n_in > RESIZE_MAX_SIZE || n_out > RESIZE_MAX_SIZE) {
        *why = "resize: sizes must lie in 1 .. " + std::to_string(RESIZE_MAX_SIZE);
        return false;
    }
    if (n_out < (n_in + 3) / 4 || n_out > 2 * n_in) {
        *why = "resize: " + std::to_string(n_in) + " -> " + std::to_string(n_out) + ": the output must lie between a quarter and twice the input";
        return false;
    }
    const long long d = 2LL * (n_in > n_out ? n_in : n_out);
    std::vector<std::vector<int>> rows((size_t)n_out);
    t->first.assign((size_t)n_out, 0);
    t->count.assign((size_t)n_out, 0);
    t->ntaps = 0;
    std::vector<i128> w;
    for (int o = 0; o < n_out; ++o) {
        const long long centre = (long long)n_in * (2 * o + 1);
        long long j = (long long)floor_div(centre - 2 * d - n_out, 2LL * n_out);   // the last index left of the support
        long long first = -1;
        w.clear();
        for (;;) {
            ++j;
            const long long n = (long long)n_out * (2 * j + 1) - centre;
            if (n >= 2 * d) break;
            if (n <= -2 * d) continue;
            const long long at = j < 0 ? 0 : (j > n_in - 1 ? n_in - 1 : j);
            if (first < 0) first = at;
            if ((size_t)(at - first) == w.size()) w.push_back(0);
            w[(size_t)(at - first)] += keys_weight(n < 0 ? -n : n, d);
        }
        i128 S = 0;
        for (const i128 x : w) S += x;
        if (first < 0 || S <= 0) {
            *why = "resize: empty filter row";
            return false;
        }
        std::vector<int>& c = rows[(size_t)o];
        c.resize(w.size());
        long long sum = 0, mag = 0;
        size_t big = 0;
        for (size_t k = 0; k < w.size(); ++k) {
            c[k] = (int)floor_div(2 * w[k] * (1 << 14) + S, 2 * S);
            sum += c[k];
            if (c[k] > c[big]) big = k;
        }
        c[big] += (int)((1 << 14) - sum);
        for (const int x : c) mag += x < 0 ? -x : x;
        if (mag > (1 << 15)) {
            *why = "resize: " + std::to_string(n_in) + " -> " + std::to_string(n_out) + ": a row's sum of magnitudes exceeds 2^15";
            return false;
        }
        t->first[(size_t)o] = (int32_t)first;
        t->count[(size_t)o] = (int32_t)c.size();
        if ((int)c.size() > t->ntaps) t->ntaps = (int)c.size();
        // the kernel sizes its tile by these: neither end of the run ever moves back
        if (o && (t->first[(size_t)o] < t->first[(size_t)o - 1] ||
                  t->first[(size_t)o] + t->count[(size_t)o] < t->first[(size_t)o - 1] + t->count[(size_t)o - 1])) {
            *why = "resize: tap runs out of order";
            return false;
        }
        if (first + (long long)c.size() > n_in) {
            *why = "resize: tap run outside the input";
            return false;
        }
    }
    t->coef.assign((size_t)n_out * t->ntaps, 0);
    for (int o = 0; o < n_out; ++o)
        for (size_t k = 0; k < rows[(size_t)o].size(); ++k) t->coef[(size_t)o * t->ntaps + k] = (int16_t)rows[(size_t)o][k];
    return true;
}

bool resize_plan(int H, int W, int oH, int oW, ResizePlan* p, std::string* why) {
    ResizeAxis h, v;
    if (!resize_axis(W, oW, &h, why) || !resize_axis(H, oH, &v, why)) return false;
    p->H = H, p->W = W, p->oH = oH, p->oW = oW, p->ht = h.ntaps, p->vt = v.ntaps;
    p->max_rows = 0;
    for (int y0 = 0; y0 < oH; y0 += RESIZE_TH) {
        const int y1 = (y0 + RESIZE_TH < oH ? y0 + RESIZE_TH : oH) - 1;
        const int rows = v.first[(size_t)y1] + v.count[(size_t)y1] - v.first[(size_t)y0];
        if (rows > p->max_rows) p->max_rows = rows;
    }
    if ((size_t)p->max_rows * RESIZE_TW * 3 * sizeof(int16_t) > 65536) {   // (a 4 : 1 reduction names 76 rows: 29 184 bytes)
        *why = "resize: the tile's intermediate does not fit the LDS";
        return false;
    }
    // hfirst [oW] | hcount [oW] | vfirst [oH] | vcount [oH] | hcoef int16 [oW][ht] | vcoef int16 [oH][vt], each part on a 4-byte boundary
    const size_t hc = ((size_t)oW * h.ntaps + 1) / 2, vc = ((size_t)oH * v.ntaps + 1) / 2;
    p->blob.assign(2 * (size_t)oW + 2 * (size_t)oH + hc + vc, 0);
    int32_t* b = p->blob.data();
    std::copy(h.first.begin(), h.first.end(), b);
    std::copy(h.count.begin(), h.count.end(), b + oW);
    std::copy(v.first.begin(), v.first.end(), b + 2 * (size_t)oW);
    std::copy(v.count.begin(), v.count.end(), b + 2 * (size_t)oW + oH);
    int16_t* c = reinterpret_cast<int16_t*>(b + 2 * (size_t)oW + 2 * (size_t)oH);
    std::copy(h.coef.begin(), h.coef.end(), c);
    std::copy(v.coef.begin(), v.coef.end(), c + 2 * hc);
    return true;
}

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int TW3 = RESIZE_TW * 3;                                     // int16 per row of the intermediate tile

struct ResizeTables {
    const int32_t *hfirst, *hcount, *vfirst, *vcount;
    const int16_t *hcoef, *vcoef;
    int ht, vt;
};

// clip((v + 2^19) >> 20, 0, 255) with the clamp ahead of the shift, as in yuv.hip (shift_clip_u8: tools/GFX950_NOTES.md)
__device__ __forceinline__ unsigned round_clip_u8(int v) {
    v += 1 << 19;
    v = v < 0 ? 0 : v;
    v = v > (256 << 20) - 1 ? (256 << 20) - 1 : v;
    return (unsigned)(v >> 20);
}

}  // namespace

// in [n][H][W][3] -> out [n][oH][oW][3]; grid (tiles across, tiles down, frames); LDS: the launch's rows x TW3 int16
template <bool WORDS>
__global__ __launch_bounds__(256) void resize_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, ResizeTables t, int H, int W,
                                                        int oH, int oW) {
    extern __shared__ __attribute__((aligned(16))) int16_t hrow[];
    const int ox0 = blockIdx.x * RESIZE_TW, oy0 = blockIdx.y * RESIZE_TH;
    const int tw = oW - ox0 < RESIZE_TW ? oW - ox0 : RESIZE_TW, th = oH - oy0 < RESIZE_TH ? oH - oy0 : RESIZE_TH;
    const int lo = t.vfirst[oy0];                                      // the tile's input rows: lo .. lo + rows - 1 (the runs never move back)
    const int rows = t.vfirst[oy0 + th - 1] + t.vcount[oy0 + th - 1] - lo;
    const uint8_t* const fin = in + (size_t)blockIdx.z * H * W * 3;
    uint8_t* const fout = out + ((size_t)blockIdx.z * oH * oW + ox0) * 3;

    // horizontal pass: element e = 3 x + c of input row lo + r; the columns right of the frame are zero (nothing reads them)
    for (int i = threadIdx.x; i < rows * TW3; i += 256) {
        const int r = i / TW3, e = i - r * TW3, x = e / 3, c = e - 3 * x;
        int v = 0;
        if (x < tw) {
            const int ox = ox0 + x, cnt = t.hcount[ox];
            const int16_t* const cf = t.hcoef + (size_t)ox * t.ht;
            const uint8_t* const p = fin + ((size_t)(lo + r) * W + t.hfirst[ox]) * 3 + c;
            int acc = 1 << 7;
            for (int k = 0; k < cnt; ++k) acc += (int)cf[k] * (int)p[3 * k];
            v = acc >> 8;
        }
        hrow[i] = (int16_t)v;
    }
    __syncthreads();

    // vertical pass
    if constexpr (WORDS) {
        const int groups = tw * 3 / 16;                                // exact: oW is a multiple of 16, ox0 of 64
        for (int i = threadIdx.x; i < th * groups; i += 256) {
            const int y = i / groups, g = i - y * groups, oy = oy0 + y, cnt = t.vcount[oy];
            const int16_t* const cf = t.vcoef + (size_t)oy * t.vt;
            const int16_t* src = hrow + (t.vfirst[oy] - lo) * TW3 + 16 * g;
            int acc[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0;
            for (int k = 0; k < cnt; ++k, src += TW3) {
                const int c = cf[k];
                const u32x4 a = *reinterpret_cast<const u32x4*>(src), b = *reinterpret_cast<const u32x4*>(src + 8);
                const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    acc[2 * q] += c * (int)(int16_t)(w[q] & 0xffffu);
                    acc[2 * q + 1] += c * ((int)w[q] >> 16);
                }
            }
            unsigned o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                o[q] = round_clip_u8(acc[4 * q]) | (round_clip_u8(acc[4 * q + 1]) << 8) | (round_clip_u8(acc[4 * q + 2]) << 16) |
                       (round_clip_u8(acc[4 * q + 3]) << 24);
            *reinterpret_cast<u32x4*>(fout + (size_t)oy * oW * 3 + 16 * g) = u32x4{o[0], o[1], o[2], o[3]};
        }
    } else {
        const int bytes = tw * 3;
        for (int i = threadIdx.x; i < th * bytes; i += 256) {
            const int y = i / bytes, e = i - y * bytes, oy = oy0 + y, cnt = t.vcount[oy];
            const int16_t* const cf = t.vcoef + (size_t)oy * t.vt;
            const int16_t* src = hrow + (t.vfirst[oy] - lo) * TW3 + e;
            int acc = 0;
            for (int k = 0; k < cnt; ++k, src += TW3) acc += (int)cf[k] * (int)*src;
            fout[(size_t)oy * oW * 3 + e] = (uint8_t)round_clip_u8(acc);
        }
    }
}

hipError_t launch_resize_u8(const uint8_t* in, uint8_t* out, const ResizePlan& p, const int32_t* blob_dev, int n, hipStream_t s) {
    if (!in || !out || !blob_dev || n < 1 || p.max_rows < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)p.max_rows * TW3 * sizeof(int16_t);
    if (lds > 65536) return hipErrorInvalidValue;
    ResizeTables t;
    t.hfirst = blob_dev;
    t.hcount = blob_dev + p.oW;
    t.vfirst = blob_dev + 2 * (size_t)p.oW;
    t.vcount = blob_dev + 2 * (size_t)p.oW + p.oH;
    t.hcoef = reinterpret_cast<const int16_t*>(blob_dev + 2 * (size_t)p.oW + 2 * (size_t)p.oH);
    t.vcoef = t.hcoef + 2 * (((size_t)p.oW * p.ht + 1) / 2);
    t.ht = p.ht;
    t.vt = p.vt;
    const bool words = p.oW % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const size_t fin = (size_t)p.H * p.W * 3, fout = (size_t)p.oH * p.oW * 3;
    for (int f0 = 0; f0 < n; f0 += 65535) {                            // (the grid's z)
        const int nf = n - f0 < 65535 ? n - f0 : 65535;
        const dim3 grid((p.oW + RESIZE_TW - 1) / RESIZE_TW, (p.oH + RESIZE_TH - 1) / RESIZE_TH, nf), block(256);
        if (words)
            hipLaunchKernelGGL(resize_u8_kernel<true>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, t, p.H, p.W, p.oH, p.oW);
        else
            hipLaunchKernelGGL(resize_u8_kernel<false>, grid, block, lds, s, in + f0 * fin, out + f0 * fout, t, p.H, p.W, p.oH, p.oW);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pfnl
