// The 8 flips and transposes of a frame, for self-ensemble inference (include/pfnl_hip.h SELF-ENSEMBLE; the rule: pfnl_amd/ensemble.py).
// Member k: bit 0 mirrors W, bit 1 mirrors H, bit 2 transposes H and W and is applied last.  Two launches share one kernel pair:
//   launch_dihedral        out = g_k(in) * scale            in [n][H][W][3] -> out [n][H][W][3], or [n][W][H][3] for k >= 4
//   launch_dihedral_accum  acc = (acc + g_k^-1(y)) * scale   y  [n][H][W][3], or [n][W][H][3] for k >= 4 -> acc [n][H][W][3]
// Both are a gather seen from the destination, which one thread owns per element: d[r][c] = s[fr(r)][fc(c)] for the mirrors and
// d[r][c] = s[fa(c)][fb(r)] for the transposing members, each f the identity or the mirror of its axis.  g_k and g_k^-1 differ only in
// which bit mirrors which source axis (Map below), so the accumulating launch is the same kernel with a read of the destination.
// Mirrors move whole pixels: a lane per 4 pixels = three 16-byte words on both sides where W % 4 == 0 and the pointers are 16-byte aligned,
// a lane per pixel otherwise.  Transposing members go through an LDS tile of 32 x 32 pixels: the source is read along its rows and the
// destination written along its rows, consecutive lanes on consecutive dwords on both sides.  A tile row is 96 dwords; its stride is 99:
// the column walk of the second pass reads dword lr * 99 + 3 lc + ch with lr = e / 3 and ch = e % 3 for consecutive e, bank
// (3 lr + ch + const) % 32 = (e + const) % 32 - 32 consecutive lanes on 32 banks (stride 96 would put every lr on one bank, stride 97
// leaves 3-way conflicts).  Edge tiles are clipped on both passes: nothing outside either image is read or written.
#include "common.h"

namespace pfnl {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DH_TILE = 32;                    // pixels per side of the transposing tile
constexpr int DH_STRIDE = DH_TILE * 3 + 3;     // dwords per tile row: 99 = 3 mod 32 (see above)

// s * scale, or (d + s) * scale; scale == 1 leaves the bits of s / of the sum as they are (the members before the last)
template <bool ACCUM>
__device__ __forceinline__ float combine(float d, float s, float scale) {
    const float v = ACCUM ? d + s : s;
    return scale == 1.0f ? v : v * scale;
}

// the mirrors, a lane per pixel: d[img][r][c] <- s[img][flip_r ? H-1-r : r][flip_c ? W-1-c : c]
template <bool ACCUM>
__global__ __launch_bounds__(256) void dihedral_mirror_px_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t rows, int H, int W,
                                                                 int flip_r, int flip_c, float scale) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * (size_t)W) return;
    const size_t row = i / (size_t)W, img = row / (size_t)H;
    const int c = (int)(i - row * (size_t)W), r = (int)(row - img * (size_t)H);
    const int sr = flip_r ? H - 1 - r : r, sc = flip_c ? W - 1 - c : c;
    const float* const s = src + ((img * H + sr) * (size_t)W + sc) * 3;
    float* const d = dst + i * 3;
    const float s0 = s[0], s1 = s[1], s2 = s[2];
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if constexpr (ACCUM) d0 = d[0], d1 = d[1], d2 = d[2];
    d[0] = combine<ACCUM>(d0, s0, scale);
    d[1] = combine<ACCUM>(d1, s1, scale);
    d[2] = combine<ACCUM>(d2, s2, scale);
}

// the mirrors, a lane per 4 pixels (W % 4 == 0, both pointers 16-byte aligned): 48 bytes = three 16-byte words in, three out; a mirrored
// row takes the group from the other end of the source row and reverses its four pixels in registers
template <bool ACCUM>
__global__ __launch_bounds__(256) void dihedral_mirror_v4_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t rows, int H, int W,
                                                                 int flip_r, int flip_c, float scale) {
    const int G = W >> 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * (size_t)G) return;
    const size_t row = i / (size_t)G, img = row / (size_t)H;
    const int g = (int)(i - row * (size_t)G), r = (int)(row - img * (size_t)H);
    const int sr = flip_r ? H - 1 - r : r, sg = flip_c ? G - 1 - g : g;
    const f32x4* const s = reinterpret_cast<const f32x4*>(src + ((img * H + sr) * (size_t)W + 4 * (size_t)sg) * 3);
    f32x4* const d = reinterpret_cast<f32x4*>(dst + i * 12);
    const f32x4 a = s[0], b = s[1], c = s[2];                  // pixels (a.xyz) (a.w b.xy) (b.zw c.x) (c.yzw)
    f32x4 o0 = a, o1 = b, o2 = c;
    if (flip_c) {
        o0 = f32x4{c.y, c.z, c.w, b.z};
        o1 = f32x4{b.w, c.x, a.w, b.x};
        o2 = f32x4{b.y, a.x, a.y, a.z};
    }
    if constexpr (ACCUM) {
        const f32x4 p0 = d[0], p1 = d[1], p2 = d[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o0[q] = combine<true>(p0[q], o0[q], scale);
            o1[q] = combine<true>(p1[q], o1[q], scale);
            o2[q] = combine<true>(p2[q], o2[q], scale);
        }
    }
    d[0] = o0;
    d[1] = o1;
    d[2] = o2;
}

// the transposing members: d [n][DH][DW][3] <- s [n][DW][DH][3], d[r][c] = s[flip_a ? DW-1-c : c][flip_b ? DH-1-r : r].
// grid (tiles across d, tiles down d, images); a tile of th x tw destination pixels reads tw source rows of th pixels each
template <bool ACCUM>
__global__ __launch_bounds__(256) void dihedral_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int DH, int DW,
                                                                 int flip_a, int flip_b, float scale) {
    __shared__ float tile[DH_TILE * DH_STRIDE];
    const int r0 = blockIdx.y * DH_TILE, c0 = blockIdx.x * DH_TILE;
    const int th = DH - r0 < DH_TILE ? DH - r0 : DH_TILE, tw = DW - c0 < DH_TILE ? DW - c0 : DH_TILE;
    const int SH = DW, SW = DH;                                          // the source image
    const int sr0 = flip_a ? SH - c0 - tw : c0, sc0 = flip_b ? SW - r0 - th : r0;   // its tile: rows sr0 .. sr0 + tw - 1, columns sc0 .. sc0 + th - 1
    const size_t img = (size_t)blockIdx.z * DH * DW * 3;
    const float* const s = src + img + ((size_t)sr0 * SW + sc0) * 3;
    float* const d = dst + img + ((size_t)r0 * DW + c0) * 3;

    const int sw3 = th * 3;                                              // dwords of one source tile row
    for (int i = threadIdx.x; i < tw * sw3; i += 256) {
        const int lr = i / sw3, e = i - lr * sw3;
        tile[lr * DH_STRIDE + e] = s[(size_t)lr * SW * 3 + e];
    }
    __syncthreads();
    const int dw3 = tw * 3;                                              // dwords of one destination tile row
    for (int i = threadIdx.x; i < th * dw3; i += 256) {
        const int r = i / dw3, e = i - r * dw3, c = e / 3, ch = e - 3 * c;
        const int lr = flip_a ? tw - 1 - c : c, lc = flip_b ? th - 1 - r : r;
        float* const p = d + (size_t)r * DW * 3 + e;
        float old = 0.f;
        if constexpr (ACCUM) old = *p;
        *p = combine<ACCUM>(old, tile[lr * DH_STRIDE + lc * 3 + ch], scale);
    }
}

// which source axis each bit of k mirrors, seen from the destination (the header of this file)
struct Map {
    bool transpose;
    int flip_first, flip_second;   // mirrors: of the row / the column index; transposing: flip_a (source rows) / flip_b (source columns)
};

// inverse = false: d = g_k(s).  Mirrors: d[r][c] = s[fH(r)][fW(c)].  Transposing: d is [W][H], d[r][c] = s[fH(c)][fW(r)] - source rows
//                  carry bit 1, source columns bit 0.
// inverse = true:  d = g_k^-1(s).  Mirrors: their own inverse.  Transposing: d is [H][W], d[r][c] = s[fW(c)][fH(r)] - source rows (the W
//                  axis) carry bit 0, source columns bit 1.
Map dihedral_map(int k, bool inverse) {
    const int bw = k & 1, bh = (k >> 1) & 1;
    if (!(k & 4)) return Map{false, bh, bw};
    return inverse ? Map{true, bw, bh} : Map{true, bh, bw};
}

// d [n][DH][DW][3]; the source is [n][DH][DW][3] for the mirrors and [n][DW][DH][3] for the transposing members
template <bool ACCUM>
hipError_t launch_map(const float* src, float* dst, int n, int DH, int DW, const Map& m, float scale, hipStream_t s) {
    if (!src || !dst || n < 1 || DH < 1 || DW < 1) return hipErrorInvalidValue;
    if (m.transpose) {
        const size_t per = (size_t)DH * DW * 3;
        for (int f0 = 0; f0 < n; f0 += 65535) {                        // (the grid's z)
            const int nf = n - f0 < 65535 ? n - f0 : 65535;
            const dim3 grid((DW + DH_TILE - 1) / DH_TILE, (DH + DH_TILE - 1) / DH_TILE, nf);
            if (grid.y > 65535u) return hipErrorInvalidValue;
            hipLaunchKernelGGL(dihedral_transpose_kernel<ACCUM>, grid, dim3(256), 0, s, src + f0 * per, dst + f0 * per, DH, DW, m.flip_first,
                               m.flip_second, scale);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    const size_t rows = (size_t)n * DH;
    const bool words = DW % 4 == 0 && (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0;
    const size_t items = rows * (size_t)(words ? DW / 4 : DW), blocks = (items + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    if (words)
        hipLaunchKernelGGL(dihedral_mirror_v4_kernel<ACCUM>, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, rows, DH, DW, m.flip_first,
                           m.flip_second, scale);
    else
        hipLaunchKernelGGL(dihedral_mirror_px_kernel<ACCUM>, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, rows, DH, DW, m.flip_first,
                           m.flip_second, scale);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_dihedral(const float* in, float* out, int n, int H, int W, int k, float scale, hipStream_t s) {
    if (k < 0 || k > 7) return hipErrorInvalidValue;
    const bool t = (k & 4) != 0;
    return launch_map<false>(in, out, n, t ? W : H, t ? H : W, dihedral_map(k, false), scale, s);
}

hipError_t launch_dihedral_accum(float* acc, const float* y, int n, int H, int W, int k, float scale, hipStream_t s) {
    if (k < 0 || k > 7) return hipErrorInvalidValue;
    return launch_map<true>(y, acc, n, H, W, dihedral_map(k, true), scale, s);
}

}  // namespace pfnl
