// Y-channel PSNR and SSIM sums of uint8 RGB frame pairs (pfnl_op_score_y), the device form of pfnl_amd/metrics.py:
// rgb2ycbcr's Y row (reference utils.py:194-211), the squared-error sums of matlab/compute_psnr.m and AVG_PSNR (utils.py:213-246)
// and the SSIM map of modules/SSIM_Index.py:23-89 (11x11 Gaussian, sigma 1.5, scipy.ndimage's 'reflect' boundary).
//
// One workgroup scores one SCORE_TW x SCORE_TH tile of one frame pair in ONE pass over the bytes:
//   1. the tile + 5-pixel halo of both frames is read once, turned into Y (fp64) and kept in LDS - no Y plane is ever stored;
//   2. the horizontal 11-tap pass of the five planes a, b, a^2, b^2, ab goes LDS -> LDS (the 2-D window is the outer product
//      of the normalised 1-D one, so the filter is separable);
//   3. the vertical pass, the SSIM map and the squared error are formed per output pixel in registers and summed.
// Everything is fp64: with L = 255 a variance is the difference of two numbers near 6.5e4 against C2 = 58.5.
// Repeatable bit for bit: every workgroup adds its pixels in a fixed order (fixed per-thread order, then a fixed LDS tree) into
// its OWN slot of the partials scratch, and score_finalize_kernel adds the slots of a frame in a fixed order.  No atomics.
#include <cmath>

#include "common.h"

namespace pfnl {

namespace {

constexpr int SCORE_TW = 32, SCORE_TH = 16;                       // output tile of one workgroup
constexpr int SCORE_R = 5;                                        // radius of the 11-tap window
constexpr int SCORE_IW = SCORE_TW + 2 * SCORE_R, SCORE_IH = SCORE_TH + 2 * SCORE_R;   // tile + halo: 42 x 26
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_SUMS = 4;                                     // sum_d2_full, sum_d2_crop, ssim_sum_full, ssim_sum_valid

struct ScoreTaps {
    double g[2 * SCORE_R + 1];                                    // exp(-(i - 5)^2 / (2 * 1.5^2)) / sum
};

// scipy.ndimage 'reflect' (half-sample symmetric): -1 -> 0, -2 -> 1, n -> n - 1.  One reflection is enough for a 5-pixel halo of an
// axis of n >= 11; the clamp only catches halo positions past the reflected range of a ragged edge tile (they feed no pixel of the frame).
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -1 - i : i;
    i = i >= n ? 2 * n - 1 - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ double luma(const uint8_t* __restrict__ p) {
    return 16.0 + 0.256788235294118 * (double)p[0] + 0.504129411764706 * (double)p[1] + 0.097905882352941 * (double)p[2];
}

// the four sums of the workgroup's threads, added in a fixed order -> dst[0..3] (thread 0 writes)
__device__ __forceinline__ void block_sum4(const double (&v)[SCORE_SUMS], double* red, double* dst) {
    const int t = threadIdx.x;
    for (int q = 0; q < SCORE_SUMS; ++q) red[q * SCORE_THREADS + t] = v[q];
    __syncthreads();
    for (int step = SCORE_THREADS / 2; step > 0; step >>= 1) {
        if (t < step)
            for (int q = 0; q < SCORE_SUMS; ++q) red[q * SCORE_THREADS + t] += red[q * SCORE_THREADS + t + step];
        __syncthreads();
    }
    if (t < SCORE_SUMS) dst[t] = red[t * SCORE_THREADS];
}

__global__ __launch_bounds__(SCORE_THREADS) void score_y_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                                int H, int W, int tiles_x, int sp_border, ScoreTaps taps,
                                                                double* __restrict__ partial) {
    __shared__ double ya[SCORE_IH][SCORE_IW], yb[SCORE_IH][SCORE_IW];     // a = truth, b = prediction (Y)
    __shared__ double hz[5][SCORE_IH][SCORE_TW];                          // horizontally filtered a, b, a^2, b^2, ab

    const int t = threadIdx.x;
    const int tile = blockIdx.x, f = blockIdx.y;
    const int x0 = (tile % tiles_x) * SCORE_TW, y0 = (tile / tiles_x) * SCORE_TH;
    const size_t frame = (size_t)f * H * W * 3;

    for (int i = t; i < SCORE_IH * SCORE_IW; i += SCORE_THREADS) {
        const int r = i / SCORE_IW, c = i % SCORE_IW;
        const size_t px = frame + ((size_t)reflect(y0 + r - SCORE_R, H) * W + reflect(x0 + c - SCORE_R, W)) * 3;
        ya[r][c] = luma(truth + px);
        yb[r][c] = luma(pred + px);
    }
    __syncthreads();

    for (int i = t; i < SCORE_IH * SCORE_TW; i += SCORE_THREADS) {
        const int r = i / SCORE_TW, c = i % SCORE_TW;
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k <= 2 * SCORE_R; ++k) {
            const double a = ya[r][c + k], b = yb[r][c + k], g = taps.g[k];
            s[0] += g * a;
            s[1] += g * b;
            s[2] += g * (a * a);
            s[3] += g * (b * b);
            s[4] += g * (a * b);
        }
#pragma unroll
        for (int p = 0; p < 5; ++p) hz[p][r][c] = s[p];
    }
    __syncthreads();

    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double acc[SCORE_SUMS] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < SCORE_TH * SCORE_TW; i += SCORE_THREADS) {
        const int r = i / SCORE_TW, c = i % SCORE_TW;
        const int y = y0 + r, x = x0 + c;
        if (y >= H || x >= W) continue;
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k <= 2 * SCORE_R; ++k) {
            const double g = taps.g[k];
#pragma unroll
            for (int p = 0; p < 5; ++p) s[p] += g * hz[p][r + k][c];
        }
        const double mu1 = s[0], mu2 = s[1];
        const double s1 = s[2] - mu1 * mu1, s2 = s[3] - mu2 * mu2, s12 = s[4] - mu1 * mu2;
        const double m = ((2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
        const double d = ya[r + SCORE_R][c + SCORE_R] - yb[r + SCORE_R][c + SCORE_R];
        const double d2 = d * d;
        acc[0] += d2;
        if (y >= sp_border && y < H - sp_border && x >= sp_border && x < W - sp_border) acc[1] += d2;
        acc[2] += m;
        if (y >= SCORE_R && y < H - SCORE_R && x >= SCORE_R && x < W - SCORE_R) acc[3] += m;
    }
    __syncthreads();                                                     // hz is reused as the reduction buffer
    block_sum4(acc, &hz[0][0][0], partial + ((size_t)f * gridDim.x + tile) * SCORE_SUMS);
}

// out[f][q] = the sum over the frame's tiles of partial[f][tile][q]: thread t adds tiles t, t + 256, ... in that order, then the fixed tree
__global__ __launch_bounds__(SCORE_THREADS) void score_finalize_kernel(const double* __restrict__ partial, int tiles,
                                                                       double* __restrict__ out) {
    __shared__ double red[SCORE_SUMS * SCORE_THREADS];
    const int f = blockIdx.x;
    const double* p = partial + (size_t)f * tiles * SCORE_SUMS;
    double acc[SCORE_SUMS] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < tiles; i += SCORE_THREADS)
        for (int q = 0; q < SCORE_SUMS; ++q) acc[q] += p[(size_t)i * SCORE_SUMS + q];
    block_sum4(acc, red, out + (size_t)f * SCORE_SUMS);
}

size_t score_tiles(int H, int W) {
    return (size_t)((H + SCORE_TH - 1) / SCORE_TH) * (size_t)((W + SCORE_TW - 1) / SCORE_TW);
}

}  // namespace

size_t score_scratch_bytes(int F, int H, int W) { return (size_t)F * score_tiles(H, W) * SCORE_SUMS * sizeof(double); }

hipError_t launch_score_y(const uint8_t* pred, const uint8_t* truth, int F, int H, int W, int sp_border, double* out, double* partial,
                          hipStream_t s) {
    static_assert(5 * SCORE_IH * SCORE_TW >= SCORE_SUMS * SCORE_THREADS, "the reduction reuses the filtered planes' LDS");
    ScoreTaps taps;
    double sum = 0.0;
    for (int i = 0; i <= 2 * SCORE_R; ++i) sum += taps.g[i] = std::exp(-(double)((i - SCORE_R) * (i - SCORE_R)) / (2.0 * 1.5 * 1.5));
    for (double& g : taps.g) g /= sum;
    const int tiles_x = (W + SCORE_TW - 1) / SCORE_TW;
    const unsigned tiles = (unsigned)score_tiles(H, W);
    hipLaunchKernelGGL(score_y_kernel, dim3(tiles, F), dim3(SCORE_THREADS), 0, s, pred, truth, H, W, tiles_x, sp_border, taps, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_finalize_kernel, dim3(F), dim3(SCORE_THREADS), 0, s, partial, (int)tiles, out);
    return hipGetLastError();
}

}  // namespace pfnl
