// The streaming session's input side (include/pfnl_hip.h, pfnl_stream_*): LR frames arrive one at a time as uint8 and live in a device
// ring; the clamped T-frame windows of a batch (reference model/pfnl.py:238-242) are gathered from it and dequantised in one pass.
#include "common.h"

namespace pfnl {

namespace {

// u8 -> the harness's (u8 / 255.).astype(np.float32) (reference model/pfnl.py:287): the division in double, rounded ONCE to fp32 - the
// very expression, evaluated by the host compiler.  v * (1 / 255.f) differs from it for 126 of the 256 values, and an fp32 division
// would hang on the compiler's division flag; a table hangs on nothing.
struct DequantTable {
    float v[256];
    constexpr DequantTable() : v() {
        for (int i = 0; i < 256; ++i) v[i] = (float)((double)i / 255.0);
    }
};
__constant__ DequantTable kDequant = DequantTable();

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 dequant4(unsigned w, const float* tab) {
    return f32x4{tab[w & 255u], tab[(w >> 8) & 255u], tab[(w >> 16) & 255u], tab[w >> 24]};
}

}  // namespace

// ring [cap][frame_bytes] uint8, frame f in slot f % cap -> win [count][T][frame_bytes] fp32: window w, slot t = frame
// clamp(first + w + t - T/2, 0, last).  WORDS = 32-bit words per lane and step: 4 (one 16-byte read) where frame_bytes is a multiple of
// 16, else 1.  A quarter of gather_windows_kernel's read bytes, and its index arithmetic (one 64-bit division per chunk); the table
// sits in LDS (a per-lane index).
template <int WORDS>
__global__ __launch_bounds__(256) void stream_gather_u8_kernel(const uint8_t* __restrict__ ring, f32x4* __restrict__ win, int cap,
                                                               long long last, long long first, int count, int T,
                                                               size_t frame_chunks) {
    __shared__ float tab[256];
    tab[threadIdx.x] = kDequant.v[threadIdx.x];
    __syncthreads();
    const size_t total = (size_t)count * T * frame_chunks;            // chunks of 4 * WORDS bytes
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t e = i % frame_chunks;
        const int wt = (int)(i / frame_chunks);
        const int w = wt / T, t = wt - w * T;
        long long f = first + w + t - T / 2;
        f = f < 0 ? 0 : (f > last ? last : f);
        const size_t src = ((size_t)(f % cap) * frame_chunks + e) * (4 * WORDS);
        if constexpr (WORDS == 4) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(ring + src);
            f32x4* const dst = win + i * 4;
            dst[0] = dequant4(q.x, tab);
            dst[1] = dequant4(q.y, tab);
            dst[2] = dequant4(q.z, tab);
            dst[3] = dequant4(q.w, tab);
        } else {
            win[i] = dequant4(*reinterpret_cast<const unsigned*>(ring + src), tab);
        }
    }
}

// ring 4-byte aligned (16 for the wide reads, else the narrow form runs), win 16-byte aligned
hipError_t launch_gather_windows_u8(const uint8_t* ring, float* win, int cap, long long last, long long first, int count, int T,
                                    size_t frame_bytes, hipStream_t s) {
    if (frame_bytes % 4 || cap < 1 || last < 0 || count < 1 || T < 1 || reinterpret_cast<uintptr_t>(ring) % 4 ||
        reinterpret_cast<uintptr_t>(win) % 16)
        return hipErrorInvalidValue;
    const bool wide = frame_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(ring) % 16 == 0;
    const size_t frame_chunks = frame_bytes / (wide ? 16 : 4);
    const size_t total = (size_t)count * T * frame_chunks;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (wide)
        hipLaunchKernelGGL(stream_gather_u8_kernel<4>, dim3(blocks ? blocks : 1), dim3(256), 0, s, ring, reinterpret_cast<f32x4*>(win), cap,
                           last, first, count, T, frame_chunks);
    else
        hipLaunchKernelGGL(stream_gather_u8_kernel<1>, dim3(blocks ? blocks : 1), dim3(256), 0, s, ring, reinterpret_cast<f32x4*>(win), cap,
                           last, first, count, T, frame_chunks);
    return hipGetLastError();
}

}  // namespace pfnl
