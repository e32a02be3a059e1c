// The streaming session's input side (include/pfnl_hip.h, pfnl_stream_*): LR frames arrive one at a time as uint8 and live in a device
// ring; the clamped T-frame windows of a batch (reference model/pfnl.py:238-242) are gathered from it and dequantised in one pass.
// With scenes on (pfnl_stream_scenes; the rule: pfnl_amd/scene.py) every pushed frame is also compared with the one before it - an exact
// integer sum of absolute luma differences - and each ring slot carries the first frame of its frame's scene, at which the windows clamp.
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

// ---- scenes ------------------------------------------------------------------------------------------------------------------------

namespace {

// integer BT.601 luma without the + 16 (only differences are used): pfnl_amd/scene.py luma_u8
__device__ __forceinline__ int luma_u8(unsigned r, unsigned g, unsigned b) { return (int)((66u * r + 129u * g + 25u * b + 128u) >> 8); }

template <int NW>
__device__ __forceinline__ unsigned byte_of(const unsigned (&w)[NW], int j) {
    return (w[j >> 2] >> (8 * (j & 3))) & 255u;
}

}  // namespace

// sum |luma(a) - luma(b)| over the npix pixels of two [npix][3] uint8 frames, exact.  A lane takes groups of 4 * WORDS pixels = 3 * WORDS
// 32-bit words (the three bytes of a pixel straddle the words; twelve bytes hold four whole pixels): WORDS = 4 reads 16 bytes at a time,
// WORDS = 1 reads 4, WORDS = 0 reads none; the pixels behind the last whole group (npix is a multiple of nothing) go byte by byte.
// Lanes -> wave (shuffles) -> block (LDS) -> scratch[0] (one atomic per block); the block that draws the last ticket of scratch[1]
// takes the total, leaves both words zero for the next launch and decides (SceneDecision).  Integer sums: any order gives the same value.
template <int WORDS>
__global__ __launch_bounds__(256) void stream_scene_sad_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t npix,
                                                               unsigned long long* __restrict__ scratch, SceneDecision d) {
    constexpr int NW = WORDS ? 3 * WORDS : 1;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    const size_t ngroups = WORDS ? npix / (4 * WORDS) : 0;
    unsigned long long sum = 0;
    if constexpr (WORDS != 0) {
        for (size_t g = gid; g < ngroups; g += nthreads) {
            unsigned wa[NW], wb[NW];
            if constexpr (WORDS == 4) {
                const u32x4* const pa = reinterpret_cast<const u32x4*>(a + g * 48);
                const u32x4* const pb = reinterpret_cast<const u32x4*>(b + g * 48);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const u32x4 qa = pa[k], qb = pb[k];
                    wa[4 * k] = qa.x, wa[4 * k + 1] = qa.y, wa[4 * k + 2] = qa.z, wa[4 * k + 3] = qa.w;
                    wb[4 * k] = qb.x, wb[4 * k + 1] = qb.y, wb[4 * k + 2] = qb.z, wb[4 * k + 3] = qb.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    wa[k] = reinterpret_cast<const unsigned*>(a + g * (12 * WORDS))[k];
                    wb[k] = reinterpret_cast<const unsigned*>(b + g * (12 * WORDS))[k];
                }
            }
            unsigned part = 0;                                    // at most 16 * 219
#pragma unroll
            for (int p = 0; p < 4 * WORDS; ++p) {
                const int ya = luma_u8(byte_of(wa, 3 * p), byte_of(wa, 3 * p + 1), byte_of(wa, 3 * p + 2));
                const int yb = luma_u8(byte_of(wb, 3 * p), byte_of(wb, 3 * p + 1), byte_of(wb, 3 * p + 2));
                part += (unsigned)(ya > yb ? ya - yb : yb - ya);
            }
            sum += part;
        }
    }
    for (size_t p = ngroups * (4 * WORDS) + gid; p < npix; p += nthreads) {
        const int ya = luma_u8(a[3 * p], a[3 * p + 1], a[3 * p + 2]), yb = luma_u8(b[3 * p], b[3 * p + 1], b[3 * p + 2]);
        sum += (unsigned)(ya > yb ? ya - yb : yb - ya);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    __shared__ unsigned long long wave_sum[4];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    atomicAdd(&scratch[0], wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3]);
    __threadfence();                                              // the block's sum is visible before its ticket is
    if (atomicAdd(&scratch[1], 1ull) != gridDim.x - 1) return;
    const unsigned long long total = atomicExch(&scratch[0], 0ull);
    atomicExch(&scratch[1], 0ull);
    d.sad[d.slot] = total;
    if (!d.scene_first) return;                                   // (the op hook: the sum alone)
    const unsigned long long prev = d.sad[d.prev], diff = total > prev ? total - prev : prev - total;
    const bool cut = d.force || (d.detect && (total < diff ? total : diff) >= d.thr_sum);
    d.scene_first[d.slot] = cut ? d.frame : d.scene_first[d.prev];
}

// frame 0 of a sequence starts scene 0 and is never a cut
__global__ void stream_scene_first_frame_kernel(unsigned long long* __restrict__ sad, long long* __restrict__ scene_first, int slot) {
    sad[slot] = 0;
    scene_first[slot] = 0;
}

// a, b: frames of npix pixels; scratch: two zeroed 64-bit words that every launch leaves zeroed (launches that share them must not overlap)
hipError_t launch_scene_sad_u8(const uint8_t* a, const uint8_t* b, size_t npix, unsigned long long* scratch, const SceneDecision& d,
                               hipStream_t s) {
    if (!npix || !scratch || !d.sad) return hipErrorInvalidValue;
    const uintptr_t align = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
    const int words = (npix * 3) % 16 == 0 && align % 16 == 0 ? 4 : (align % 4 == 0 ? 1 : 0);
    const size_t ngroups = words ? npix / (4 * words) : 0, rest = npix - ngroups * 4 * words;
    const size_t items = ngroups > rest ? ngroups : rest;
    const int blocks = (int)((items + 255) / 256 < 1024 ? (items + 255) / 256 : 1024);
    if (words == 4)
        hipLaunchKernelGGL(stream_scene_sad_kernel<4>, dim3(blocks), dim3(256), 0, s, a, b, npix, scratch, d);
    else if (words == 1)
        hipLaunchKernelGGL(stream_scene_sad_kernel<1>, dim3(blocks), dim3(256), 0, s, a, b, npix, scratch, d);
    else
        hipLaunchKernelGGL(stream_scene_sad_kernel<0>, dim3(blocks), dim3(256), 0, s, a, b, npix, scratch, d);
    return hipGetLastError();
}

hipError_t launch_scene_first_frame(unsigned long long* sad, long long* scene_first, int slot, hipStream_t s) {
    hipLaunchKernelGGL(stream_scene_first_frame_kernel, dim3(1), dim3(1), 0, s, sad, scene_first, slot);
    return hipGetLastError();
}

// stream_gather_u8_kernel with the windows kept inside the centre's scene: scene_first [cap], slot f % cap = the first frame of frame f's
// scene (non-decreasing in f, so a scene's frames are contiguous).  Window w (centre c = first + w), slot t = frame
// clamp(c + t - T/2, a, b): a = scene_first[c], b = the last frame <= min(c + T/2, last) whose scene_first is a - resolved per chunk, at most
// T/2 reads of a table that stays in cache.  One scene: stream_gather_u8_kernel's windows.
template <int WORDS>
__global__ __launch_bounds__(256) void stream_gather_u8_scenes_kernel(const uint8_t* __restrict__ ring, const long long* __restrict__ scene_first,
                                                                      f32x4* __restrict__ win, int cap, long long last, long long first,
                                                                      int count, int T, size_t frame_chunks) {
    __shared__ float tab[256];
    tab[threadIdx.x] = kDequant.v[threadIdx.x];
    __syncthreads();
    const size_t total = (size_t)count * T * frame_chunks;            // chunks of 4 * WORDS bytes
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t e = i % frame_chunks;
        const int wt = (int)(i / frame_chunks);
        const int w = wt / T, t = wt - w * T;
        const long long c = first + w, a = scene_first[c % cap];
        long long f = c + t - T / 2;
        if (t < T / 2) {
            f = f < a ? a : f;
            f = f < 0 ? 0 : f;                                        // (a table that is not a session's: stay in the ring)
        } else if (t > T / 2) {
            long long b = c;
            for (long long g = c + 1; g <= f && g <= last && scene_first[g % cap] == a; ++g) b = g;
            f = b;
        }
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

// as launch_gather_windows_u8; scene_first [cap] on the device, first >= 0
hipError_t launch_gather_windows_u8_scenes(const uint8_t* ring, const long long* scene_first, float* win, int cap, long long last,
                                           long long first, int count, int T, size_t frame_bytes, hipStream_t s) {
    if (frame_bytes % 4 || cap < 1 || last < 0 || first < 0 || count < 1 || T < 1 || !scene_first || reinterpret_cast<uintptr_t>(ring) % 4 ||
        reinterpret_cast<uintptr_t>(win) % 16)
        return hipErrorInvalidValue;
    const bool wide = frame_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(ring) % 16 == 0;
    const size_t frame_chunks = frame_bytes / (wide ? 16 : 4);
    const size_t total = (size_t)count * T * frame_chunks;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (wide)
        hipLaunchKernelGGL(stream_gather_u8_scenes_kernel<4>, dim3(blocks ? blocks : 1), dim3(256), 0, s, ring, scene_first,
                           reinterpret_cast<f32x4*>(win), cap, last, first, count, T, frame_chunks);
    else
        hipLaunchKernelGGL(stream_gather_u8_scenes_kernel<1>, dim3(blocks ? blocks : 1), dim3(256), 0, s, ring, scene_first,
                           reinterpret_cast<f32x4*>(win), cap, last, first, count, T, frame_chunks);
    return hipGetLastError();
}

}  // namespace pfnl
