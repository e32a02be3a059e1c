// The streaming session's input side (include/pfnl_hip.h, pfnl_stream_*): LR frames arrive one at a time as uint8 - or, at an input depth
// of 10 bits (pfnl_stream_input_depth), as uint16 with values 0 .. 1023 - and live in a device ring; the clamped T-frame windows of a batch
// (reference model/pfnl.py:238-242) are gathered from it and dequantised in one pass.  Each kernel is one body over the sample type.
// With scenes on (pfnl_stream_scenes; the rule: pfnl_amd/scene.py) every pushed frame is also compared with the one before it - an exact
// integer sum of absolute luma differences - and each ring slot carries the first frame of its frame's scene, at which the windows clamp.
#include "sample_depth.h"

namespace pfnl {

namespace {

// u8 -> the harness's (u8 / 255.).astype(np.float32) (reference model/pfnl.py:287): the division in double, rounded ONCE to fp32 - the
// very expression, evaluated by the host compiler.  v * (1 / 255.f) differs from it for 126 of the 256 values, and an fp32 division
// would hang on the compiler's division flag; a table hangs on nothing.  10 bits: u10 / 1023. by the same expression (depth10.py
// dequantise10), 1024 entries = 4 KB of LDS; a sample above 1023 reads entry 1023.
template <int N>
struct DequantTable {
    float v[N];
    constexpr DequantTable() : v() {
        for (int i = 0; i < N; ++i) v[i] = (float)((double)i / (double)(N - 1));
    }
};
__constant__ DequantTable<256> kDequant = DequantTable<256>();
__constant__ DequantTable<1024> kDequant10 = DequantTable<1024>();

template <typename T>
__device__ __forceinline__ void fill_dequant_table(float* tab) {
    if constexpr (sizeof(T) == 1) {
        tab[threadIdx.x] = kDequant.v[threadIdx.x];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) tab[threadIdx.x + 256 * k] = kDequant10.v[threadIdx.x + 256 * k];
    }
    __syncthreads();
}

__device__ __forceinline__ f32x4 dequant4(unsigned w, const float* tab) {
    return f32x4{tab[w & 255u], tab[(w >> 8) & 255u], tab[(w >> 16) & 255u], tab[w >> 24]};
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned clamp10(unsigned v) { return v > 1023u ? 1023u : v; }

// chunk i of the windows (4 * WORDS bytes of samples at src) -> its fp32 values at win: 4 * WORDS floats of uint8, 2 * WORDS of uint16
template <typename T, int WORDS>
__device__ __forceinline__ void dequant_chunk(const T* __restrict__ src, float* __restrict__ win, size_t i, const float* tab) {
    if constexpr (sizeof(T) == 1) {
        f32x4* const dst = reinterpret_cast<f32x4*>(win) + i * WORDS;
        if constexpr (WORDS == 4) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(src);
            dst[0] = dequant4(q.x, tab);
            dst[1] = dequant4(q.y, tab);
            dst[2] = dequant4(q.z, tab);
            dst[3] = dequant4(q.w, tab);
        } else {
            dst[0] = dequant4(*reinterpret_cast<const unsigned*>(src), tab);
        }
    } else {
        if constexpr (WORDS == 4) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(src);
            f32x4* const dst = reinterpret_cast<f32x4*>(win) + i * 2;
            dst[0] = f32x4{tab[clamp10(q.x & 65535u)], tab[clamp10(q.x >> 16)], tab[clamp10(q.y & 65535u)], tab[clamp10(q.y >> 16)]};
            dst[1] = f32x4{tab[clamp10(q.z & 65535u)], tab[clamp10(q.z >> 16)], tab[clamp10(q.w & 65535u)], tab[clamp10(q.w >> 16)]};
        } else {
            const unsigned w = *reinterpret_cast<const unsigned*>(src);
            reinterpret_cast<f32x2*>(win)[i] = f32x2{tab[clamp10(w & 65535u)], tab[clamp10(w >> 16)]};
        }
    }
}

}  // namespace

// ring [cap][frame_bytes] samples of T, frame f in slot f % cap -> win [count][NT][frame samples] fp32: window w, slot t = frame
// clamp(first + w + t - NT/2, 0, last).  WORDS = 32-bit words per lane and step: 4 (one 16-byte read) where frame_bytes is a multiple of
// 16, else 1.  A quarter (uint16: half) of gather_windows_kernel's read bytes, and its index arithmetic (one 64-bit division per chunk);
// the table sits in LDS (a per-lane index).
// SCENES: the windows are kept inside the centre's scene: scene_first [cap], slot f % cap = the first frame of frame f's scene
// (non-decreasing in f, so a scene's frames are contiguous).  Window w (centre c = first + w), slot t = frame clamp(c + t - NT/2, a, b):
// a = scene_first[c], b = the last frame <= min(c + NT/2, last) whose scene_first is a - resolved per chunk, at most NT/2 reads of a table
// that stays in cache.  One scene: the plain windows.
template <typename T, int WORDS, bool SCENES>
__global__ __launch_bounds__(256) void stream_gather_kernel(const T* __restrict__ ring, const long long* __restrict__ scene_first,
                                                            float* __restrict__ win, int cap, long long last, long long first, int count,
                                                            int NT, size_t frame_chunks) {
    __shared__ float tab[Depth<T>::LEVELS];
    fill_dequant_table<T>(tab);
    const size_t total = (size_t)count * NT * frame_chunks;           // chunks of 4 * WORDS bytes
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t e = i % frame_chunks;
        const int wt = (int)(i / frame_chunks);
        const int w = wt / NT, t = wt - w * NT;
        long long f = first + w + t - NT / 2;
        if constexpr (SCENES) {
            const long long c = first + w, a = scene_first[c % cap];
            if (t < NT / 2) {
                f = f < a ? a : f;
                f = f < 0 ? 0 : f;                                    // (a table that is not a session's: stay in the ring)
            } else if (t > NT / 2) {
                long long b = c;
                for (long long g = c + 1; g <= f && g <= last && scene_first[g % cap] == a; ++g) b = g;
                f = b;
            }
        } else {
            f = f < 0 ? 0 : (f > last ? last : f);
        }
        const size_t src = ((size_t)(f % cap) * frame_chunks + e) * (4 * WORDS);
        dequant_chunk<T, WORDS>(reinterpret_cast<const T*>(reinterpret_cast<const uint8_t*>(ring) + src), win, i, tab);
    }
}

namespace {

// scene_first null: the plain windows.  ring 4-byte aligned (16 for the wide reads, else the narrow form runs), win 16-byte aligned
template <typename T>
hipError_t launch_gather(const T* ring, const long long* scene_first, bool scenes, float* win, int cap, long long last, long long first,
                         int count, int NT, size_t frame_bytes, hipStream_t s) {
    if (frame_bytes % 4 || cap < 1 || last < 0 || count < 1 || NT < 1 || reinterpret_cast<uintptr_t>(ring) % 4 ||
        reinterpret_cast<uintptr_t>(win) % 16 || (scenes && (first < 0 || !scene_first)))
        return hipErrorInvalidValue;
    const bool wide = frame_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(ring) % 16 == 0;
    const size_t frame_chunks = frame_bytes / (wide ? 16 : 4);
    const size_t total = (size_t)count * NT * frame_chunks;
    const size_t blocks = (total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192;
    const dim3 grid((unsigned)(blocks ? blocks : 1)), block(256);
#define PFNL_GATHER_LAUNCH(W_, S_) \
    hipLaunchKernelGGL((stream_gather_kernel<T, W_, S_>), grid, block, 0, s, ring, scene_first, win, cap, last, first, count, NT, frame_chunks)
    if (wide && scenes)
        PFNL_GATHER_LAUNCH(4, true);
    else if (wide)
        PFNL_GATHER_LAUNCH(4, false);
    else if (scenes)
        PFNL_GATHER_LAUNCH(1, true);
    else
        PFNL_GATHER_LAUNCH(1, false);
#undef PFNL_GATHER_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gather_windows_u8(const uint8_t* ring, float* win, int cap, long long last, long long first, int count, int T,
                                    size_t frame_bytes, hipStream_t s) {
    return launch_gather<uint8_t>(ring, nullptr, false, win, cap, last, first, count, T, frame_bytes, s);
}

hipError_t launch_gather_windows_u10(const uint16_t* ring, float* win, int cap, long long last, long long first, int count, int T,
                                     size_t frame_bytes, hipStream_t s) {
    return launch_gather<uint16_t>(ring, nullptr, false, win, cap, last, first, count, T, frame_bytes, s);
}

// as launch_gather_windows_u8 / _u10; scene_first [cap] on the device, first >= 0
hipError_t launch_gather_windows_u8_scenes(const uint8_t* ring, const long long* scene_first, float* win, int cap, long long last,
                                           long long first, int count, int T, size_t frame_bytes, hipStream_t s) {
    return launch_gather<uint8_t>(ring, scene_first, true, win, cap, last, first, count, T, frame_bytes, s);
}

hipError_t launch_gather_windows_u10_scenes(const uint16_t* ring, const long long* scene_first, float* win, int cap, long long last,
                                            long long first, int count, int T, size_t frame_bytes, hipStream_t s) {
    return launch_gather<uint16_t>(ring, scene_first, true, win, cap, last, first, count, T, frame_bytes, s);
}

// ---- scenes ------------------------------------------------------------------------------------------------------------------------

namespace {

// integer BT.601 luma without the + 16 (only differences are used): pfnl_amd/scene.py luma_u8; 10-bit samples: luma_u10 - the same weights
// on the clamped values, (+ 512) >> 10: luma on the 8-bit scale, so a threshold and a sum mean the same at either depth
template <typename T>
__device__ __forceinline__ int luma_of(unsigned r, unsigned g, unsigned b) {
    return (int)luma601<T>(r, g, b);
}

template <typename T, int NW>
__device__ __forceinline__ unsigned sample_of(const unsigned (&w)[NW], int j) {
    constexpr int SPW = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    return (w[j / SPW] >> (BITS * (j % SPW))) & ((1u << BITS) - 1);
}

}  // namespace

// sum |luma(a) - luma(b)| over the npix pixels of two [npix][3] frames of samples of T, exact.  A lane takes groups of 3 * WORDS 32-bit
// words = 4 * WORDS pixels of uint8, 2 * WORDS of uint16 (the samples of a pixel straddle the words; twelve bytes hold four | two whole
// pixels): WORDS = 4 reads 16 bytes at a time, WORDS = 1 reads 4, WORDS = 0 reads none; the pixels behind the last whole group (npix is a
// multiple of nothing) go sample by sample.
// Lanes -> wave (shuffles) -> block (LDS) -> scratch[0] (one atomic per block); the block that draws the last ticket of scratch[1]
// takes the total, leaves both words zero for the next launch and decides (SceneDecision).  Integer sums: any order gives the same value.
template <typename T, int WORDS>
__global__ __launch_bounds__(256) void stream_scene_sad_kernel(const T* __restrict__ a, const T* __restrict__ b, size_t npix,
                                                               unsigned long long* __restrict__ scratch, SceneDecision d) {
    constexpr int NW = WORDS ? 3 * WORDS : 1, PPG = 4 * WORDS / (int)sizeof(T);   // pixels per group
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    const size_t ngroups = WORDS ? npix / (PPG ? PPG : 1) : 0;
    unsigned long long sum = 0;
    if constexpr (WORDS != 0) {
        const uint8_t* const ab = reinterpret_cast<const uint8_t*>(a);
        const uint8_t* const bb = reinterpret_cast<const uint8_t*>(b);
        for (size_t g = gid; g < ngroups; g += nthreads) {
            unsigned wa[NW], wb[NW];
            if constexpr (WORDS == 4) {
                const u32x4* const pa = reinterpret_cast<const u32x4*>(ab + g * 48);
                const u32x4* const pb = reinterpret_cast<const u32x4*>(bb + g * 48);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const u32x4 qa = pa[k], qb = pb[k];
                    wa[4 * k] = qa.x, wa[4 * k + 1] = qa.y, wa[4 * k + 2] = qa.z, wa[4 * k + 3] = qa.w;
                    wb[4 * k] = qb.x, wb[4 * k + 1] = qb.y, wb[4 * k + 2] = qb.z, wb[4 * k + 3] = qb.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    wa[k] = reinterpret_cast<const unsigned*>(ab + g * (12 * WORDS))[k];
                    wb[k] = reinterpret_cast<const unsigned*>(bb + g * (12 * WORDS))[k];
                }
            }
            unsigned part = 0;                                    // at most 16 * 219
#pragma unroll
            for (int p = 0; p < PPG; ++p) {
                const int ya = luma_of<T>(sample_of<T>(wa, 3 * p), sample_of<T>(wa, 3 * p + 1), sample_of<T>(wa, 3 * p + 2));
                const int yb = luma_of<T>(sample_of<T>(wb, 3 * p), sample_of<T>(wb, 3 * p + 1), sample_of<T>(wb, 3 * p + 2));
                part += (unsigned)(ya > yb ? ya - yb : yb - ya);
            }
            sum += part;
        }
    }
    for (size_t p = ngroups * PPG + gid; p < npix; p += nthreads) {
        const int ya = luma_of<T>(a[3 * p], a[3 * p + 1], a[3 * p + 2]), yb = luma_of<T>(b[3 * p], b[3 * p + 1], b[3 * p + 2]);
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

namespace {

template <typename T>
hipError_t launch_sad(const T* a, const T* b, size_t npix, unsigned long long* scratch, const SceneDecision& d, hipStream_t s) {
    if (!npix || !scratch || !d.sad) return hipErrorInvalidValue;
    const uintptr_t align = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
    if (align % sizeof(T)) return hipErrorInvalidValue;
    const int words = (npix * 3 * sizeof(T)) % 16 == 0 && align % 16 == 0 ? 4 : (align % 4 == 0 ? 1 : 0);
    const size_t ppg = 4 * words / sizeof(T);
    const size_t ngroups = words ? npix / ppg : 0, rest = npix - ngroups * ppg;
    const size_t items = ngroups > rest ? ngroups : rest;
    const int blocks = (int)((items + 255) / 256 < 1024 ? (items + 255) / 256 : 1024);
    if (words == 4)
        hipLaunchKernelGGL((stream_scene_sad_kernel<T, 4>), dim3(blocks), dim3(256), 0, s, a, b, npix, scratch, d);
    else if (words == 1)
        hipLaunchKernelGGL((stream_scene_sad_kernel<T, 1>), dim3(blocks), dim3(256), 0, s, a, b, npix, scratch, d);
    else
        hipLaunchKernelGGL((stream_scene_sad_kernel<T, 0>), dim3(blocks), dim3(256), 0, s, a, b, npix, scratch, d);
    return hipGetLastError();
}

}  // namespace

// a, b: frames of npix pixels; scratch: two zeroed 64-bit words that every launch leaves zeroed (launches that share them must not overlap)
hipError_t launch_scene_sad_u8(const uint8_t* a, const uint8_t* b, size_t npix, unsigned long long* scratch, const SceneDecision& d,
                               hipStream_t s) {
    return launch_sad<uint8_t>(a, b, npix, scratch, d, s);
}

hipError_t launch_scene_sad_u10(const uint16_t* a, const uint16_t* b, size_t npix, unsigned long long* scratch, const SceneDecision& d,
                                hipStream_t s) {
    return launch_sad<uint16_t>(a, b, npix, scratch, d, s);
}

hipError_t launch_scene_first_frame(unsigned long long* sad, long long* scene_first, int slot, hipStream_t s) {
    hipLaunchKernelGGL(stream_scene_first_frame_kernel, dim3(1), dim3(1), 0, s, sad, scene_first, slot);
    return hipGetLastError();
}

}  // namespace pfnl
