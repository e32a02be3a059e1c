// Stage 0 of the streaming session's output route with a colour conversion in it (include/pfnl_hip.h COLOUR; the rule: pfnl_amd/colour.py;
// its integers: colour_geom.h): the fp32 result is quantised exactly as misc_kernels.hip quantise_kernel does, and the levels of a pixel go
// through D -> the 3 x 3 gamut matrix in int32 -> E before they are stored.  The launch reads every fp32 value and writes every sample
// once, as the plain quantise does: the conversion moves no extra byte of device memory.
#include <mutex>

#include "colour_geom.h"
#include "sample_depth.h"

namespace pfnl {

constexpr int COLOUR_MAX_BLOCKS = 1024;                               // the grid strides: a workgroup loads the tables once, 3 or 6 KB

// One body over the sample type.  A lane takes 4 pixels - three 16-byte loads, 12 samples stored in whole words (three 4-byte words of
// uint8, three 8-byte words of uint16).  tab: colour_blob of the depth, [D][start][threshold] uint16, copied into LDS by the workgroup;
// the table reads are gathers by value, so their bank conflicts follow the picture.  n4: pixels / 4.
template <typename T>
__global__ __launch_bounds__(256) void quantise_colour_kernel(const f32x4* __restrict__ sr, T* __restrict__ out, size_t n4,
                                                              const uint32_t* __restrict__ tab, ColourMatrix m) {
    constexpr int LEVELS = Depth<T>::LEVELS, WORDS = 2 * LEVELS + COLOUR_BUCKETS;
    constexpr float TOP = (float)(LEVELS - 1);
    __shared__ uint32_t lds[WORDS / 2];
    for (int i = threadIdx.x; i < WORDS / 2; i += 256) lds[i] = tab[i];
    __syncthreads();
    const uint16_t* const D = reinterpret_cast<const uint16_t*>(lds);
    const uint16_t* const start = D + LEVELS;
    const uint16_t* const threshold = start + COLOUR_BUCKETS;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 a = sr[3 * i], b = sr[3 * i + 1], c = sr[3 * i + 2];
        const float x[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        const auto level = [](float v) { return (int)(uint32_t)rintf(fminf(fmaxf(v * TOP, 0.f), TOP)); };   // quantise_kernel's: NaN -> 0
        int q[12];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = D[level(x[3 * p])], g = D[level(x[3 * p + 1])], bl = D[level(x[3 * p + 2])];
#pragma unroll
            for (int k = 0; k < 3; ++k) {                             // at most 18224 * 65535 + 2^13: int32 holds it (colour.py)
                const int l = shift_clip<COLOUR_FRAC, COLOUR_LINEAR>(m.m[3 * k] * r + m.m[3 * k + 1] * g + m.m[3 * k + 2] * bl + (1 << (COLOUR_FRAC - 1)));
                q[3 * p + k] = encode_lookup<LEVELS>(start, threshold, l);
            }
        }
        store_samples<T, 12, true>(out + 12 * i, q);
    }
}

namespace {

template <typename T>
hipError_t launch_as(const float* sr, T* out, size_t pixels, const uint16_t* tab, const ColourMatrix& m, hipStream_t s) {
    if (!sr || !out || !tab || !pixels || pixels % 4 || reinterpret_cast<uintptr_t>(sr) % 16 || reinterpret_cast<uintptr_t>(out) % 8 ||
        reinterpret_cast<uintptr_t>(tab) % 4)
        return hipErrorInvalidValue;
    const size_t n4 = pixels / 4, blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(quantise_colour_kernel<T>, dim3((unsigned)(blocks < COLOUR_MAX_BLOCKS ? blocks : COLOUR_MAX_BLOCKS)), dim3(256), 0, s,
                       reinterpret_cast<const f32x4*>(sr), out, n4, reinterpret_cast<const uint32_t*>(tab), m);
    return hipGetLastError();
}

}  // namespace

// The tables of both depths on the current device, [colour_blob(8)][colour_blob(10)]: uploaded by the first call that asks for them on that
// device and kept for the life of the process (9 KB), so neither a session nor a hook owns them and every launch after the first finds them.
hipError_t colour_device_tables(const uint16_t** tab8, const uint16_t** tab10) {
    constexpr int MAX_DEVICES = 64;
    static std::mutex lock;
    static uint16_t* held[MAX_DEVICES] = {};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= MAX_DEVICES) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> g(lock);
    if (!held[dev]) {
        std::vector<uint16_t> blob, blob10;
        colour_blob(8, &blob);
        colour_blob(10, &blob10);
        blob.insert(blob.end(), blob10.begin(), blob10.end());
        uint16_t* tab = nullptr;
        if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&tab), blob.size() * sizeof(uint16_t))) return e;
        hipError_t e;
        {
            BlockingCopyGuard guard;                                  // (never beside another handle's graph capture: common.h)
            e = hipMemcpy(tab, blob.data(), blob.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            (void)hipFree(tab);
            return e;
        }
        held[dev] = tab;
    }
    *tab8 = held[dev];
    *tab10 = held[dev] + colour_blob_words(8);
    return hipSuccess;
}

hipError_t launch_quantise_colour(const float* sr, uint8_t* out, size_t pixels, const uint16_t* tab, const ColourMatrix& m, hipStream_t s) {
    return launch_as(sr, out, pixels, tab, m, s);
}

hipError_t launch_quantise_colour(const float* sr, uint16_t* out, size_t pixels, const uint16_t* tab, const ColourMatrix& m, hipStream_t s) {
    return launch_as(sr, out, pixels, tab, m, s);
}

}  // namespace pfnl
