// The sample depth of the streaming session's two edges, and the device primitives their stages share (misc_kernels.hip quantise,
// place.hip resample, yuv.hip 4:2:0 both ways, stream.hip ring): 8 bits in uint8_t samples, 10 bits (0 .. 1023) in uint16_t samples.  A stage is one body over the
// sample type T; what differs between the depths is in Depth<T> and in the width of a sample.
#pragma once
#include "common.h"

namespace pfnl {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <typename T>
struct Depth;
template <>
struct Depth<uint8_t> {
    static constexpr int LEVELS = 256, CHROMA = 128;                   // sample values 0 .. 255; the chroma offset
    static constexpr int HS = 8, VS = 20;                              // the resampler: (+2^7) >> 8 into the int16 intermediate, then (+2^19) >> 20
};
template <>
struct Depth<uint16_t> {
    static constexpr int LEVELS = 1024, CHROMA = 512;
    static constexpr int HS = 10, VS = 18;                             // (+2^9) >> 10, then (+2^17) >> 18
};

// clip(v >> S, 0, LEVELS - 1) with the clamp AHEAD of the shift (the same value: both are monotonic).  Every clip of the edge is this one.
// Written as shift-then-clamp, two 8-bit results that are packed into neighbouring bytes become one v_ashr_pk_u8_i32 (new on gfx950), which
// the compiler ORs with bytes 2 and 3 as if the instruction left the upper half of its result zero.  With that code the 4-pixel NV12
// decode delivered wrong bytes 2 of its packed words on the device (values no input can produce) and right ones in a host build of the
// same source: tools/GFX950_NOTES.md.  Results of either depth that are packed into one word invite these packed shift-and-clamp
// instructions, so no stage writes the other order.
template <int S, int LEVELS>
__device__ __forceinline__ int shift_clip(int v) {
    v = v < 0 ? 0 : v;
    v = v > (LEVELS << S) - 1 ? (LEVELS << S) - 1 : v;
    return v >> S;
}

// Integer BT.601 luma of one RGB pixel on the 8-BIT scale without its + 16 - black is 0, white 219 | 220 - at either depth: pfnl_amd/scene.py
// luma_u8, and luma_u10 on values clamped onto 1023.  The scene sums (stream.hip) and the content box (bars.hip) read frames through it.
template <typename T>
__device__ __forceinline__ unsigned luma601(unsigned r, unsigned g, unsigned b) {
    if constexpr (sizeof(T) == 1) {
        return (66u * r + 129u * g + 25u * b + 128u) >> 8;
    } else {
        r = r > 1023u ? 1023u : r, g = g > 1023u ? 1023u : g, b = b > 1023u ? 1023u : b;
        return (66u * r + 129u * g + 25u * b + 512u) >> 10;
    }
}

// the widest word, in bytes, that divides N samples of T: the strips are laid out so that a run of N samples is aligned to it in the
// forms that use words
template <typename T, int N>
constexpr int word_of() {
    constexpr int B = N * (int)sizeof(T);
    return B % 16 == 0 ? 16 : (B % 8 == 0 ? 8 : (B % 4 == 0 ? 4 : (B % 2 == 0 ? 2 : 1)));
}

// N samples at p -> v[0 .. N), each sample >> SH (P010 keeps its values in the upper ten bits: the shift is part of the load, and the low
// six bits are ignored), in words (WORDS) or sample by sample
template <typename T, int N, bool WORDS, int SH = 0>
__device__ __forceinline__ void load_samples(const T* __restrict__ p, int* v) {
    constexpr int SZ = (int)sizeof(T), BITS = 8 * SZ, SPW = 4 / SZ, WB = WORDS ? word_of<T, N>() : SZ;   // SPW: samples per 32 bits
    constexpr unsigned MASK = (1u << BITS) - 1;
    static_assert(SH == 0 || SZ == 2, "only 16-bit samples are loaded shifted");
    if constexpr (WB == SZ) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = p[k] >> SH;
    } else if constexpr (WB == 2) {                                    // (two bytes)
#pragma unroll
        for (int k = 0; k < N; k += 2) {
            const unsigned w = *reinterpret_cast<const uint16_t*>(p + k);
            v[k] = (int)(w & 255u), v[k + 1] = (int)(w >> 8);
        }
    } else {
        unsigned w[N / SPW];
#pragma unroll
        for (int k = 0; k < N / SPW; k += WB / 4) {
            if constexpr (WB == 16) {
                const u32x4 q = *reinterpret_cast<const u32x4*>(p + SPW * k);
                w[k] = q.x, w[k + 1] = q.y, w[k + 2] = q.z, w[k + 3] = q.w;
            } else if constexpr (WB == 8) {
                const u32x2 q = *reinterpret_cast<const u32x2*>(p + SPW * k);
                w[k] = q.x, w[k + 1] = q.y;
            } else {
                w[k] = *reinterpret_cast<const unsigned*>(p + SPW * k);
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = (int)(((w[k / SPW] >> (BITS * (k % SPW))) & MASK) >> SH);
    }
}

// load_samples as an input edge takes a caller's samples: values of at most LEVELS - 1 whatever the memory holds.  8 bits: every byte is a
// value.  16 bits: >> 6 leaves ten bits (P010); unshifted samples (I010, RGB10) clamp onto 1023 - no multiply and no table index ever
// sees more (pfnl_amd/depth10.py values10).
template <typename T, int N, bool WORDS, int SH = 0>
__device__ __forceinline__ void load_values(const T* __restrict__ p, int* v) {
    load_samples<T, N, WORDS, SH>(p, v);
    if constexpr (sizeof(T) == 2 && SH == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = v[k] > Depth<T>::LEVELS - 1 ? Depth<T>::LEVELS - 1 : v[k];
    }
}

// v[0 .. N), each a sample value -> N samples at p, each v << SH (P010 keeps its values in the upper ten bits: the shift is part of the store)
template <typename T, int N, bool WORDS, int SH = 0>
__device__ __forceinline__ void store_samples(T* __restrict__ p, const int* v) {
    constexpr int SZ = (int)sizeof(T), BITS = 8 * SZ, SPW = 4 / SZ, WB = WORDS ? word_of<T, N>() : SZ;
    static_assert(SH == 0 || SZ == 2, "only 16-bit samples are stored shifted");
    if constexpr (WB == SZ) {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = (T)(v[k] << SH);
    } else if constexpr (WB == 2) {                                    // (two bytes)
#pragma unroll
        for (int k = 0; k < N; k += 2) *reinterpret_cast<uint16_t*>(p + k) = (uint16_t)(v[k] | (v[k + 1] << 8));
    } else {
        unsigned w[N / SPW];
#pragma unroll
        for (int k = 0; k < N / SPW; ++k) {
            w[k] = (unsigned)v[SPW * k] << SH;
#pragma unroll
            for (int j = 1; j < SPW; ++j) w[k] |= (unsigned)v[SPW * k + j] << (BITS * j + SH);
        }
#pragma unroll
        for (int k = 0; k < N / SPW; k += WB / 4) {
            if constexpr (WB == 16)
                *reinterpret_cast<u32x4*>(p + SPW * k) = u32x4{w[k], w[k + 1], w[k + 2], w[k + 3]};
            else if constexpr (WB == 8)
                *reinterpret_cast<u32x2*>(p + SPW * k) = u32x2{w[k], w[k + 1]};
            else
                *reinterpret_cast<unsigned*>(p + SPW * k) = w[k];
        }
    }
}

}  // namespace pfnl
