// The words a lane of the field kernels moves (deinterlace.hip, telecine.hip): the rules have no horizontal term, so a row is a flat run of
// 3 W samples and a lane owns 16 bytes of it, 4 bytes, or one sample - the form is read off the addresses - as pairs of 16-bit lanes, two
// samples per packed instruction.  Device code: included by the two .hip files alone.
#pragma once
#include "sample_depth.h"

namespace pfnl {

namespace {

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ s16x2 lanes_of(unsigned w) { return __builtin_bit_cast(s16x2, w); }
__device__ __forceinline__ unsigned word_of_lanes(s16x2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ s16x2 vmax(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ s16x2 vmin(s16x2 a, s16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ s16x2 vabsdiff(s16x2 a, s16x2 b) { return vmax(a - b, b - a); }

// A 32-bit word of samples <-> NP pairs of 16-bit lanes.  Samples are handled alone, so bytes 0 | 2 and 1 | 3 of a word share a pair: two
// masks apart, one OR together.  A uint16 word is its pair, each sample min(v, 1023) as every 10-bit input edge takes it.
template <typename T>
struct Lanes;
template <>
struct Lanes<uint8_t> {
    static constexpr int NP = 2;
    static __device__ __forceinline__ void unpack(unsigned w, s16x2* v) { v[0] = lanes_of(w & 0x00FF00FFu), v[1] = lanes_of((w >> 8) & 0x00FF00FFu); }
    static __device__ __forceinline__ unsigned pack(const s16x2* v) { return word_of_lanes(v[0]) | (word_of_lanes(v[1]) << 8); }
};
template <>
struct Lanes<uint16_t> {
    static constexpr int NP = 1;
    static __device__ __forceinline__ void unpack(unsigned w, s16x2* v) {
        v[0] = __builtin_bit_cast(s16x2, __builtin_elementwise_min(__builtin_bit_cast(u16x2, w), (u16x2)(1023)));
    }
    static __device__ __forceinline__ unsigned pack(const s16x2* v) { return word_of_lanes(v[0]); }
};

// WB: the bytes a lane moves per row - 16, 4, or sizeof(T) (one sample, in the low lane of its pair)
template <typename T, int WB>
struct Word {
    static constexpr int NW = WB == 16 ? 4 : 1, NV = NW * Lanes<T>::NP;
    static __device__ __forceinline__ void load(const uint8_t* p, s16x2* v) {
        unsigned w[NW];
        if constexpr (WB == 16) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(p);
            w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
        } else if constexpr (WB == 4) {
            w[0] = *reinterpret_cast<const unsigned*>(p);
        } else {
            w[0] = *reinterpret_cast<const T*>(p);
        }
#pragma unroll
        for (int k = 0; k < NW; ++k) Lanes<T>::unpack(w[k], v + k * Lanes<T>::NP);
    }
    static __device__ __forceinline__ void store(uint8_t* p, const s16x2* v) {
        unsigned w[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = Lanes<T>::pack(v + k * Lanes<T>::NP);
        if constexpr (WB == 16)
            *reinterpret_cast<u32x4*>(p) = u32x4{w[0], w[1], w[2], w[3]};
        else if constexpr (WB == 4)
            *reinterpret_cast<unsigned*>(p) = w[0];
        else
            *reinterpret_cast<T*>(p) = (T)w[0];
    }
};

}  // namespace

}  // namespace pfnl
