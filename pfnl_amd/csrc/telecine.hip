// INVERSE TELECINE (include/pfnl_hip.h TELECINE; the rule: pfnl_amd/telecine.py; index rules: telecine_geom.h): the kept field A and its two
// candidate partners Xc, Xp - tight [H/2][W][3] samples each - -> both comb counts and the decision, then the matched frame [H][W][3].
// Two launches, no host round trip between them: the second reads the decision the first left in device memory.
//   1. telecine_match_kernel.  The rule has no horizontal term, so a row is a flat run of 3 W samples: a lane owns ONE word of the row
//      (16 bytes, or 4, or one sample: read off the addresses, field_words.h) and walks down a strip of TC_STRIP_ROWS field rows with A's two
//      neighbour rows in registers - A[u + 1] is the next row's A[u] -, reading Xc[j] and Xp[j] once: both counts in one pass over A, Xc, Xp.
//      8 bits: a, b and |a| |b| <= 65 025 fit packed 16-bit lanes - combed iff a, b have one sign and |a| |b| > T^2 -, two samples per
//      instruction.  10 bits: the product needs 32 bits and is taken per sample.  Lanes -> wave (shuffles) -> workgroup (LDS) -> ONE 64-bit
//      atomic per workgroup on a word that holds both counts (c low, p high; a count is at most h 3 W < 2^32: the launcher checks); the
//      workgroup that draws the last ticket takes the totals, leaves both scratch words zero for the next launch and writes the decision.
//   2. telecine_weave_kernel.  The same lanes and strips.  Not post-flagged: rows 2 j + p = A[j] and 2 j + 1 - p = X[j] of the chosen partner
//      leave as whole words.  Post-flagged: `out` already holds the deinterlaced frame (deinterlace.hip ran into it) and is left alone.
//      With `prev` the same pass sums |m_n - m_(n-1)| over all samples - of the rows just made, or of the rows read back where flagged - and
//      the last workgroup stores D_n; the reduction is the match kernel's.
// Integer sums: any order gives the same value.
#include "field_words.h"
#include "telecine_geom.h"

namespace pfnl {

namespace {

constexpr int TC_BLOCK = 256;
constexpr int TC_STRIP_ROWS = 4;                                  // a lane walks down this many field rows; the next strip re-reads one row of A

// sum over the workgroup; the value is valid in thread 0
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __shared__ unsigned long long wave_sum[TC_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long total = 0;
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < TC_BLOCK / 64; ++k) total += wave_sum[k];
    return total;
}

// thread 0 of every workgroup: adds `part` to scratch[0] and draws a ticket of scratch[1]; true in the one that drew the last, with the
// total in *total and both words zero again
__device__ __forceinline__ bool last_block_total(unsigned long long* scratch, unsigned long long part, unsigned long long* total) {
    atomicAdd(&scratch[0], part);
    __threadfence();                                              // the workgroup's sum is visible before its ticket is
    if (atomicAdd(&scratch[1], 1ull) != gridDim.x - 1) return false;
    *total = atomicExch(&scratch[0], 0ull);
    atomicExch(&scratch[1], 0ull);
    return true;
}

// how many of the 2 * NV samples of a word are combed: X beside its vertical neighbours lo = A[u], hi = A[u + 1]
// (a single sample is loaded into the low lane of its pair: the high lane of every operand is then 0 and counts nothing)
template <typename T, int NV>
__device__ __forceinline__ unsigned combed(const s16x2* x, const s16x2* lo, const s16x2* hi, int t2) {
    unsigned n = 0;
    if constexpr (sizeof(T) == 1) {
        s16x2 hits = (s16x2)(0);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const s16x2 a = x[k] - lo[k], b = x[k] - hi[k];
            const u16x2 prod = __builtin_bit_cast(u16x2, vmax(a, -a)) * __builtin_bit_cast(u16x2, vmax(b, -b));
            const s16x2 one_sign = (a ^ b) >= (s16x2)(0), over = __builtin_bit_cast(s16x2, prod > (u16x2)((unsigned short)t2));
            hits -= one_sign & over;                              // a comparison's lanes are 0 or -1
        }
        n = (unsigned)(hits.x + hits.y);
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int a0 = x[k].x - lo[k].x, b0 = x[k].x - hi[k].x, a1 = x[k].y - lo[k].y, b1 = x[k].y - hi[k].y;
            n += (unsigned)(a0 * b0 > t2) + (unsigned)(a1 * b1 > t2);
        }
    }
    return n;
}

template <int NV>
__device__ __forceinline__ unsigned abs_diff_sum(const s16x2* a, const s16x2* b) {
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const s16x2 d = vabsdiff(a[k], b[k]);
        n += (unsigned)d.x + (unsigned)d.y;
    }
    return n;
}

}  // namespace

// Lane t: word t % words of the row, strip t / words of the h field rows.
template <typename T, int WB>
__global__ __launch_bounds__(TC_BLOCK) void telecine_match_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Xc,
                                                                  const uint8_t* __restrict__ Xp, int h, size_t row_bytes, int p, int t2,
                                                                  unsigned long long* __restrict__ scratch, TelecineDecide d) {
    typedef Word<T, WB> Wd;
    constexpr int NV = Wd::NV;
    const size_t words = row_bytes / WB, strips = ((size_t)h + TC_STRIP_ROWS - 1) / TC_STRIP_ROWS, total = words * strips;
    const auto row = [&](const uint8_t* f, int i) { return f + (size_t)(i < 0 ? 0 : (i > h - 1 ? h - 1 : i)) * row_bytes; };
    unsigned nc = 0, np = 0;                                          // at most h 3 W each
    for (size_t t = (size_t)blockIdx.x * TC_BLOCK + threadIdx.x; t < total; t += (size_t)gridDim.x * TC_BLOCK) {
        const size_t at = t % words * WB;
        const int j0 = (int)(t / words) * TC_STRIP_ROWS, j1 = j0 + TC_STRIP_ROWS < h ? j0 + TC_STRIP_ROWS : h;
        s16x2 lo[NV], hi[NV], xc[NV], xp[NV];
        int u = j0 - p;
        Wd::load(row(A, u) + at, lo);
        for (int j = j0; j < j1; ++j, ++u) {
            Wd::load(row(A, u + 1) + at, hi);
            Wd::load(Xc + (size_t)j * row_bytes + at, xc);
            Wd::load(Xp + (size_t)j * row_bytes + at, xp);
            nc += combed<T, NV>(xc, lo, hi, t2);
            np += combed<T, NV>(xp, lo, hi, t2);
#pragma unroll
            for (int k = 0; k < NV; ++k) lo[k] = hi[k];
        }
    }
    const unsigned long long part = block_sum((unsigned long long)nc | ((unsigned long long)np << 32));
    if (threadIdx.x != 0) return;
    unsigned long long both = 0;
    if (!last_block_total(scratch, part, &both)) return;
    const unsigned long long count_c = both & 0xffffffffull, count_p = both >> 32;
    const unsigned long long match = count_p < count_c ? 1 : 0, least = match ? count_p : count_c;
    const unsigned long long post = d.post && least > d.comb_limit ? 1 : 0;
    d.decision[0] = count_c, d.decision[1] = count_p, d.decision[2] = match, d.decision[3] = post;
    if (d.stats) d.stats[post ? 2 : match] += 1;                      // launches that share `stats` do not overlap
}

template <typename T, int WB>
__global__ __launch_bounds__(TC_BLOCK) void telecine_weave_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Xc,
                                                                  const uint8_t* __restrict__ Xp, uint8_t* out, const uint8_t* __restrict__ prev,
                                                                  int h, size_t row_bytes, int p, const unsigned long long* __restrict__ decision,
                                                                  unsigned long long* __restrict__ scratch, unsigned long long* __restrict__ dist) {
    typedef Word<T, WB> Wd;
    constexpr int NV = Wd::NV;
    const size_t words = row_bytes / WB, strips = ((size_t)h + TC_STRIP_ROWS - 1) / TC_STRIP_ROWS, total = words * strips;
    const uint8_t* const X = decision[2] ? Xp : Xc;
    const bool flagged = decision[3] != 0;
    unsigned long long sum = 0;
    if (!flagged || prev) {
        for (size_t t = (size_t)blockIdx.x * TC_BLOCK + threadIdx.x; t < total; t += (size_t)gridDim.x * TC_BLOCK) {
            const size_t at = t % words * WB;
            const int j0 = (int)(t / words) * TC_STRIP_ROWS, j1 = j0 + TC_STRIP_ROWS < h ? j0 + TC_STRIP_ROWS : h;
            unsigned part = 0;                                        // at most TC_STRIP_ROWS * 2 * 16 * 1023
            for (int j = j0; j < j1; ++j) {
                const size_t kept = (size_t)(2 * j + p) * row_bytes + at, made = (size_t)(2 * j + 1 - p) * row_bytes + at;
                s16x2 a[NV], x[NV], q[NV];
                if (flagged) {
                    Wd::load(out + kept, a);
                    Wd::load(out + made, x);
                } else {
                    Wd::load(A + (size_t)j * row_bytes + at, a);
                    Wd::load(X + (size_t)j * row_bytes + at, x);
                    Wd::store(out + kept, a);
                    Wd::store(out + made, x);
                }
                if (prev) {
                    Wd::load(prev + kept, q);
                    part += abs_diff_sum<NV>(a, q);
                    Wd::load(prev + made, q);
                    part += abs_diff_sum<NV>(x, q);
                }
            }
            sum += part;
        }
    }
    if (!dist) return;
    const unsigned long long part = block_sum(sum);
    if (threadIdx.x != 0) return;
    unsigned long long all = 0;
    if (last_block_total(scratch, part, &all)) *dist = prev ? all : TC_D_FIRST;
}

namespace {

// 16, 4 or sizeof(T): the widest word every address and the row allow; 0: a pointer that no sample can have
template <typename T>
int word_bytes(size_t row_bytes, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = row_bytes;
    for (const void* ptr : ptrs) bits |= reinterpret_cast<uintptr_t>(ptr);
    if (bits % sizeof(T)) return 0;
    return bits % 16 == 0 ? 16 : (bits % 4 == 0 ? 4 : (int)sizeof(T));
}

unsigned grid_of(size_t row_bytes, int wb, int h) {
    const size_t lanes = row_bytes / wb * (((size_t)h + TC_STRIP_ROWS - 1) / TC_STRIP_ROWS), blocks = (lanes + TC_BLOCK - 1) / TC_BLOCK;
    return (unsigned)(blocks < 4096 ? blocks : 4096);
}

template <typename T>
hipError_t match_of(const T* A, const T* Xc, const T* Xp, int h, int W, int parity, int threshold, unsigned long long* scratch, const TelecineDecide& d,
                    hipStream_t s) {
    if (!A || !Xc || !Xp || !scratch || !d.decision || h < 1 || W < 1 || (parity != 0 && parity != 1) || threshold < 1 || threshold > 255)
        return hipErrorInvalidValue;
    if ((unsigned long long)h * 3ull * (unsigned long long)W >= (1ull << 32)) return hipErrorInvalidValue;   // a count fits its half of the word
    const size_t row_bytes = (size_t)W * 3 * sizeof(T);
    const int wb = word_bytes<T>(row_bytes, {A, Xc, Xp});
    if (!wb || (reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(d.decision) | reinterpret_cast<uintptr_t>(d.stats)) % 8)
        return hipErrorInvalidValue;
    const int t = threshold * (sizeof(T) == 1 ? 1 : 4), t2 = t * t;
    const uint8_t *a = reinterpret_cast<const uint8_t*>(A), *xc = reinterpret_cast<const uint8_t*>(Xc), *xp = reinterpret_cast<const uint8_t*>(Xp);
    const dim3 grid(grid_of(row_bytes, wb, h)), block(TC_BLOCK);
    if (wb == 16)
        hipLaunchKernelGGL((telecine_match_kernel<T, 16>), grid, block, 0, s, a, xc, xp, h, row_bytes, parity, t2, scratch, d);
    else if (wb == 4)
        hipLaunchKernelGGL((telecine_match_kernel<T, 4>), grid, block, 0, s, a, xc, xp, h, row_bytes, parity, t2, scratch, d);
    else
        hipLaunchKernelGGL((telecine_match_kernel<T, (int)sizeof(T)>), grid, block, 0, s, a, xc, xp, h, row_bytes, parity, t2, scratch, d);
    return hipGetLastError();
}

template <typename T>
hipError_t weave_of(const T* A, const T* Xc, const T* Xp, int h, int W, int parity, const unsigned long long* decision, T* out, const T* prev,
                    unsigned long long* scratch, unsigned long long* dist, hipStream_t s) {
    if (!A || !Xc || !Xp || !decision || !out || h < 1 || W < 1 || (parity != 0 && parity != 1) || (dist && !scratch)) return hipErrorInvalidValue;
    const size_t row_bytes = (size_t)W * 3 * sizeof(T);
    const int wb = word_bytes<T>(row_bytes, {A, Xc, Xp, out, prev});
    if (!wb || (reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(decision) | reinterpret_cast<uintptr_t>(dist)) % 8)
        return hipErrorInvalidValue;
    const uint8_t *a = reinterpret_cast<const uint8_t*>(A), *xc = reinterpret_cast<const uint8_t*>(Xc), *xp = reinterpret_cast<const uint8_t*>(Xp);
    uint8_t* const o = reinterpret_cast<uint8_t*>(out);
    const uint8_t* const q = reinterpret_cast<const uint8_t*>(prev);
    const dim3 grid(grid_of(row_bytes, wb, h)), block(TC_BLOCK);
    if (wb == 16)
        hipLaunchKernelGGL((telecine_weave_kernel<T, 16>), grid, block, 0, s, a, xc, xp, o, q, h, row_bytes, parity, decision, scratch, dist);
    else if (wb == 4)
        hipLaunchKernelGGL((telecine_weave_kernel<T, 4>), grid, block, 0, s, a, xc, xp, o, q, h, row_bytes, parity, decision, scratch, dist);
    else
        hipLaunchKernelGGL((telecine_weave_kernel<T, (int)sizeof(T)>), grid, block, 0, s, a, xc, xp, o, q, h, row_bytes, parity, decision, scratch, dist);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_telecine_match(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, int threshold,
                                 unsigned long long* scratch, const TelecineDecide& d, hipStream_t s) {
    return match_of(A, Xc, Xp, h, W, parity, threshold, scratch, d, s);
}
hipError_t launch_telecine_match(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity, int threshold,
                                 unsigned long long* scratch, const TelecineDecide& d, hipStream_t s) {
    return match_of(A, Xc, Xp, h, W, parity, threshold, scratch, d, s);
}
hipError_t launch_telecine_weave(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, const unsigned long long* decision,
                                 uint8_t* out, const uint8_t* prev, unsigned long long* scratch, unsigned long long* dist, hipStream_t s) {
    return weave_of(A, Xc, Xp, h, W, parity, decision, out, prev, scratch, dist, s);
}
hipError_t launch_telecine_weave(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity, const unsigned long long* decision,
                                 uint16_t* out, const uint16_t* prev, unsigned long long* scratch, unsigned long long* dist, hipStream_t s) {
    return weave_of(A, Xc, Xp, h, W, parity, decision, out, prev, scratch, dist, s);
}

}  // namespace pfnl
