// The content box of RGB frames (include/pfnl_hip.h BARS; the rule: pfnl_amd/bars.py, its integer steps: bars_geom.h): the sums of luma
// along every row and every column of a frame, and from them the box between the first and the last picture row and column - where the
// picture lies inside letterbox or pillarbox bars.  One launch for n frames, no host round trip; one kernel body over the sample type.
// Integer sums: any order of accumulation gives the same value.
#include "bars_geom.h"
#include "sample_depth.h"

namespace pfnl {

namespace {

constexpr int BARS_THREADS = 256;
constexpr int BARS_STRIP = 8;                         // rows of a workgroup's strip
constexpr int BARS_SCAN_AT_ONCE = 8;                  // sums a thread of the last workgroup holds before it compares them
constexpr int BARS_ROWS_AT_ONCE = 4;                  // rows whose words a lane holds before it sums them: twelve 16-byte reads in flight

// the words of one group of pixels at p: WORDS = 4: three 16-byte reads (16 pixels of uint8, 8 of uint16), WORDS = 1: three 4-byte reads
// (4 | 2 pixels), WORDS = 0: the three samples of one pixel
template <typename T, int WORDS, int NW>
__device__ __forceinline__ void load_group(const T* __restrict__ p, unsigned (&w)[NW]) {
    if constexpr (WORDS == 4) {
        const u32x4* const q = reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x4 v = q[k];
            w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
    } else if constexpr (WORDS == 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = reinterpret_cast<const unsigned*>(p)[k];
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = p[k];
    }
}

// sample j of a loaded group
template <typename T, int WORDS, int NW>
__device__ __forceinline__ unsigned group_sample(const unsigned (&w)[NW], int j) {
    if constexpr (WORDS == 0) {
        return w[j];
    } else {
        constexpr int SPW = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        return (w[j / SPW] >> (BITS * (j % SPW))) & ((1u << BITS) - 1);
    }
}

}  // namespace

// frames [n][H][W][3] samples of T -> per frame f = blockIdx.y: rows[f][H], the box and, where asked for, cols[f][W].
// A workgroup owns the strip of BARS_STRIP whole rows blockIdx.x, so a row's sum is complete inside it: lanes -> the lanes of the row in
// the wave (shuffles) -> LDS -> one store per row.  The 256 lanes are TY rows of TX = 2^tx_log2 lanes; a lane owns the pixels of one
// group per pass - W is a multiple of the group in the form the launcher picks - and walks down the strip with their column sums in
// registers; those meet in LDS and leave as one 32-bit add per column, strip and pass, in column order.
// col_sums [n][W] and ticket [n] are zero on entry and on exit: the workgroup that draws a frame's last ticket reads and clears the
// frame's column sums in one exchange, scans both arrays line by line (bars_geom.h), writes the box and clears the ticket.
// Across workgroups (the release / acquire hand-off by counter): every wave drains its stores, the workgroup meets, one lane releases at
// agent scope and draws the ticket; the last one acquires at agent scope before the workgroup reads - and what it reads, it reads with
// agent-scope loads and exchanges, which no stale line of this compute unit's cache can answer.
template <typename T, int WORDS>
__global__ __launch_bounds__(BARS_THREADS) void content_box_kernel(const T* __restrict__ frames, int H, int W, int limit, int tx_log2,
                                                                   uint32_t* __restrict__ col_sums, uint32_t* __restrict__ ticket,
                                                                   uint32_t* __restrict__ rows, uint32_t* __restrict__ cols_out,
                                                                   int32_t* __restrict__ box) {
    constexpr int PPG = WORDS ? 4 * WORDS / (int)sizeof(T) : 1;   // pixels per group
    constexpr int NW = WORDS ? 3 * WORDS : 3;
    __shared__ uint32_t lds_cols[BARS_THREADS * PPG];
    __shared__ uint32_t lds_rows[BARS_STRIP];
    __shared__ int lds_span[4];
    __shared__ int lds_is_last;
    const int tid = threadIdx.x, TX = 1 << tx_log2, TY = BARS_THREADS >> tx_log2, tx = tid & (TX - 1), ty = tid >> tx_log2;
    const int seg = TX < 64 ? TX : 64;                            // the lanes of a wave that share a row
    const int f = blockIdx.y, r0 = blockIdx.x * BARS_STRIP, r1 = r0 + BARS_STRIP < H ? r0 + BARS_STRIP : H;
    const T* const frame = frames + (size_t)f * H * W * 3;
    const int groups = W / PPG, passes = (groups + TX - 1) / TX;
    if (tid < BARS_STRIP) lds_rows[tid] = 0;
    if (tid == 0) lds_span[0] = H, lds_span[1] = -1, lds_span[2] = W, lds_span[3] = -1;
    for (int pass = 0; pass < passes; ++pass) {
        for (int i = tid; i < TX * PPG; i += BARS_THREADS) lds_cols[i] = 0;
        __syncthreads();
        const int cg = pass * TX + tx;
        const bool col_ok = cg < groups;
        const size_t at = (size_t)(col_ok ? cg : groups - 1) * PPG;   // (a lane past the end reads the last group and adds nothing)
        uint32_t colpart[PPG];
#pragma unroll
        for (int p = 0; p < PPG; ++p) colpart[p] = 0;
        for (int yb = r0; yb < r1; yb += BARS_ROWS_AT_ONCE * TY) {
            unsigned w[BARS_ROWS_AT_ONCE][NW];
#pragma unroll
            for (int u = 0; u < BARS_ROWS_AT_ONCE; ++u) {
                const int y = yb + u * TY + ty;
                load_group<T, WORDS, NW>(frame + ((size_t)(y < r1 ? y : r1 - 1) * W + at) * 3, w[u]);
            }
#pragma unroll
            for (int u = 0; u < BARS_ROWS_AT_ONCE; ++u) {
                const int y = yb + u * TY + ty;
                const bool ok = col_ok && y < r1;
                uint32_t rowpart = 0;
#pragma unroll
                for (int p = 0; p < PPG; ++p) {
                    const unsigned l = luma601<T>(group_sample<T, WORDS, NW>(w[u], 3 * p), group_sample<T, WORDS, NW>(w[u], 3 * p + 1),
                                                  group_sample<T, WORDS, NW>(w[u], 3 * p + 2));
                    colpart[p] += ok ? l : 0u;
                    rowpart += ok ? l : 0u;
                }
                for (int off = seg >> 1; off > 0; off >>= 1) rowpart += __shfl_down(rowpart, off, seg);
                if ((tid & (seg - 1)) == 0 && y < r1 && rowpart) atomicAdd(&lds_rows[y - r0], rowpart);
            }
        }
        if (col_ok) {
#pragma unroll
            for (int p = 0; p < PPG; ++p)
                if (colpart[p]) atomicAdd(&lds_cols[tx * PPG + p], colpart[p]);
        }
        __syncthreads();
        for (int i = tid; i < TX * PPG; i += BARS_THREADS) {
            const int x = pass * TX * PPG + i;
            const uint32_t v = lds_cols[i];
            if (x < W && v) atomicAdd(&col_sums[(size_t)f * W + x], v);
        }
        __syncthreads();
    }
    uint32_t* const rows_f = rows + (size_t)f * H;
    if (tid < r1 - r0) __hip_atomic_store(&rows_f[r0 + tid], lds_rows[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // every wave: its row sums and column adds have left
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (the fence first, then this wait, then the ticket: in this order)
        const unsigned drawn = __hip_atomic_fetch_add(&ticket[f], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lds_is_last = drawn == gridDim.x - 1;
        if (lds_is_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!lds_is_last) return;
    uint32_t* const cols_f = col_sums + (size_t)f * W;
    // BARS_SCAN_AT_ONCE sums of a thread are in flight together: a sum is a round trip to memory, and one after the other they were most
    // of the kernel's time
    int first = H, last = -1;
    const uint32_t row_thr = bars_threshold(limit, W), col_thr = bars_threshold(limit, H);
    for (int base = tid; base < H; base += BARS_THREADS * BARS_SCAN_AT_ONCE) {
        uint32_t v[BARS_SCAN_AT_ONCE];
#pragma unroll
        for (int k = 0; k < BARS_SCAN_AT_ONCE; ++k) {
            const int i = base + k * BARS_THREADS;
            v[k] = i < H ? __hip_atomic_load(&rows_f[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;   // (0 is never picture)
        }
#pragma unroll
        for (int k = 0; k < BARS_SCAN_AT_ONCE; ++k) bars_scan_line(base + k * BARS_THREADS, v[k], row_thr, &first, &last);
    }
    atomicMin(&lds_span[0], first);
    atomicMax(&lds_span[1], last);
    first = W, last = -1;
    for (int base = tid; base < W; base += BARS_THREADS * BARS_SCAN_AT_ONCE) {
        uint32_t v[BARS_SCAN_AT_ONCE];
#pragma unroll
        for (int k = 0; k < BARS_SCAN_AT_ONCE; ++k) {
            const int i = base + k * BARS_THREADS;
            v[k] = i < W ? __hip_atomic_exchange(&cols_f[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
#pragma unroll
        for (int k = 0; k < BARS_SCAN_AT_ONCE; ++k) {
            const int i = base + k * BARS_THREADS;
            if (cols_out && i < W) cols_out[(size_t)f * W + i] = v[k];
            bars_scan_line(i, v[k], col_thr, &first, &last);
        }
    }
    atomicMin(&lds_span[2], first);
    atomicMax(&lds_span[3], last);
    __syncthreads();
    if (tid != 0) return;
    int32_t b[4];
    bars_box(lds_span[0], lds_span[1], lds_span[2], lds_span[3], b);
#pragma unroll
    for (int k = 0; k < 4; ++k) box[4 * (size_t)f + k] = b[k];
    __hip_atomic_store(&ticket[f], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

namespace {

constexpr int BARS_FRAMES_PER_LAUNCH = 32768;         // (a grid's second dimension holds 65535)

template <typename T>
hipError_t launch_box(const T* frames, int n, int H, int W, int limit, uint32_t* scratch, const BarsOut& out, hipStream_t s) {
    if (!frames || !scratch || !out.box || n < 1 || !bars_args_ok(H, W, limit) || reinterpret_cast<uintptr_t>(frames) % sizeof(T))
        return hipErrorInvalidValue;
    const size_t row_bytes = (size_t)W * 3 * sizeof(T);
    const uintptr_t base = reinterpret_cast<uintptr_t>(frames);
    const int words = base % 16 == 0 && row_bytes % 16 == 0 ? 4 : (base % 4 == 0 && row_bytes % 4 == 0 ? 1 : 0);
    const int groups = W / (words ? 4 * words / (int)sizeof(T) : 1);   // (a multiple: 16 | 8 pixels are 48 bytes, 4 | 2 are 12)
    int tx_log2 = 0;
    while (tx_log2 < 8 && (1 << tx_log2) < groups) ++tx_log2;
    uint32_t* const col_sums = scratch;
    uint32_t* const ticket = col_sums + (size_t)n * W;
    uint32_t* const rows = out.rows ? out.rows : ticket + n;
    for (int f0 = 0; f0 < n; f0 += BARS_FRAMES_PER_LAUNCH) {
        const int nf = n - f0 < BARS_FRAMES_PER_LAUNCH ? n - f0 : BARS_FRAMES_PER_LAUNCH;
        const dim3 grid((unsigned)((H + BARS_STRIP - 1) / BARS_STRIP), (unsigned)nf), block(BARS_THREADS);
        const T* const at = frames + (size_t)f0 * H * W * 3;
        uint32_t* const cols_out = out.cols ? out.cols + (size_t)f0 * W : nullptr;
#define PFNL_BARS_LAUNCH(W_)                                                                                                          \
    hipLaunchKernelGGL((content_box_kernel<T, W_>), grid, block, 0, s, at, H, W, limit, tx_log2, col_sums + (size_t)f0 * W, ticket + f0, \
                       rows + (size_t)f0 * H, cols_out, out.box + 4 * (size_t)f0)
        if (words == 4)
            PFNL_BARS_LAUNCH(4);
        else if (words == 1)
            PFNL_BARS_LAUNCH(1);
        else
            PFNL_BARS_LAUNCH(0);
#undef PFNL_BARS_LAUNCH
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace

size_t bars_scratch_words(int n, int H, int W) { return (size_t)n * ((size_t)W + 1 + (size_t)H); }

hipError_t launch_content_box(const uint8_t* frames, int n, int H, int W, int limit, uint32_t* scratch, const BarsOut& out, hipStream_t s) {
    return launch_box<uint8_t>(frames, n, H, W, limit, scratch, out, s);
}

hipError_t launch_content_box(const uint16_t* frames, int n, int H, int W, int limit, uint32_t* scratch, const BarsOut& out, hipStream_t s) {
    return launch_box<uint16_t>(frames, n, H, W, limit, scratch, out, s);
}

}  // namespace pfnl
