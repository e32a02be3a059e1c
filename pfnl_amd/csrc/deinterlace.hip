// INTERLACED INPUT (include/pfnl_hip.h INTERLACED; the rule: pfnl_amd/deinterlace.py; strips and index rules: field_geom.h): five decoded
// fields P2, P1, A, N1, N2 - tight [H/2][W][3] samples each - -> the progressive frame [H][W][3] at the time of field A.  Row 2 i + p is
// A[i]; row 2 j + (1 - p) is the vertical cubic of A's own rows, held within `diff` of the temporal mean of P1[j] and N1[j].
// The rule has no horizontal term, so a row is a flat run of 3 W samples: a lane owns ONE 16-byte word of the row (16 or 8 samples) and
// walks down a strip of DEINT_STRIP_PAIRS pairs of output rows.  The same-parity rows it needs again for the next pair - A[u - 1 .. u + 2],
// P2 / N2[u, u + 1] - stay in registers, P1[j] and N1[j] are read once, the kept row and the made row leave as 16-byte stores; no LDS.  The
// arithmetic runs two samples per instruction on packed 16-bit lanes: every intermediate fits an int16 at both depths.  Where the bytes of a
// row or one of the pointers are no multiple of 16 the whole launch moves 4-byte words, and single samples where not of 4 either: the
// form is read off the addresses.  The fields are read-only and may be one another (the ends of a sequence repeat a field).
#include "field_geom.h"
#include "field_words.h"

namespace pfnl {

namespace {

// the missing sample, two at a time (pfnl_amd/deinterlace.py; the clip ahead of the shift, as sample_depth.h shift_clip has it)
template <int MAXV>
__device__ __forceinline__ s16x2 made_sample(s16x2 cc, s16x2 c, s16x2 e, s16x2 ee, s16x2 x, s16x2 y, s16x2 p2a, s16x2 p2b, s16x2 n2a, s16x2 n2b) {
    s16x2 num = (c + e) * (short)9 - (cc + ee) + (short)8;
    num = vmin(vmax(num, (s16x2)(0)), (s16x2)((MAXV << 4) + 15));
    const s16x2 s = num >> 4;
    const s16x2 d = (x + y + (short)1) >> 1;
    const s16x2 t0 = (vabsdiff(x, y) + (short)1) >> 1;
    const s16x2 t1 = (vabsdiff(p2a, c) + vabsdiff(p2b, e) + (short)1) >> 1;
    const s16x2 t2 = (vabsdiff(n2a, c) + vabsdiff(n2b, e) + (short)1) >> 1;
    const s16x2 diff = vmax(t0, vmax(t1, t2));
    return vmin(vmax(s, d - diff), d + diff);
}

struct DeintJob {
    const uint8_t *p2, *p1, *cur, *n1, *n2;
    uint8_t* out;
    int parity;
};
struct DeintJobs {
    DeintJob j[2];
};

}  // namespace

// blockIdx.y: the job.  Lane t: word t % words of the row, strip t / words of the h = H / 2 pairs of output rows.
template <typename T, int WB>
__global__ __launch_bounds__(64) void deinterlace_kernel(DeintJobs jobs, int h, size_t row_bytes) {
    typedef Word<T, WB> Wd;
    constexpr int NV = Wd::NV, MAXV = Depth<T>::LEVELS - 1;
    const DeintJob job = jobs.j[blockIdx.y];
    const int p = job.parity;
    const size_t words = row_bytes / WB, strips = ((size_t)h + DEINT_STRIP_PAIRS - 1) / DEINT_STRIP_PAIRS, total = words * strips;
    const auto row = [&](const uint8_t* f, int i) { return f + (size_t)(i < 0 ? 0 : (i > h - 1 ? h - 1 : i)) * row_bytes; };
    for (size_t t = (size_t)blockIdx.x * 64 + threadIdx.x; t < total; t += (size_t)gridDim.x * 64) {
        const size_t at = t % words * WB;
        const int j0 = (int)(t / words) * DEINT_STRIP_PAIRS, j1 = j0 + DEINT_STRIP_PAIRS < h ? j0 + DEINT_STRIP_PAIRS : h;
        s16x2 cc[NV], c[NV], e[NV], ee[NV], p2a[NV], p2b[NV], n2a[NV], n2b[NV], x[NV], y[NV], o[NV];
        int u = j0 - p;
        Wd::load(row(job.cur, u - 1) + at, cc);
        Wd::load(row(job.cur, u) + at, c);
        Wd::load(row(job.cur, u + 1) + at, e);
        Wd::load(row(job.p2, u) + at, p2a);
        Wd::load(row(job.n2, u) + at, n2a);
        for (int j = j0; j < j1; ++j, ++u) {
            Wd::load(row(job.cur, u + 2) + at, ee);
            Wd::load(row(job.p2, u + 1) + at, p2b);
            Wd::load(row(job.n2, u + 1) + at, n2b);
            Wd::load(job.p1 + (size_t)j * row_bytes + at, x);
            Wd::load(job.n1 + (size_t)j * row_bytes + at, y);
#pragma unroll
            for (int k = 0; k < NV; ++k) o[k] = made_sample<MAXV>(cc[k], c[k], e[k], ee[k], x[k], y[k], p2a[k], p2b[k], n2a[k], n2b[k]);
            // the kept row is A[j]: c with the top field current (u = j), e with the bottom one (u = j - 1)
            uint8_t* const pair = job.out + (size_t)(2 * j) * row_bytes + at;
            Wd::store(pair + (size_t)p * row_bytes, p ? e : c);
            Wd::store(pair + (size_t)(1 - p) * row_bytes, o);
#pragma unroll
            for (int k = 0; k < NV; ++k) cc[k] = c[k], c[k] = e[k], e[k] = ee[k], p2a[k] = p2b[k], n2a[k] = n2b[k];
        }
    }
}

namespace {

template <typename T>
hipError_t launch_jobs(const DeinterlaceJob<T>* jobs, int n, int H, int W, hipStream_t s) {
    if (!jobs || n < 1 || n > 2 || H < 2 || (H & 1) || W < 1) return hipErrorInvalidValue;
    const size_t row_bytes = (size_t)W * 3 * sizeof(T);
    uintptr_t bits = row_bytes;
    DeintJobs a{};
    for (int i = 0; i < n; ++i) {
        const DeinterlaceJob<T>& q = jobs[i];
        if (!q.p2 || !q.p1 || !q.cur || !q.n1 || !q.n2 || !q.out || (q.parity != 0 && q.parity != 1)) return hipErrorInvalidValue;
        const void* const all[6] = {q.p2, q.p1, q.cur, q.n1, q.n2, q.out};
        for (const void* ptr : all) bits |= reinterpret_cast<uintptr_t>(ptr);
        a.j[i] = DeintJob{reinterpret_cast<const uint8_t*>(q.p2), reinterpret_cast<const uint8_t*>(q.p1), reinterpret_cast<const uint8_t*>(q.cur),
                          reinterpret_cast<const uint8_t*>(q.n1), reinterpret_cast<const uint8_t*>(q.n2), reinterpret_cast<uint8_t*>(q.out), q.parity};
    }
    if (bits % sizeof(T)) return hipErrorInvalidValue;
    const int wb = bits % 16 == 0 ? 16 : (bits % 4 == 0 ? 4 : (int)sizeof(T));
    const size_t h = (size_t)H / 2, lanes = row_bytes / wb * ((h + DEINT_STRIP_PAIRS - 1) / DEINT_STRIP_PAIRS), blocks = (lanes + 63) / 64;
    const dim3 grid((unsigned)(blocks < 32768 ? blocks : 32768), (unsigned)n), block(64);
    if (wb == 16)
        hipLaunchKernelGGL((deinterlace_kernel<T, 16>), grid, block, 0, s, a, (int)h, row_bytes);
    else if (wb == 4)
        hipLaunchKernelGGL((deinterlace_kernel<T, 4>), grid, block, 0, s, a, (int)h, row_bytes);
    else
        hipLaunchKernelGGL((deinterlace_kernel<T, (int)sizeof(T)>), grid, block, 0, s, a, (int)h, row_bytes);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_deinterlace(const DeinterlaceJob<uint8_t>* jobs, int n, int H, int W, hipStream_t s) { return launch_jobs(jobs, n, H, W, s); }
hipError_t launch_deinterlace(const DeinterlaceJob<uint16_t>* jobs, int n, int H, int W, hipStream_t s) { return launch_jobs(jobs, n, H, W, s); }

hipError_t launch_deinterlace(const uint8_t* p2, const uint8_t* p1, const uint8_t* cur, const uint8_t* n1, const uint8_t* n2, int H, int W, int parity,
                              uint8_t* out, hipStream_t s) {
    const DeinterlaceJob<uint8_t> job{p2, p1, cur, n1, n2, out, parity};
    return launch_jobs(&job, 1, H, W, s);
}

hipError_t launch_deinterlace(const uint16_t* p2, const uint16_t* p1, const uint16_t* cur, const uint16_t* n1, const uint16_t* n2, int H, int W,
                              int parity, uint16_t* out, hipStream_t s) {
    const DeinterlaceJob<uint16_t> job{p2, p1, cur, n1, n2, out, parity};
    return launch_jobs(&job, 1, H, W, s);
}

}  // namespace pfnl
