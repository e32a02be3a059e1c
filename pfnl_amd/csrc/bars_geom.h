// THE INTEGER RULES OF THE CONTENT BOX (include/pfnl_hip.h BARS; the rule in full: pfnl_amd/bars.py): the threshold a line's sum of luma
// is compared with, the scan for the first and the last picture line, the box of two scans, the union of boxes, the snap onto a grid and
// the decision of a probe.  The last workgroup of the kernel (bars.hip) and the session (capi_stream.hip) call the same functions.  No HIP
// types and no HIP runtime calls: a plain C++ program can include this file and walk the rules (tests/test_bars_host.py does).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PFNL_BARS_FN __host__ __device__ inline
#else
#define PFNL_BARS_FN inline
#endif

namespace pfnl {

constexpr int BARS_LIMIT_MAX = 219;                                   // the luma of white at 8 bits
constexpr int BARS_MAX_SIDE = 16384;                                  // 220 * 16384 < 2^32: the sums are 32-bit

PFNL_BARS_FN bool bars_args_ok(int H, int W, int limit) {
    return H >= 1 && H <= BARS_MAX_SIDE && W >= 1 && W <= BARS_MAX_SIDE && limit >= 0 && limit <= BARS_LIMIT_MAX;
}

// a line of `across` pixels is picture iff its sum exceeds this (at most 219 * 16384: it fits 32 bits, as every sum does)
PFNL_BARS_FN uint32_t bars_threshold(int limit, int across) { return (uint32_t)limit * (uint32_t)across; }

// One line of a scan: line i, whose sum is v, widens the span first .. last where it is picture.  A span starts as first = n, last = -1
// (no picture line); the lines may come in any order, and spans over disjoint sets of lines merge by min and max - the kernel's last
// workgroup deals the lines out to its threads, which hold several sums at a time.
PFNL_BARS_FN void bars_scan_line(int i, uint32_t v, uint32_t thr, int* first, int* last) {
    if (v > thr) {
        *first = *first < i ? *first : i;
        *last = *last > i ? *last : i;
    }
}

// the span of the lines start, start + stride, .. < n, each sum read once: the host scans with (0, 1)
template <class Sum>
PFNL_BARS_FN void bars_scan(Sum&& sum, int n, uint32_t thr, int start, int stride, int* first, int* last) {
    *first = n;
    *last = -1;
    for (int i = start; i < n; i += stride) bars_scan_line(i, (uint32_t)sum(i), thr, first, last);
}

// (y0, x0, h, w) of the two spans; no picture row or no picture column: the empty box (0, 0, 0, 0)
PFNL_BARS_FN void bars_box(int row_first, int row_last, int col_first, int col_last, int32_t box[4]) {
    const bool none = row_last < row_first || col_last < col_first;
    box[0] = none ? 0 : row_first;
    box[1] = none ? 0 : col_first;
    box[2] = none ? 0 : row_last - row_first + 1;
    box[3] = none ? 0 : col_last - col_first + 1;
}

PFNL_BARS_FN bool bars_empty(const int32_t b[4]) { return b[2] <= 0 || b[3] <= 0; }

// acc = the bounding box of acc and b; an empty box adds nothing
PFNL_BARS_FN void bars_union(int32_t acc[4], const int32_t b[4]) {
    if (bars_empty(b)) return;
    if (bars_empty(acc)) {
        for (int k = 0; k < 4; ++k) acc[k] = b[k];
        return;
    }
    const int32_t y1 = acc[0] + acc[2] > b[0] + b[2] ? acc[0] + acc[2] : b[0] + b[2];
    const int32_t x1 = acc[1] + acc[3] > b[1] + b[3] ? acc[1] + acc[3] : b[1] + b[3];
    acc[0] = acc[0] < b[0] ? acc[0] : b[0];
    acc[1] = acc[1] < b[1] ? acc[1] : b[1];
    acc[2] = y1 - acc[0];
    acc[3] = x1 - acc[1];
}

// the box shrunk inward onto multiples of ay rows and ax columns (ay, ax >= 1): the start rounded up, the end down; what vanishes is empty
PFNL_BARS_FN void bars_snap(int32_t b[4], int ay, int ax) {
    if (!bars_empty(b)) {
        const int32_t y0 = (b[0] + ay - 1) / ay * ay, x0 = (b[1] + ax - 1) / ax * ax;
        const int32_t y1 = (b[0] + b[2]) / ay * ay, x1 = (b[1] + b[3]) / ax * ax;
        if (y1 > y0 && x1 > x0) {
            b[0] = y0, b[1] = x0, b[2] = y1 - y0, b[3] = x1 - x0;
            return;
        }
    }
    b[0] = b[1] = b[2] = b[3] = 0;
}

// the grid of a crop ahead of the network: even H and W; woven 4:2:0 planes keep field parity and whole chroma rows
PFNL_BARS_FN void bars_align(bool planes_420, bool woven, int* ay, int* ax) {
    *ay = planes_420 && woven ? 4 : 2;
    *ax = 2;
}

// the crop of a probe whose union is `u`: its snap, or the whole frame where that is empty, leaves the frame or keeps less than keep_p / keep_q
// of either axis
PFNL_BARS_FN void bars_decide(const int32_t u[4], int H, int W, int ay, int ax, int keep_p, int keep_q, int32_t out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = u[k];
    bars_snap(out, ay, ax);
    const bool whole = bars_empty(out) || out[0] + out[2] > H || out[1] + out[3] > W || (long long)out[2] * keep_q < (long long)H * keep_p ||
                       (long long)out[3] * keep_q < (long long)W * keep_p;
    if (whole) out[0] = 0, out[1] = 0, out[2] = H, out[3] = W;
}

}  // namespace pfnl
