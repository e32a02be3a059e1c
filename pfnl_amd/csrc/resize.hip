// The tap tables of the resampler at stage 1 of the streaming session's output edge (include/pfnl_hip.h, pfnl_stream_resize /
// pfnl_stream_place), behind the quantisation and ahead of the YUV conversion.  The rule is stated once on the host in integers,
// pfnl_amd/resize.py: a separable Keys cubic (a = -1/2) whose support widens by in / out when the raster shrinks, coefficients with 14
// fractional bits that sum to 2^14 per row, horizontal pass first into an unclipped intermediate, one rounding and one clip at the end.
// resize_axis builds that module's tables with 128-bit integers (no floating point, no device); resize_plan lays both axes out as the one
// block of device memory the kernel of place.hip reads - it reads tables and never evaluates the filter.  sum |c| <= 2^15 per row (checked
// when the table is built) keeps the intermediate inside int16 and the second pass's sum inside int32, at both sample depths.
#include <string>

#include "common.h"

namespace pfnl {

namespace {

typedef __int128 i128;

i128 floor_div(i128 a, i128 b) {                                       // b > 0
    const i128 q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

i128 keys_weight(long long u, long long d) {                           // the Keys kernel at u / d, times 2 d^3
    const i128 U = u, D = d;
    if (u <= d) return 3 * U * U * U - 5 * U * U * D + 2 * D * D * D;
    if (u < 2 * d) return -U * U * U + 5 * U * U * D - 8 * U * D * D + 4 * D * D * D;
    return 0;
}

}  // namespace

bool resize_axis(int n_in, int n_out, ResizeAxis* t, std::string* why) {
    if (n_in < 1 || n_out < 1 || n_in > RESIZE_MAX_SIZE || n_out > RESIZE_MAX_SIZE) {
        *why = "resize: sizes must lie in 1 .. " + std::to_string(RESIZE_MAX_SIZE);
        return false;
    }
    if (n_out < (n_in + 3) / 4 || n_out > 2 * n_in) {
        *why = "resize: " + std::to_string(n_in) + " -> " + std::to_string(n_out) + ": the output must lie between a quarter and twice the input";
        return false;
    }
    const long long d = 2LL * (n_in > n_out ? n_in : n_out);
    std::vector<std::vector<int>> rows((size_t)n_out);
    t->first.assign((size_t)n_out, 0);
    t->count.assign((size_t)n_out, 0);
    t->ntaps = 0;
    std::vector<i128> w;
    for (int o = 0; o < n_out; ++o) {
        const long long centre = (long long)n_in * (2 * o + 1);
        long long j = (long long)floor_div(centre - 2 * d - n_out, 2LL * n_out);   // the last index left of the support
        long long first = -1;
        w.clear();
        for (;;) {
            ++j;
            const long long n = (long long)n_out * (2 * j + 1) - centre;
            if (n >= 2 * d) break;
            if (n <= -2 * d) continue;
            const long long at = j < 0 ? 0 : (j > n_in - 1 ? n_in - 1 : j);
            if (first < 0) first = at;
            if ((size_t)(at - first) == w.size()) w.push_back(0);
            w[(size_t)(at - first)] += keys_weight(n < 0 ? -n : n, d);
        }
        i128 S = 0;
        for (const i128 x : w) S += x;
        if (first < 0 || S <= 0) {
            *why = "resize: empty filter row";
            return false;
        }
        std::vector<int>& c = rows[(size_t)o];
        c.resize(w.size());
        long long sum = 0, mag = 0;
        size_t big = 0;
        for (size_t k = 0; k < w.size(); ++k) {
            c[k] = (int)floor_div(2 * w[k] * (1 << 14) + S, 2 * S);
            sum += c[k];
            if (c[k] > c[big]) big = k;
        }
        c[big] += (int)((1 << 14) - sum);
        for (const int x : c) mag += x < 0 ? -x : x;
        if (mag > (1 << 15)) {
            *why = "resize: " + std::to_string(n_in) + " -> " + std::to_string(n_out) + ": a row's sum of magnitudes exceeds 2^15";
            return false;
        }
        t->first[(size_t)o] = (int32_t)first;
        t->count[(size_t)o] = (int32_t)c.size();
        if ((int)c.size() > t->ntaps) t->ntaps = (int)c.size();
        // the kernel sizes its tile by these: neither end of the run ever moves back
        if (o && (t->first[(size_t)o] < t->first[(size_t)o - 1] ||
                  t->first[(size_t)o] + t->count[(size_t)o] < t->first[(size_t)o - 1] + t->count[(size_t)o - 1])) {
            *why = "resize: tap runs out of order";
            return false;
        }
        if (first + (long long)c.size() > n_in) {
            *why = "resize: tap run outside the input";
            return false;
        }
    }
    t->coef.assign((size_t)n_out * t->ntaps, 0);
    for (int o = 0; o < n_out; ++o)
        for (size_t k = 0; k < rows[(size_t)o].size(); ++k) t->coef[(size_t)o * t->ntaps + k] = (int16_t)rows[(size_t)o][k];
    return true;
}

bool resize_plan(int H, int W, int oH, int oW, ResizePlan* p, std::string* why) {
    ResizeAxis h, v;
    if (!resize_axis(W, oW, &h, why) || !resize_axis(H, oH, &v, why)) return false;
    p->H = H, p->W = W, p->oH = oH, p->oW = oW, p->ht = h.ntaps, p->vt = v.ntaps;
    p->max_rows = 0;
    for (int y0 = 0; y0 < oH; y0 += RESIZE_TH) {
        const int y1 = (y0 + RESIZE_TH < oH ? y0 + RESIZE_TH : oH) - 1;
        const int rows = v.first[(size_t)y1] + v.count[(size_t)y1] - v.first[(size_t)y0];
        if (rows > p->max_rows) p->max_rows = rows;
    }
    if ((size_t)p->max_rows * RESIZE_TW * 3 * sizeof(int16_t) > 65536) {   // (a 4 : 1 reduction names 76 rows: 29 184 bytes)
        *why = "resize: the tile's intermediate does not fit the LDS";
        return false;
    }
    // hfirst [oW] | hcount [oW] | vfirst [oH] | vcount [oH] | hcoef int16 [oW][ht] | vcoef int16 [oH][vt], each part on a 4-byte boundary
    const size_t hc = ((size_t)oW * h.ntaps + 1) / 2, vc = ((size_t)oH * v.ntaps + 1) / 2;
    p->blob.assign(2 * (size_t)oW + 2 * (size_t)oH + hc + vc, 0);
    int32_t* b = p->blob.data();
    std::copy(h.first.begin(), h.first.end(), b);
    std::copy(h.count.begin(), h.count.end(), b + oW);
    std::copy(v.first.begin(), v.first.end(), b + 2 * (size_t)oW);
    std::copy(v.count.begin(), v.count.end(), b + 2 * (size_t)oW + oH);
    int16_t* c = reinterpret_cast<int16_t*>(b + 2 * (size_t)oW + 2 * (size_t)oH);
    std::copy(h.coef.begin(), h.coef.end(), c);
    std::copy(v.coef.begin(), v.coef.end(), c + 2 * hc);
    return true;
}

}  // namespace pfnl
