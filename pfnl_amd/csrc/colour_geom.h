// THE INTEGERS OF THE COLOUR CONVERSION (include/pfnl_hip.h COLOUR; the rule in full: pfnl_amd/colour.py): the gamut matrix between two
// sets of primaries with 14 fractional bits, the transfer tables D (sample -> 16-bit linear light) and E (linear light -> sample), and E
// in the form the kernel holds in LDS - the code at the start of each 64-wide bucket of l and the thresholds, read by encode_lookup.  No
// HIP types and no HIP runtime calls: a plain C++ program can include this file and walk every entry (tests/test_colour_host.py does).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PFNL_COLOUR_FN __host__ __device__ inline
#else
#define PFNL_COLOUR_FN inline
#endif

namespace pfnl {

constexpr int COLOUR_PRIMARIES = 3;                                   // PFNL_PRIM_BT709 | _BT601_525 | _BT601_625
constexpr int COLOUR_FRAC = 14;                                       // fractional bits of the matrix
constexpr int COLOUR_LINEAR = 65536;                                  // linear light is 16 bits
constexpr int COLOUR_BUCKET = 6, COLOUR_BUCKETS = COLOUR_LINEAR >> COLOUR_BUCKET;
constexpr int COLOUR_STEPS_8 = 2, COLOUR_STEPS_10 = 5;                // code boundaries inside one bucket, at most (the OETF's slope is at most 4.5)

inline bool is_primaries(int v) { return v >= 0 && v < COLOUR_PRIMARIES; }

struct ColourMatrix {
    int32_t m[9];                                                     // row-major: out channel r = sum over c of m[3 r + c] in[c]
};

namespace colour_detail {

// CIE 1931 x, y of R, G, B in thousandths: BT.709 | SMPTE 170M | BT.470BG; white D65 = (0.3127, 0.3290) for all three, in ten-thousandths
constexpr int XY[COLOUR_PRIMARIES][3][2] = {{{640, 330}, {300, 600}, {150, 60}}, {{630, 340}, {310, 595}, {155, 70}}, {{640, 330}, {290, 600}, {150, 60}}};
constexpr long long WHITE[3] = {3127, 3290, 10000 - 3127 - 3290};

typedef __int128 wide;
struct M3 {
    wide v[3][3];
};
// the columns (x, y, 1 - x - y) of the three primaries, in thousandths.  RGB -> XYZ is P diag(s) / det P with s = adj(P) white: the
// factor 1 / y of each column is part of s, and white's own scale is common to both sides of a conversion.
inline M3 chromaticities(int id) {
    M3 p;
    for (int c = 0; c < 3; ++c) p.v[0][c] = XY[id][c][0], p.v[1][c] = XY[id][c][1], p.v[2][c] = 1000 - XY[id][c][0] - XY[id][c][1];
    return p;
}
inline M3 adjugate(const M3& m) {
    const wide a = m.v[0][0], b = m.v[0][1], c = m.v[0][2], d = m.v[1][0], e = m.v[1][1], f = m.v[1][2], g = m.v[2][0], h = m.v[2][1], i = m.v[2][2];
    return M3{{{e * i - f * h, c * h - b * i, b * f - c * e}, {f * g - d * i, a * i - c * g, c * d - a * f}, {d * h - e * g, b * g - a * h, a * e - b * d}}};
}
inline wide determinant(const M3& m) {
    return m.v[0][0] * (m.v[1][1] * m.v[2][2] - m.v[1][2] * m.v[2][1]) - m.v[0][1] * (m.v[1][0] * m.v[2][2] - m.v[1][2] * m.v[2][0]) +
           m.v[0][2] * (m.v[1][0] * m.v[2][1] - m.v[1][1] * m.v[2][0]);
}
inline void white_scale(const M3& adj, wide s[3]) {
    for (int r = 0; r < 3; ++r) s[r] = adj.v[r][0] * WHITE[0] + adj.v[r][1] * WHITE[1] + adj.v[r][2] * WHITE[2];
}

constexpr double ALPHA = 1.09929682680944, BETA = 0.018053968510807;  // the BT.709 OETF
inline double oetf(double L) { return L < BETA ? 4.5 * L : ALPHA * std::pow(L, 0.45) - (ALPHA - 1.0); }
inline double oetf_inverse(double V) { return V < 4.5 * BETA ? V / 4.5 : std::pow((V + (ALPHA - 1.0)) / ALPHA, 1.0 / 0.45); }

}  // namespace colour_detail

// colour.py gamut_matrix: src -> XYZ -> dst in exact arithmetic, each entry times 2^14 rounded half away from zero, the diagonal entry
// then the residual of its row, so every row sums to 2^14 and src == dst is 2^14 I.  With P, s as above the entry is the rational
// (adj(P_dst) P_src)[r][c] s_src[c] / (s_dst[r] det P_src): integers below 2^80, so 128 bits hold them with the 2^15 of the rounding.
// false: an id outside the enum.
inline bool colour_matrix(int src, int dst, ColourMatrix* out) {
    using namespace colour_detail;
    if (!is_primaries(src) || !is_primaries(dst) || !out) return false;
    const M3 ps = chromaticities(src), ad = adjugate(chromaticities(dst));
    wide ss[3], sd[3];
    white_scale(adjugate(ps), ss);
    white_scale(ad, sd);
    const wide det = determinant(ps);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            wide n = (ad.v[r][0] * ps.v[0][c] + ad.v[r][1] * ps.v[1][c] + ad.v[r][2] * ps.v[2][c]) * ss[c] * (1 << COLOUR_FRAC), d = sd[r] * det;
            if (d < 0) n = -n, d = -d;
            const wide a = n < 0 ? -n : n, q = (2 * a + d) / (2 * d);
            out->m[3 * r + c] = (int32_t)(n < 0 ? -q : q);
        }
        out->m[4 * r] = (1 << COLOUR_FRAC) - out->m[3 * r + (r + 1) % 3] - out->m[3 * r + (r + 2) % 3];
    }
    return true;
}

// colour.py tables: D[v] = floor(65535 f^-1(v / top) + 0.5), v = 0 .. top; E[l] = floor(top f(l / 65535) + 0.5), l = 0 .. 65535; double
// arithmetic and the C library's pow, as math.pow is.  false: bits other than 8 or 10.  Either pointer may be null.
inline bool colour_tables(int bits, uint16_t* decode, uint16_t* encode) {
    if (bits != 8 && bits != 10) return false;
    const int top = (1 << bits) - 1;
    for (int v = 0; v <= top && decode; ++v) decode[v] = (uint16_t)std::floor(65535.0 * colour_detail::oetf_inverse((double)v / top) + 0.5);
    for (int l = 0; l < COLOUR_LINEAR && encode; ++l) encode[l] = (uint16_t)std::floor(top * colour_detail::oetf((double)l / 65535.0) + 0.5);
    return true;
}

// What the kernel holds, [D: levels][start: 1024][threshold: levels] uint16 (levels = 2^bits): start[k] = E[64 k]; threshold[c] = the
// smallest l with E[l] >= c (E is monotone and takes every code; threshold[0] = 0).  colour.py encode_form.
inline int colour_blob_words(int bits) { return 2 * (1 << bits) + COLOUR_BUCKETS; }
inline bool colour_blob(int bits, std::vector<uint16_t>* blob) {
    if ((bits != 8 && bits != 10) || !blob) return false;
    const int levels = 1 << bits;
    std::vector<uint16_t> E(COLOUR_LINEAR);
    blob->assign(colour_blob_words(bits), 0);
    colour_tables(bits, blob->data(), E.data());
    uint16_t* const start = blob->data() + levels;
    uint16_t* const threshold = start + COLOUR_BUCKETS;
    for (int k = 0; k < COLOUR_BUCKETS; ++k) start[k] = E[k << COLOUR_BUCKET];
    for (int l = COLOUR_LINEAR - 1; l >= 0; --l) threshold[E[l]] = (uint16_t)l;   // (descending: the smallest l of a code stays)
    threshold[0] = 0;
    return true;
}

// E[l] from that form: the bucket's code, then at most STEPS compares against the next code's threshold.  P: a pointer to uint16 (LDS in
// the kernel).  The host test walks all 65536 values of l at both depths against E.
template <int LEVELS, typename P>
PFNL_COLOUR_FN int encode_lookup(P start, P threshold, int l) {
    constexpr int STEPS = LEVELS == 256 ? COLOUR_STEPS_8 : COLOUR_STEPS_10;
    int c = start[l >> COLOUR_BUCKET];
    for (int k = 0; k < STEPS; ++k) {
        const int next = c < LEVELS - 1 ? c + 1 : c;                  // (no code above the top: the index stays inside the table)
        c = (c < LEVELS - 1 && l >= (int)threshold[next]) ? next : c;
    }
    return c;
}

}  // namespace pfnl
