// THE INTEGER RULES OF INVERSE TELECINE (include/pfnl_hip.h TELECINE; the rule in full: pfnl_amd/telecine.py): which fields a match reads, the
// cycle a frame belongs to, how many ring frames a push or the end completes in each mode, which frame of a cycle is dropped, where a cut
// mark lands for a given drop index, and whether the ring's bound - field_geom.h's, applied to everything a push completes - can ever
// admit a cycle.  No HIP types and no HIP runtime calls: a plain C++ program can include this file and walk the rules
// (tests/test_telecine_host.py does).
#pragma once
#include "field_geom.h"

namespace pfnl {

constexpr int TC_CYCLE = 5;                                           // pushed frames per decimation cycle: one of them is dropped
constexpr unsigned long long TC_D_FIRST = ~0ull;                      // D_0: the first frame of a sequence is never the repeat

// the fields the match of pushed frame n reads, of a sequence of n_fields fields so far: the kept field A = 2 n, the candidates c = 2 n + 1
// (the frame as pushed) and p = 2 n - 1, replaced at n = 0 (it becomes field 1: c = p there)
struct MatchFields {
    long long a, c, p;
};
inline MatchFields telecine_match_fields(long long n, long long n_fields) { return MatchFields{2 * n, 2 * n + 1, field_replace(2 * n - 1, n_fields)}; }

inline long long telecine_cycle(long long n) { return n / TC_CYCLE; }
inline int telecine_cycle_slot(long long n) { return (int)(n % TC_CYCLE); }

// the ring frames that become admissible when matched frame n has been made, the sequence not ended: every one in mode MATCH; in mode
// DECIMATE the four kept frames of a cycle with its last frame
inline int telecine_yield(int mode, long long n) {
    if (mode == PFNL_TELECINE_MATCH) return 1;
    return mode == PFNL_TELECINE_DECIMATE && telecine_cycle_slot(n) == TC_CYCLE - 1 ? TC_CYCLE - 1 : 0;
}
// ... by the push that finds `pushed` frames pushed before it: it makes matched frame pushed - 1 (the first push makes none)
inline int telecine_push_yield(int mode, long long pushed) { return pushed > 0 ? telecine_yield(mode, pushed - 1) : 0; }
// ... by pfnl_stream_end after `pushed` frames of which `matched` have been made: the held frame, and in mode DECIMATE the frames of the
// cycle it leaves incomplete, whole
inline int telecine_end_yield(int mode, long long pushed, long long matched) {
    if (mode == PFNL_TELECINE_MATCH) return (int)(pushed - matched);
    if (mode != PFNL_TELECINE_DECIMATE || pushed == 0) return 0;
    const int rest = telecine_cycle_slot(pushed);
    return rest ? rest : (pushed > matched ? TC_CYCLE - 1 : 0);
}

// the ring frames a session has made of `pushed` pushed frames (pfnl_telecine_deliverable)
inline long long telecine_deliverable(int mode, long long pushed, int ended) {
    const long long matched = ended ? pushed : (pushed > 0 ? pushed - 1 : 0);
    if (mode == PFNL_TELECINE_MATCH) return matched;
    if (mode != PFNL_TELECINE_DECIMATE) return 0;
    return (TC_CYCLE - 1) * (matched / TC_CYCLE) + (ended ? matched % TC_CYCLE : 0);
}

// the frame of a complete cycle that is dropped: the smallest D, the lowest index on a tie
inline int telecine_drop_index(const unsigned long long d[TC_CYCLE]) {
    int at = 0;
    for (int j = 1; j < TC_CYCLE; ++j)
        if (d[j] < d[at]) at = j;
    return at;
}

// The marks of the delivered frames of one cycle of n pushed frames (drop < 0: an incomplete cycle, nothing dropped): a mark lands on the
// first delivered frame made from its own frame or a later one.  *carry: the mark the cycle before left, and on return the one this
// cycle leaves.  Returns how many frames are delivered.
inline int telecine_place_marks(const bool* marks, int n, int drop, bool* carry, bool* out) {
    int made = 0;
    for (int j = 0; j < n; ++j) {
        *carry = *carry || marks[j];
        if (j == drop) continue;
        out[made++] = *carry;
        *carry = false;
    }
    return made;
}

// Can the session's ring ever take the four frames the end of a cycle completes?  The ring holds at most 2 batch undelivered SR frames and
// cap = 3 batch + T - 2 slots (pfnl_stream_open).  With everything popped, launched = delivered = L, pushed <= L + batch + T / 2 - 1 and the
// oldest frame a window may name is L - T / 2: four more frames launch at most ceil(4 / batch) batches and reach slot distance
// batch + T + 2, so both clauses of ring_admit hold iff 2 batch >= 4.  A batch of 1 launches a batch per frame and is refused at the third
// whatever has been popped.  (tests/test_telecine_host.py walks ring_admit_all from an empty ring, popping where refused, against this.)
inline bool telecine_ring_fits(int batch) { return 2 * batch >= TC_CYCLE - 1; }

// nullptr, or why a session does not take telecined frames in this setting: the deinterlacer's rules on H, and a ring that holds a cycle
inline const char* telecine_refused(int mode, int field_order, int H, bool yuv_in, int in_chroma, int in_pack, int batch) {
    if (mode < PFNL_TELECINE_OFF || mode > PFNL_TELECINE_DECIMATE) return "telecine: mode PFNL_TELECINE_OFF, PFNL_TELECINE_MATCH or PFNL_TELECINE_DECIMATE";
    if (field_order != PFNL_FIELD_TFF && field_order != PFNL_FIELD_BFF) return "telecine: field_order PFNL_FIELD_TFF or PFNL_FIELD_BFF";
    if (mode == PFNL_TELECINE_OFF) return nullptr;
    if (H < 2 || (H & 1)) return "telecine: H must be even";
    if (yuv_in && in_pack == PFNL_PACK_NONE && in_chroma == PFNL_CHROMA_420 && (H & 3))
        return "telecine: the fields of a 4:2:0 frame need H to be a multiple of 4";
    if (mode == PFNL_TELECINE_DECIMATE && !telecine_ring_fits(batch))
        return "telecine: the ring of this batch never holds the four frames a cycle completes (a larger batch does)";
    return nullptr;
}

// nullptr, or why the parameters are refused; *out: the parameters with the defaults of an h x W field filled in (p NULL: all defaults)
inline const char* telecine_params_refused(const pfnl_telecine_params* p, int h, int W, pfnl_telecine_params* out) {
    const pfnl_telecine_params dflt{10, 1, (long long)(((unsigned long long)h * 3ull * (unsigned long long)W) >> 8)};
    *out = p ? *p : dflt;
    if (out->comb_limit < 0) out->comb_limit = dflt.comb_limit;       // (negative: the default)
    if (out->threshold < 1 || out->threshold > 255) return "telecine: threshold in 1 .. 255";
    if (out->post != 0 && out->post != 1) return "telecine: post is 0 or 1";
    return nullptr;
}

}  // namespace pfnl
