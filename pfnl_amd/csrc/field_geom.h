// THE INTEGER RULES OF INTERLACED INPUT (include/pfnl_hip.h INTERLACED; the rule in full: pfnl_amd/deinterlace.py): which field stands for an
// index past a sequence's ends, a field's surface as a surface of the pushed frame, which settings a session refuses with interlacing on,
// the strip of the kernel, and what a push may admit into the ring - the session's own bound, once per ring frame.  No HIP types and no HIP
// runtime calls: a plain C++ program can include this file and walk the rules (tests/test_deinterlace_host.py does).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pfnl_hip.h"

namespace pfnl {

// deinterlace.hip: a lane walks down this many pairs of output rows (a kept row and a made row); the next strip re-reads its boundary rows.
// 2 pairs: a 480 x 720 frame of bytes is 135 words x 120 strips = 16 200 lanes, one wave for every CU of the chip in the one-frame launch
// and two in the two-frame launch (twice that at 10 bits).
constexpr int DEINT_STRIP_PAIRS = 2;
constexpr int DEINT_STRIP_ROWS = 2 * DEINT_STRIP_PAIRS;               // ... in rows of the progressive frame

// the field that stands for index q of a sequence of n_fields (even, >= 2) fields, -2 <= q <= n_fields + 1: same parity, and it exists
inline long long field_replace(long long q, long long n_fields) { return q < 0 ? q + 2 : (q > n_fields - 1 ? q - 2 : q); }

// fields k = 2 n and 2 n + 1 are frame n's; the first in time has the parity of the field order (PFNL_FIELD_TFF 0: top)
inline long long field_frame(long long k) { return k >> 1; }
inline int field_parity(long long k, int field_order) { return (int)(k & 1) ^ field_order; }

// The field of parity p of a frame's surface as a surface of H / 2 rows: every plane pointer advanced by p rows, every pitch doubled.  (The
// rows of a chroma plane of a 4:2:0 frame are split the same way, so H is then a multiple of 4: interlace_refused.)
inline pfnl_surface field_surface(const pfnl_surface& frame, int planes, int p) {
    pfnl_surface f = frame;
    for (int k = 0; k < planes && k < 3; ++k) {
        f.plane[k] = static_cast<uint8_t*>(frame.plane[k]) + (size_t)p * frame.pitch[k];
        f.pitch[k] = 2 * frame.pitch[k];
    }
    return f;
}

// nullptr, or why a session of H rows does not take interlaced frames in this input setting
inline const char* interlace_refused(int mode, int field_order, int H, bool yuv_in, int in_chroma, int in_pack) {
    if (mode < PFNL_INTERLACE_OFF || mode > PFNL_INTERLACE_FIELD) return "interlace: mode PFNL_INTERLACE_OFF, PFNL_INTERLACE_FRAME or PFNL_INTERLACE_FIELD";
    if (field_order != PFNL_FIELD_TFF && field_order != PFNL_FIELD_BFF) return "interlace: field_order PFNL_FIELD_TFF or PFNL_FIELD_BFF";
    if (mode == PFNL_INTERLACE_OFF) return nullptr;
    if (H < 2 || (H & 1)) return "interlace: H must be even";
    if (yuv_in && in_pack == PFNL_PACK_NONE && in_chroma == PFNL_CHROMA_420 && (H & 3))
        return "interlace: the fields of a 4:2:0 frame need H to be a multiple of 4";
    return nullptr;
}

// ---- the ring's counters, and the bound of a push applied once per ring frame ----
struct RingCounters {
    long long pushed, launched, delivered;   // ring frames
    int in_flight;                           // batches launched and not yet fully delivered: 0 .. 2
    long long oldest;                        // the first frame of the oldest of them (in_flight > 0)
};

// the session's batch rule while the sequence has not ended (pfnl_stream_next_batch)
inline int ring_next_batch(int T, int batch, long long pushed, long long launched) { return pushed >= launched + batch + T / 2 ? batch : 0; }

// One more frame into a ring of `cap` slots: false where the push is refused ("pop first"; *c unchanged), else the counters behind the push
// and the batches it launches.
inline bool ring_admit(int T, int batch, int cap, RingCounters* c) {
    const int count = ring_next_batch(T, batch, c->pushed + 1, c->launched);
    const long long oldest = c->in_flight ? c->oldest : c->launched;
    const long long lo = oldest - T / 2 < 0 ? 0 : oldest - T / 2;
    if ((count && c->launched - c->delivered + count > 2LL * batch) || c->pushed - lo + 1 > cap) return false;
    ++c->pushed;
    while (c->in_flight < 2) {
        const int n = ring_next_batch(T, batch, c->pushed, c->launched);
        if (!n) break;
        if (!c->in_flight) c->oldest = c->launched;
        c->launched += n;
        ++c->in_flight;
    }
    return true;
}

// all of `frames` ring frames or none: the counters are advanced only where every one is admitted
inline bool ring_admit_all(int T, int batch, int cap, int frames, RingCounters* c) {
    RingCounters t = *c;
    for (int i = 0; i < frames; ++i)
        if (!ring_admit(T, batch, cap, &t)) return false;
    *c = t;
    return true;
}

// the ring frames one woven frame becomes
inline int interlace_yield(int mode) { return mode == PFNL_INTERLACE_FIELD ? 2 : (mode == PFNL_INTERLACE_FRAME ? 1 : 0); }

}  // namespace pfnl
