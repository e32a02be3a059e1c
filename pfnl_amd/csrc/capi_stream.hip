// The streaming session of the C-ABI (include/pfnl_hip.h, pfnl_stream_*): uint8 LR frames are pushed one at a time, uint8 SR frames are
// popped in order (uint16 samples at 10 bits on either side: pfnl_stream_input_depth, the 10-bit out_fmts).
// What the harness's loop does around the forward (reference model/pfnl.py:236-262; pfnl_amd/model.py
// _run_sequence_on_device) - clamped windows, batching, quantisation, the range flag and the recomputation on the strict kernels - lives
// here, behind pfnl_forward's own interface: the session calls pfnl_forward / pfnl_get_option / pfnl_set_option / pfnl_range_flag like
// any other caller and knows nothing of the handle's layout (capi_internal.h, pfnl_handle_view).
// The output side is one route (stream_route.h: quantise - with the change of primaries in it where the two edges' differ, colour.hip -
// -> resize / place -> YUV, at 1 or 2 bytes per sample) and one slot per stage: the
// setters validate through that header and hand their candidate to apply_setting, the only place that allocates or frees a slot
// after open; enqueue and pop_frame read the stored route.
// The input side is one route as well (stream_route.h InRoute: the pushed surface, its tight frame, the staging frame, the decode kind),
// stored by apply_setting next to the output route: every push - a tight frame is the surface with the tight pitches - is stage_host
// (host pointers: the planes into the staging frame) and decode_surface (the one dispatch on decode kind and depth), on the whole frame
// or, with interlacing on, on each of its fields.  A setter copies the stored Setting, changes its own fields and asks candidate_refused.
#include <cmath>
#include <deque>
#include <string>

#include "../../include/pfnl_hip.h"
#include "bars_geom.h"
#include "capi_internal.h"
#include "colour_geom.h"
#include "common.h"
#include "field_geom.h"
#include "stream_route.h"
#include "telecine_geom.h"
#include "tile_geom.h"

namespace {

int fail(int code, const std::string& msg) { return pfnl_internal_fail(code, msg); }

struct Batch {
    long long first, last;   // its first frame; the newest frame its windows may name (the clamp)
    int count, slot;
    bool was_strict;         // launched after the session went strict: the range fence was not armed, nothing to check
    bool checked;            // its event has been waited for and its range flag read (and the batch recomputed if need be)
};

struct StageSlot {
    uint8_t* buf[2] = {nullptr, nullptr};             // [batch][the stage's frame] each: the undelivered frames of at most two batches
    size_t cap = 0;                                   // bytes of each
};

// The colour of one edge (pfnl_stream_colour; pfnl_stream_format sets matrix and range of both): the YUV coefficients of its matrix and
// range at both depths - an RGB edge reads neither - and its primaries.
struct SideColour {
    pfnl::YuvCoef coef{};                             // 8 bits: an 8-bit input, NV12 / I420 out
    pfnl::YuvCoef coef10{};                           // 10 bits: an input depth of 10, P010 / I010 out
    int prim = PFNL_PRIM_BT709;
};

// What the setters set and both routes follow (pfnl_stream_format, _colour, _input_depth, _chroma_format, _packing): in_fmt / out_fmt name the
// layout, the depth the pushed sample, the chroma formats the subsampling of a YUV edge, a packing an edge as one plane of interleaved samples.
struct Setting {
    int in_fmt = PFNL_PIX_RGB24, out_fmt = PFNL_PIX_RGB24;
    int in_depth = 8;                                 // 8, or 10: pushed samples, ring and staging frame are uint16
    int in_chroma = PFNL_CHROMA_420, out_chroma = PFNL_CHROMA_420;
    int in_pack = PFNL_PACK_NONE, out_pack = PFNL_PACK_NONE;
    SideColour cin, cout;                             // the decode reads the input's coefficients, stage 2 the output's
    pfnl::ColourMatrix gamut{};                       // cin.prim -> cout.prim: stage 0 converts exactly when the two differ
};

}  // namespace

struct pfnl_stream {
    pfnl_handle* h = nullptr;
    int H = 0, W = 0, batch = 0, T = 0, scale = 0, device = 0, cap = 0;
    size_t lr_bytes = 0, sr_bytes = 0;                // one LR / SR frame, uint8
    hipStream_t s = nullptr;                          // everything the session computes runs here
    hipStream_t cs = nullptr;                         // host-pointer frames in and out: copies that never wait for a later batch
    uint8_t* ring = nullptr;                          // [cap][H][W][3] samples of the input depth, frame f in slot f % cap
    float* win = nullptr;                             // [batch][T][H][W][3]
    float* sr = nullptr;                              // [batch][sH][sW][3]
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool slot_busy[2] = {false, false};
    long long pushed = 0, launched = 0, delivered = 0;
    bool ended = false;
    std::deque<Batch> q;                              // launched, not yet fully delivered: at most two
    bool strict = false;                              // a batch was flagged: the rest of the sequence runs on the strict kernels
    std::string prior_strict, prior_precision;        // what the library held before go_strict changed it ("" = unchanged)
    int ensemble = 1;                                 // pfnl_stream_ensemble: the members of every batch's forward (1: the plain forward)
    bool tiled = false;                               // pfnl_stream_tile: every batch's forward runs as tiles of `tiling`
    pfnl_tiling tiling{};
    // scenes (pfnl_stream_scenes): allocated by the first call that turns them on; they have the ring's lifetime and its slots
    int scene_mode = 0;                               // 0 off | 1 marks | 2 marks + detector
    unsigned long long thr_sum = 0;                   // ceil(threshold H W): the detector compares sums
    bool mark = false;                                // pfnl_stream_mark_cut: the next pushed frame starts a scene
    long long* scene_first = nullptr;                 // [cap] the first frame of the scene of the frame in the slot | sad [cap] | scratch [2]
    unsigned long long* sad = nullptr;                // (= scene_first + cap)
    long long* info[2] = {nullptr, nullptr};          // pinned host copies of scene_first | sad, one per output slot: they travel with the batch
    hipEvent_t scene_ev = nullptr;                    // the newest decision on the session's stream (device-pointer pushes)
    bool decided_on_s = false;                        // ... that a decision on the copy stream has not yet been ordered behind
    bool has_info = false;                            // what pfnl_stream_pop_info returns
    long long info_first = 0;
    unsigned long long info_sad = 0;
    // the setting (pfnl_stream_format, pfnl_stream_input_depth, pfnl_stream_chroma_format, pfnl_stream_packing, pfnl_stream_resize,
    // pfnl_stream_place; stored by apply_setting alone, with the two routes it yields).  The ring stays RGB: a YUV frame is converted
    // on its way into its ring slot.  Every stage `route` runs has a slot with room for a batch - 8- and 10-bit samples share it, as a
    // sequence has one route - and no other stage holds memory; stage 0 is allocated at open.
    Setting set;
    int in_siting = PFNL_SITING_LEFT, out_siting = PFNL_SITING_LEFT;   // pfnl_stream_chroma_siting: where a 4:2:0 edge's chroma sits
    uint8_t* yin = nullptr;                           // [in.staging_bytes] the staging frame: a host-pointer frame on its way to the kernel; from the first YUV in_fmt or input packing on
    size_t yin_cap = 0;                               // its bytes
    pfnl::PlacePlan rplan;                            // stage 1: a rectangle of the raster on a canvas, the whole onto the whole for a plain size; cH = 0: off
    int32_t* rtab = nullptr;                          // rplan.r.blob on the device
    const uint16_t* ctab[2] = {nullptr, nullptr};     // the device's colour tables at 8 | 10 bits (colour_device_tables: not the session's to free)
    pfnl::OutRoute route{};
    pfnl::InRoute in{};                               // the pushed frame of `set` at H x W: in.ring_bytes is one LR frame as the ring holds it
    StageSlot slot[pfnl::ROUTE_STAGES];
    // interlaced input (pfnl_stream_interlace; field_geom.h): the decoded fields of the three newest woven frames, ahead of the ring
    int il_mode = PFNL_INTERLACE_OFF, il_order = PFNL_FIELD_TFF;
    uint8_t* fstore = nullptr;                        // [3][2][H/2][W][3] samples of the input depth: woven frame m in slot m % 3, its field of parity p at [p]
    long long woven = 0, woven_done = 0;              // woven frames pushed; of those, the ones that have become ring frames
    bool woven_mark[3] = {false, false, false};       // pfnl_stream_mark_cut's mark, travelling with the woven frame in the slot
    hipEvent_t il_ev = nullptr;                       // the newest use of the field store on the session's stream (device-pointer pushes, end)
    bool il_on_s = false;                             // ... that the copy stream has not yet been ordered behind
    // inverse telecine (pfnl_stream_telecine; telecine_geom.h): exclusive with interlacing, and on its field store, `woven`, the marks and
    // the event; woven_done counts the matched frames made
    int tc_mode = PFNL_TELECINE_OFF, tc_order = PFNL_FIELD_TFF;
    pfnl_telecine_params tc_par{};                    // with the defaults filled in
    uint8_t* tc_frames = nullptr;                     // [5][H][W][3] samples of the input depth: the matched frames of the current cycle (mode DECIMATE reads them)
    unsigned long long* tc_words = nullptr;           // device: the match's scratch [2] | the distance's scratch [2] | D [5] | stats [3] | decision [4]
    unsigned long long* tc_host = nullptr;            // pinned: D [5] of a complete cycle | stats [3]
    bool tc_mark[pfnl::TC_CYCLE] = {false, false, false, false, false};   // the marks of the cycle's pushed frames
    bool tc_carry = false;                            // the mark of a dropped last frame, on its way to the next cycle's first
    long long tc_dropped = 0, tc_admitted = 0;        // of the current sequence
    // the content box (pfnl_stream_bars; bars_geom.h): allocated by the first call that turns it on, with the ring's slots
    int bars_mode = 0, bars_limit = 0;                // 0 off | 1 every ring frame is measured as it is admitted
    int32_t* bars_box = nullptr;                      // device: box [cap][4], slot f % cap = frame f's | the kernel's scratch words (zero between launches)
    int32_t* bars_info[2] = {nullptr, nullptr};       // pinned host copies of box [cap][4], one per output slot: they travel with the batch
    hipEvent_t bars_ev = nullptr;                     // the newest measurement on the session's stream (device-pointer pushes)
    bool bars_on_s = false;                           // ... that a measurement on the copy stream has not yet been ordered behind
    bool has_box = false;                             // what pfnl_stream_pop_box and pfnl_stream_content_box return
    int32_t pop_box[4] = {0, 0, 0, 0}, seq_box[4] = {0, 0, 0, 0};
    long long box_frames = 0;
};

constexpr int TC_WORDS = 16, TC_AT_SAD = 2, TC_AT_D = 4, TC_AT_STATS = 9, TC_AT_DECISION = 12;

namespace {

// a frame of the current sequence has been pushed: the settings are fixed until pfnl_stream_reset
bool started(const pfnl_stream* s) { return s->pushed || s->woven; }

int get_option(pfnl_stream* s, const char* key, std::string* v) {
    char buf[64];
    if (int e = pfnl_get_option(s->h, key, buf, sizeof buf)) return e;
    *v = buf;
    return 0;
}

// The route on samples of T (uint8_t, or uint16_t for the 10-bit formats), each stage out of the slot of the one before it; a replay takes
// the same route, so pop stays a copy.  The launchers are overloaded on the sample type: one kernel body per stage (sample_depth.h).
template <typename T>
int run_route(pfnl_stream* s, const Batch& b) {
    constexpr bool ten = sizeof(T) == 2;
    const pfnl::OutRoute& r = s->route;
    const Setting& c = s->set;
    const pfnl::YuvCoef& coef = ten ? c.cout.coef10 : c.cout.coef;
    const auto slot = [&](int k) { return reinterpret_cast<T*>(s->slot[k].buf[b.slot]); };
    if (c.cin.prim != c.cout.prim)                    // the same levels, in the output's primaries: everything behind sees output-colour RGB
        HIPCHK(pfnl::launch_quantise_colour(s->sr, slot(0), (size_t)b.count * (s->sr_bytes / 3), s->ctab[ten ? 1 : 0], c.gamut, s->s));
    else
        HIPCHK(pfnl::launch_quantise(s->sr, slot(0), (size_t)b.count * s->sr_bytes, s->s));
    if (r.runs[1]) {                                  // one launch writes the whole canvas, the fill colour included (a plain size has none)
        const auto sample = [](uint8_t v) { return (T)(ten ? pfnl::fill_u10(v) : v); };
        const T fill[3] = {sample(s->rplan.fill[0]), sample(s->rplan.fill[1]), sample(s->rplan.fill[2])};
        HIPCHK(pfnl::launch_resize_place(slot(0), slot(1), s->rplan, s->rtab, fill, b.count, s->s));
    }
    const bool semiplanar = c.out_fmt == PFNL_PIX_NV12 || c.out_fmt == PFNL_PIX_P010;
    if (r.runs[2] && c.out_pack != PFNL_PACK_NONE)       // the tight packed frame: rows of pack_tight_pitch, frames of stage_bytes[2]
        HIPCHK(pfnl::launch_rgb_to_packed(slot(r.runs[1] ? 1 : 0), slot(2), pfnl::pack_tight_pitch(c.out_pack, r.out_w), r.stage_bytes[2], c.out_pack,
                                          coef, b.count, r.out_h, r.out_w, s->out_siting, s->s));
    else if (r.runs[2] && c.out_chroma == PFNL_CHROMA_420)    // reads the resampled frames where stage 1 runs
        HIPCHK(pfnl::launch_rgb_to_yuv420(slot(r.runs[1] ? 1 : 0), slot(2), semiplanar, coef, b.count, r.out_h, r.out_w, s->out_siting, s->s));
    else if (r.runs[2])
        HIPCHK(pfnl::launch_rgb_to_yuv_chroma(slot(r.runs[1] ? 1 : 0), slot(2), semiplanar, coef, b.count, r.out_h, r.out_w, c.out_chroma,
                                              s->out_siting, s->s));
    return 0;
}

// gather -> forward -> quantise (-> resize -> 4:2:0) into the batch's slots, then its event; asynchronous on the session's stream
int enqueue(pfnl_stream* s, const Batch& b) {
    const uint16_t* const ring10 = reinterpret_cast<const uint16_t*>(s->ring);   // (read at an input depth of 10 alone)
    if (s->scene_mode) {
        // every frame up to b.last has been decided: on this stream, or on the copy stream before its push returned.  A replay
        // (check_batch) reads the same entries: the push bound keeps a batch's slots until it has been delivered.
        if (s->set.in_depth == 10)
            HIPCHK(pfnl::launch_gather_windows_u10_scenes(ring10, s->scene_first, s->win, s->cap, b.last, b.first, b.count, s->T, s->in.ring_bytes, s->s));
        else
            HIPCHK(pfnl::launch_gather_windows_u8_scenes(s->ring, s->scene_first, s->win, s->cap, b.last, b.first, b.count, s->T, s->lr_bytes, s->s));
        HIPCHK(hipMemcpyAsync(s->info[b.slot], s->scene_first, 2 * (size_t)s->cap * sizeof(long long), hipMemcpyDeviceToHost, s->s));
    } else if (s->set.in_depth == 10) {
        HIPCHK(pfnl::launch_gather_windows_u10(ring10, s->win, s->cap, b.last, b.first, b.count, s->T, s->in.ring_bytes, s->s));
    } else {
        HIPCHK(pfnl::launch_gather_windows_u8(s->ring, s->win, s->cap, b.last, b.first, b.count, s->T, s->lr_bytes, s->s));
    }
    if (s->bars_mode)                                 // (every frame up to b.last has been measured, as it has been decided)
        HIPCHK(hipMemcpyAsync(s->bars_info[b.slot], s->bars_box, 4 * (size_t)s->cap * sizeof(int32_t), hipMemcpyDeviceToHost, s->s));
    // (no tiling: pfnl_forward_ensemble itself, and with 1 member pfnl_forward itself)
    if (int e = pfnl_forward_tiled(s->h, s->win, 1, s->sr, 1, b.count, s->H, s->W, s->tiled ? &s->tiling : nullptr, s->ensemble, s->s)) return e;
    if (int e = s->route.sample_bytes == 2 ? run_route<uint16_t>(s, b) : run_route<uint8_t>(s, b)) return e;
    HIPCHK(hipEventRecord(s->ev[b.slot], s->s));
    return 0;
}

// launches every batch the rule yields for which an output slot is free
int pump(pfnl_stream* s) {
    for (;;) {
        long long first = 0;
        int count = 0;
        if (int e = pfnl_stream_next_batch(s->T, s->batch, s->pushed, s->ended, s->launched, &first, &count)) return e;
        if (!count) return 0;
        const int slot = !s->slot_busy[0] ? 0 : (!s->slot_busy[1] ? 1 : -1);
        if (slot < 0) return 0;
        const Batch b{first, s->pushed - 1, count, slot, s->strict, false};
        if (int e = enqueue(s, b)) return e;
        s->slot_busy[slot] = true;
        s->launched += count;
        s->q.push_back(b);
    }
}

// The rest of the sequence on the kernels without a binary16 domain (pfnl_hip.h "strict_fp32"); under precision=bf16 that means
// precision=fp32 as well, as strict_fp32 changes nothing about that precision's non-local block and conv0.
int go_strict(pfnl_stream* s) {
    HIPCHK(hipStreamSynchronize(s->s));               // no forward of the old configuration is in flight when it changes
    std::string v;
    if (int e = get_option(s, "precision", &v)) return e;
    if (v == "bf16") {
        if (int e = pfnl_set_option(s->h, "precision", "fp32")) return e;
        s->prior_precision = v;
    }
    if (int e = get_option(s, "strict_fp32", &v)) return e;
    if (v != "on") {
        if (int e = pfnl_set_option(s->h, "strict_fp32", "on")) return e;
        s->prior_strict = v;
    }
    s->strict = true;
    return 0;
}

// back to what the library held before go_strict; only the keys it changed.  The caller has made sure nothing is in flight.
int restore_options(pfnl_stream* s) {
    int r = 0;
    if (!s->prior_strict.empty()) {
        if (int e = pfnl_set_option(s->h, "strict_fp32", s->prior_strict.c_str())) r = e;
        s->prior_strict.clear();
    }
    if (!s->prior_precision.empty()) {
        if (int e = pfnl_set_option(s->h, "precision", s->prior_precision.c_str())) r = e;
        s->prior_precision.clear();
    }
    s->strict = false;
    return r;
}

// The range fence, once per batch, before any of its frames leaves: wait for the batch, read the flag; a flagged batch - and every batch
// that was enqueued behind it before the flag was seen - is computed again on the strict kernels from the frames the ring still holds.
int check_batch(pfnl_stream* s, Batch& b) {
    HIPCHK(hipEventSynchronize(s->ev[b.slot]));
    if (!b.was_strict) {
        int flagged = 0;
        if (int e = pfnl_range_flag(s->h, &flagged)) return e;
        if (flagged || s->strict) {
            if (!s->strict)
                if (int e = go_strict(s)) return e;
            if (int e = enqueue(s, b)) return e;
            HIPCHK(hipEventSynchronize(s->ev[b.slot]));
            (void)pfnl_range_flag(s->h, &flagged);    // (strict path: the fence is not armed; clears a stale flag)
        }
    }
    b.checked = true;
    return 0;
}

// frame s->pushed has been copied into its slot on `on`: its sum against the frame before it and its scene, behind the copy
int decide_scene(pfnl_stream* s, hipStream_t on) {
    const long long f = s->pushed;
    const int slot = (int)(f % s->cap);
    if (f == 0) {
        HIPCHK(pfnl::launch_scene_first_frame(s->sad, s->scene_first, slot, on));
        return 0;
    }
    const int prev = (int)((f - 1) % s->cap);
    const pfnl::SceneDecision d{s->sad, s->scene_first, slot, prev, f, s->mark ? 1 : 0, s->scene_mode == 2 ? 1 : 0, s->thr_sum};
    const uint8_t* const a = s->ring + (size_t)slot * s->in.ring_bytes;
    const uint8_t* const b = s->ring + (size_t)prev * s->in.ring_bytes;
    if (s->set.in_depth == 10)
        HIPCHK(pfnl::launch_scene_sad_u10(reinterpret_cast<const uint16_t*>(a), reinterpret_cast<const uint16_t*>(b), (size_t)s->H * s->W,
                                          s->sad + s->cap, d, on));
    else
        HIPCHK(pfnl::launch_scene_sad_u8(a, b, (size_t)s->H * s->W, s->sad + s->cap, d, on));
    return 0;
}

// frame s->pushed is in its slot on `on`: its content box into the slot's entry, behind whatever put the frame there
int measure_bars(pfnl_stream* s, hipStream_t on) {
    const int slot = (int)(s->pushed % s->cap);
    const uint8_t* const a = s->ring + (size_t)slot * s->in.ring_bytes;
    uint32_t* const scratch = reinterpret_cast<uint32_t*>(s->bars_box + 4 * (size_t)s->cap);
    const pfnl::BarsOut out{s->bars_box + 4 * slot, nullptr, nullptr};
    if (s->set.in_depth == 10)
        HIPCHK(pfnl::launch_content_box(reinterpret_cast<const uint16_t*>(a), 1, s->H, s->W, s->bars_limit, scratch, out, on));
    else
        HIPCHK(pfnl::launch_content_box(a, 1, s->H, s->W, s->bars_limit, scratch, out, on));
    return 0;
}

// forgets the sequence: nothing in flight afterwards, options as before the session changed them
int drop_sequence(pfnl_stream* s) {
    int r = 0;
    if (hipStreamSynchronize(s->s) != hipSuccess || hipStreamSynchronize(s->cs) != hipSuccess)
        r = fail(PFNL_ERR_HIP, "stream synchronisation failed");
    bool unchecked = false;
    for (const Batch& b : s->q) unchecked = unchecked || !b.checked;
    if (unchecked) {                                  // a flag raised by a batch that is dropped must not fall on the next sequence
        int flagged = 0;
        (void)pfnl_range_flag(s->h, &flagged);
    }
    s->q.clear();
    s->slot_busy[0] = s->slot_busy[1] = false;
    s->pushed = s->launched = s->delivered = 0;
    s->ended = false;
    s->mark = s->decided_on_s = s->has_info = false;
    s->bars_on_s = s->has_box = false;                // (the kernel's scratch words are zero between launches)
    for (int k = 0; k < 4; ++k) s->pop_box[k] = s->seq_box[k] = 0;
    s->box_frames = 0;
    s->woven = s->woven_done = 0;                     // (both streams are idle: nothing reads the field store)
    s->woven_mark[0] = s->woven_mark[1] = s->woven_mark[2] = s->il_on_s = false;
    for (bool& m : s->tc_mark) m = false;
    s->tc_carry = false;
    s->tc_dropped = s->tc_admitted = 0;
    if (s->tc_words)                                  // the statistics are the sequence's (the scratch words are zero between launches)
        if (hipMemsetAsync(s->tc_words, 0, TC_WORDS * sizeof(unsigned long long), s->cs) != hipSuccess || hipStreamSynchronize(s->cs) != hipSuccess)
            r = fail(PFNL_ERR_HIP, "clearing the telecine statistics failed");
    if (int e = restore_options(s)) r = e;
    return r;
}

// What every push is, around the step that puts the frame into its ring slot as RGB: the state rules first (nothing has changed where
// one of them refuses), then on_device(slot) on the session's stream or on_host(slot) on the copy stream, the scene decision behind it,
// the synchronisation that frees the caller's host memory, and the batches the frame completes.
template <class OnDevice, class OnHost>
int push_frame(pfnl_stream* s, int is_device, OnDevice&& on_device, OnHost&& on_host) {
    if (s->ended) return fail(PFNL_ERR_STATE, "push after pfnl_stream_end (pfnl_stream_reset starts the next sequence)");
    long long first = 0;
    int count = 0;
    if (int e = pfnl_stream_next_batch(s->T, s->batch, s->pushed + 1, 0, s->launched, &first, &count)) return e;
    const long long oldest = s->q.empty() ? s->launched : s->q.front().first;
    const long long lo = oldest - s->T / 2 < 0 ? 0 : oldest - s->T / 2;
    if ((count && s->launched - s->delivered + count > 2LL * s->batch) || s->pushed - lo + 1 > s->cap)
        return fail(PFNL_ERR_STATE, "pop first: the session holds at most 2 * batch undelivered SR frames");
    HIPCHK(hipSetDevice(s->device));
    uint8_t* const dst = s->ring + (size_t)(s->pushed % s->cap) * s->in.ring_bytes;
    if (is_device) {
        if (int e = on_device(dst)) return e;
        if (s->scene_mode) {                          // behind the copy, ahead of any gather that can name the frame
            if (int e = decide_scene(s, s->s)) return e;
            HIPCHK(hipEventRecord(s->scene_ev, s->s));
            s->decided_on_s = true;
        }
        if (s->bars_mode) {                           // likewise: the frame's box is in its slot's entry ahead of any batch that names it
            if (int e = measure_bars(s, s->s)) return e;
            HIPCHK(hipEventRecord(s->bars_ev, s->s));
            s->bars_on_s = true;
        }
    } else {
        // the slot's previous frame belongs to batches that have been delivered, so nothing on the session's stream reads it; the copy
        // runs beside the batches in flight and the caller's buffer is free on return
        // With scenes on, the frame's sum and decision go on the copy stream as well, so that they are complete when push returns: on
        // the session's stream they could still be queued behind a long forward when the copy of frame f + cap - 1 overwrites the slot
        // they have yet to read.  They read the frame before and its decision, and share the sum's scratch: where those came through
        // device-pointer pushes they are on the session's stream, and the copy stream falls in behind them first.
        if (s->scene_mode && s->decided_on_s) {
            HIPCHK(hipStreamWaitEvent(s->cs, s->scene_ev, 0));
            s->decided_on_s = false;
        }
        if (s->bars_mode && s->bars_on_s) {           // (the measurement shares its scratch words as the scene sum does)
            HIPCHK(hipStreamWaitEvent(s->cs, s->bars_ev, 0));
            s->bars_on_s = false;
        }
        if (int e = on_host(dst)) return e;
        if (s->scene_mode)
            if (int e = decide_scene(s, s->cs)) return e;
        if (s->bars_mode)
            if (int e = measure_bars(s, s->cs)) return e;
        HIPCHK(hipStreamSynchronize(s->cs));
    }
    s->mark = false;
    ++s->pushed;
    return pump(s);
}

// What every pop is, around the copy that delivers: the batch at the front, checked (and replayed) once; deliver(src, bytes, on) copies
// the packed frame at src out on the session's stream (device pointers: ordered like the caller's own work there) or the copy stream
// (host pointers: the batch has completed, no wait for a later one; synchronised here); then the scene info, the index, the slot's
// release and the options' return.  *got = 0: no frame is deliverable and deliver has not run.
template <class Deliver>
int pop_frame(pfnl_stream* s, int is_device, long long* index, int* got, Deliver&& deliver) {
    *got = 0;
    HIPCHK(hipSetDevice(s->device));
    if (int e = pump(s)) return e;
    if (s->q.empty()) return 0;
    Batch& b = s->q.front();
    if (!b.checked)
        if (int e = check_batch(s, b)) return e;
    const size_t bytes = s->route.frame_bytes;
    const uint8_t* const src = s->slot[s->route.last].buf[b.slot] + (size_t)(s->delivered - b.first) * bytes;
    if (is_device) {
        if (int e = deliver(src, bytes, s->s)) return e;
    } else {
        if (int e = deliver(src, bytes, s->cs)) return e;
        HIPCHK(hipStreamSynchronize(s->cs));
    }
    if (s->scene_mode) {                              // (the copy is ahead of the batch's event, which check_batch has waited for)
        const int slot = (int)(s->delivered % s->cap);
        s->info_first = s->info[b.slot][slot];
        s->info_sad = (unsigned long long)s->info[b.slot][s->cap + slot];
    } else {
        s->info_first = 0;
        s->info_sad = 0;
    }
    s->has_info = true;
    if (s->bars_mode) {                               // (copied ahead of the batch's event as well)
        const int32_t* const box = s->bars_info[b.slot] + 4 * (size_t)(s->delivered % s->cap);
        for (int k = 0; k < 4; ++k) s->pop_box[k] = box[k];
        pfnl::bars_union(s->seq_box, box);
        ++s->box_frames;
        s->has_box = true;
    }
    *index = s->delivered++;
    *got = 1;
    if (s->delivered == b.first + b.count) {
        s->slot_busy[b.slot] = false;                 // (a device-pointer copy out of it is ahead of the next batch on the same stream)
        s->q.pop_front();
        if (int e = pump(s)) return e;
        if (s->ended && s->delivered == s->pushed) return restore_options(s);   // (every forward has completed: its batch was checked)
    }
    return 0;
}

// ---- the input route (stream_route.h InRoute, stored as s->in): a pushed surface -> RGB rows at `dst` ----

// a tightly packed pushed frame at `base` as the surface it is: its planes one behind the other at the route's tight pitches
pfnl_surface tight_surface(const pfnl_stream* s, const uint8_t* base) {
    pfnl_surface sf{};
    for (int k = 0; k < s->in.geom.planes; ++k) {
        sf.plane[k] = const_cast<uint8_t*>(base);
        sf.pitch[k] = s->in.pitch[k];
        base += s->in.geom.plane[k].rows * sf.pitch[k];
    }
    return sf;
}

// The one decode: `rows` rows of the surface `sf` of the session's input setting (the frame: H; one of its fields: H / 2) -> RGB at dst,
// on `on`.  The only place that looks at the decode kind and the sample depth.  sf lies on the device; planar RGB is a copy and may lie
// in host memory (from_host).
// A tight frame comes here as tight_surface(), so the plane launchers see a frame stride of 0 where the tight launchers of yuv.hip /
// yuv_chroma.hip pass the tight frame's bytes.  With n = 1 the stride enters the choice of the strip width alone (decode_strip_width,
// strip_of), and never changes it: a strip of P samples needs W % P == 0, and the tight frame is H W 3/2 = (H / 2) 3 W samples at 4:2:0
// (H even), 2 H W at 4:2:2, 3 H W at 4:4:4 - a multiple of W samples, so its bytes are a multiple of the P-sample word whenever W is.
int decode_surface(pfnl_stream* s, const pfnl_surface& sf, int rows, uint8_t* dst, bool from_host, hipStream_t on) {
    const Setting& c = s->set;
    const bool ten = s->in.sample_bytes == 2, nv12 = c.in_fmt == PFNL_PIX_NV12;
    const pfnl::YuvCoef& coef = ten ? c.cin.coef10 : c.cin.coef;
    const pfnl::YuvPlanes yuv = pfnl_internal_yuv_planes(sf, nv12);   // (read by the two YUV kinds alone)
    uint16_t* const dst10 = reinterpret_cast<uint16_t*>(dst);
    const size_t row = s->in.geom.plane[0].row_bytes;
    const hipMemcpyKind copy = from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    switch (s->in.kind) {
    case pfnl::IN_DECODE_PACK:
        HIPCHK(pfnl::launch_packed_to_rgb(sf.plane[0], sf.pitch[0], 0, c.in_pack, dst, coef, 1, rows, s->W, s->in_siting, on));
        return 0;
    case pfnl::IN_DECODE_CHROMA:
        HIPCHK(ten ? pfnl::launch_yuv_planes_to_rgb_chroma(yuv, dst10, nv12, coef, 1, rows, s->W, c.in_chroma, s->in_siting, on)
                   : pfnl::launch_yuv_planes_to_rgb_chroma(yuv, dst, nv12, coef, 1, rows, s->W, c.in_chroma, s->in_siting, on));
        return 0;
    case pfnl::IN_DECODE_420:
        HIPCHK(ten ? pfnl::launch_yuv420_planes_to_rgb_u10(yuv, dst10, nv12, coef, 1, rows, s->W, s->in_siting, on)
                   : pfnl::launch_yuv420_planes_to_rgb_u8(yuv, dst, nv12, coef, 1, rows, s->W, s->in_siting, on));
        return 0;
    case pfnl::IN_DECODE_COPY:                        // rows that abut: one copy
        HIPCHK(sf.pitch[0] == row ? hipMemcpyAsync(dst, sf.plane[0], rows * row, copy, on)
                                  : hipMemcpy2DAsync(dst, row, sf.plane[0], sf.pitch[0], row, rows, copy, on));
        return 0;
    }
    return fail(PFNL_ERR_STATE, "the session has no input route");   // (IN_DECODE_NONE: apply_setting stores no such setting)
}

// The one staging step of a host push, on the copy stream: the caller's planes into the staging frame at the tight pitches (it is free
// again: every push ends with the copy stream idle); *at = where the decode finds the frame.  Planar RGB has no staging frame: the decode
// copies it from where it lies.  Planes that are tight and abut move in one copy - up to the last row's samples, as a surface promises
// nothing behind them - else each plane in a 2-D copy of its rows' samples.
int stage_host(pfnl_stream* s, const pfnl_surface& frame, pfnl_surface* at) {
    *at = frame;
    if (!s->in.staging_bytes) return 0;
    *at = tight_surface(s, s->yin);
    const pfnl::SurfaceGeom& g = s->in.geom;
    const pfnl_surface tight = tight_surface(s, static_cast<const uint8_t*>(frame.plane[0]));
    bool abut = true;
    for (int k = 0; k < g.planes; ++k) abut = abut && frame.plane[k] == tight.plane[k] && frame.pitch[k] == tight.pitch[k];
    const int last = g.planes - 1;
    if (abut) {
        HIPCHK(hipMemcpyAsync(s->yin, frame.plane[0], s->in.frame_bytes - (s->in.pitch[last] - g.plane[last].row_bytes), hipMemcpyHostToDevice, s->cs));
        return 0;
    }
    for (int k = 0; k < g.planes; ++k)
        HIPCHK(hipMemcpy2DAsync(at->plane[k], at->pitch[k], frame.plane[k], frame.pitch[k], g.plane[k].row_bytes, g.plane[k].rows, hipMemcpyHostToDevice, s->cs));
    return 0;
}

// ---- interlaced input (include/pfnl_hip.h INTERLACED): woven frames -> decoded fields in the field store -> progressive ring frames ----

uint8_t* field_at(const pfnl_stream* s, long long k) {    // field k of the sequence, in the slot of its frame
    return s->fstore + ((size_t)(pfnl::field_frame(k) % 3) * 2 + pfnl::field_parity(k, s->tc_mode ? s->tc_order : s->il_order)) * (s->in.ring_bytes / 2);
}

// The field of parity p of the woven frame `frame` (device planes; an RGB frame's may be host memory: from_host) -> its place in the slot
// of woven frame s->woven, as RGB, by the launch that decodes a progressive frame of this setting - on a surface of H / 2 rows.
int decode_field(pfnl_stream* s, const pfnl_surface& frame, int p, bool from_host, hipStream_t on) {
    uint8_t* const dst = s->fstore + ((size_t)(s->woven % 3) * 2 + p) * (s->in.ring_bytes / 2);
    return decode_surface(s, pfnl::field_surface(frame, s->in.geom.planes, p), s->H / 2, dst, from_host, on);
}


pfnl::RingCounters ring_counters(const pfnl_stream* s) {
    return pfnl::RingCounters{s->pushed, s->launched, s->delivered, (int)s->q.size(), s->q.empty() ? 0 : s->q.front().first};
}

// the ring frames of woven frame s->woven_done, one launch, into the slots of ring frames s->pushed ..
template <typename T>
int launch_woven(pfnl_stream* s, int yield, hipStream_t on) {
    const long long n = s->woven_done, fields = 2 * s->woven;
    pfnl::DeinterlaceJob<T> job[2];
    for (int i = 0; i < yield; ++i) {
        const long long k = 2 * n + i;
        const auto at = [&](long long q) { return reinterpret_cast<const T*>(field_at(s, pfnl::field_replace(q, fields))); };
        job[i] = pfnl::DeinterlaceJob<T>{at(k - 2), at(k - 1), at(k), at(k + 1), at(k + 2),
                                         reinterpret_cast<T*>(s->ring + (size_t)((s->pushed + i) % s->cap) * s->in.ring_bytes), pfnl::field_parity(k, s->il_order)};
    }
    HIPCHK(pfnl::launch_deinterlace(job, yield, s->H, s->W, on));
    return 0;
}

// Woven frame s->woven_done becomes its ring frames: the kernel writes them into their slots in one launch, and each is admitted as a
// progressive push admits a frame (push_frame: the scene decision behind it, `pushed`, pump).  The caller has seen that the bound admits
// them all.  The frame's mark lands on the first of them.
int admit_woven(pfnl_stream* s, int is_device) {
    const int yield = pfnl::interlace_yield(s->il_mode);
    s->mark = s->woven_mark[s->woven_done % 3];
    for (int i = 0; i < yield; ++i) {
        const auto make = [&](hipStream_t on) {           // (the second frame's slot was written with the first's)
            if (i) return 0;
            return s->set.in_depth == 10 ? launch_woven<uint16_t>(s, yield, on) : launch_woven<uint8_t>(s, yield, on);
        };
        if (int e = push_frame(s, is_device, [&](uint8_t*) { return make(s->s); }, [&](uint8_t*) { return make(s->cs); })) return e;
    }
    ++s->woven_done;
    return 0;
}

// ---- inverse telecine (include/pfnl_hip.h TELECINE): the field store's fields -> matched frames -> the ring, all of them or four in five ----

// Matched frame n into `out` on `on`: the match, which leaves its decision on the device; with post on the deinterlacer's frame at the time
// of field 2 n, which a flagged frame keeps; the weave, which in mode DECIMATE also sums D_n against the matched frame before it.
template <typename T>
int make_matched(pfnl_stream* s, long long n, uint8_t* out, hipStream_t on) {
    const long long fields = 2 * s->woven, k = 2 * n;
    const pfnl::MatchFields mf = pfnl::telecine_match_fields(n, fields);
    const auto at = [&](long long q) { return reinterpret_cast<const T*>(field_at(s, pfnl::field_replace(q, fields))); };
    const int h = s->H / 2, parity = pfnl::field_parity(k, s->tc_order), slot = pfnl::telecine_cycle_slot(n);
    const bool decimate = s->tc_mode == PFNL_TELECINE_DECIMATE;
    unsigned long long* const w = s->tc_words;
    HIPCHK(pfnl::launch_telecine_match(at(mf.a), at(mf.c), at(mf.p), h, s->W, parity, s->tc_par.threshold, w,
                                       pfnl::TelecineDecide{w + TC_AT_DECISION, w + TC_AT_STATS, s->tc_par.post, (unsigned long long)s->tc_par.comb_limit}, on));
    if (s->tc_par.post)
        HIPCHK(pfnl::launch_deinterlace(at(k - 2), at(k - 1), at(k), at(k + 1), at(k + 2), s->H, s->W, parity, reinterpret_cast<T*>(out), on));
    const uint8_t* const prev = decimate && n ? s->tc_frames + (size_t)pfnl::telecine_cycle_slot(n - 1) * s->in.ring_bytes : nullptr;
    HIPCHK(pfnl::launch_telecine_weave(at(mf.a), at(mf.c), at(mf.p), h, s->W, parity, w + TC_AT_DECISION, reinterpret_cast<T*>(out),
                                       reinterpret_cast<const T*>(prev), decimate ? w + TC_AT_SAD : nullptr, decimate ? w + TC_AT_D + slot : nullptr, on));
    return 0;
}

// Pushed frame s->woven_done becomes its matched frame, and that whatever it completes.  Mode MATCH: written straight into its ring slot and
// admitted as a progressive push admits a frame.  Mode DECIMATE: written into its place in the cycle; the cycle's last frame (at_end: the
// sequence's) has the host wait - once per cycle - for the cycle's five D, and the kept frames are copied into their ring slots and
// admitted in order, each with the mark that lands on it.  The caller has seen that the bound admits them all.
int admit_matched(pfnl_stream* s, int is_device, bool at_end) {
    const hipStream_t on = is_device ? s->s : s->cs;
    const long long n = s->woven_done;
    const bool ten = s->set.in_depth == 10;
    const auto make = [&](uint8_t* dst, hipStream_t q) { return ten ? make_matched<uint16_t>(s, n, dst, q) : make_matched<uint8_t>(s, n, dst, q); };
    if (s->tc_mode == PFNL_TELECINE_MATCH) {
        s->mark = s->woven_mark[n % 3];
        if (int e = push_frame(s, is_device, [&](uint8_t* dst) { return make(dst, s->s); }, [&](uint8_t* dst) { return make(dst, s->cs); })) return e;
        ++s->woven_done;
        ++s->tc_admitted;
        return 0;
    }
    const int slot = pfnl::telecine_cycle_slot(n);
    if (int e = make(s->tc_frames + (size_t)slot * s->in.ring_bytes, on)) return e;
    s->tc_mark[slot] = s->woven_mark[n % 3];
    ++s->woven_done;
    const bool complete = slot == pfnl::TC_CYCLE - 1;
    if (!complete && !at_end) {
        if (!is_device) HIPCHK(hipStreamSynchronize(s->cs));          // (the caller's memory is free on return)
        return 0;
    }
    int drop = -1;
    if (complete) {
        HIPCHK(hipMemcpyAsync(s->tc_host, s->tc_words + TC_AT_D, pfnl::TC_CYCLE * sizeof(unsigned long long), hipMemcpyDeviceToHost, on));
        // The D depend on the frame this push decoded on `on`.  For a device-pointer push that is the session's stream - the caller's frame
        // is read in the caller's order - so this also waits for the forwards queued there, once per cycle; an event behind the copy
        // would complete no earlier on an in-order stream, and the copy stream cannot run ahead of a decode it must follow.
        HIPCHK(hipStreamSynchronize(on));
        drop = pfnl::telecine_drop_index(s->tc_host);
        ++s->tc_dropped;
    }
    bool marks[pfnl::TC_CYCLE];
    (void)pfnl::telecine_place_marks(s->tc_mark, slot + 1, drop, &s->tc_carry, marks);
    for (int j = 0, i = 0; j <= slot; ++j) {
        if (j == drop) continue;
        const uint8_t* const src = s->tc_frames + (size_t)j * s->in.ring_bytes;
        const auto copy = [&](uint8_t* dst, hipStream_t q) {
            HIPCHK(hipMemcpyAsync(dst, src, s->in.ring_bytes, hipMemcpyDeviceToDevice, q));
            return 0;
        };
        s->mark = marks[i++];
        if (int e = push_frame(s, is_device, [&](uint8_t* dst) { return copy(dst, s->s); }, [&](uint8_t* dst) { return copy(dst, s->cs); })) return e;
        ++s->tc_admitted;
    }
    return 0;
}

// What every push is with interlacing or inverse telecine on: the bound for every ring frame the push completes, on copies of the
// counters (nothing has changed where it refuses); the frame's two fields decoded into the slot of the field store - device pointers on
// the session's stream, host pointers on the copy stream, YUV and packings through the staging frame -; then the woven frame before it,
// which now has both neighbours, becomes its ring frames (admit_woven), or its matched frame and whatever that completes (admit_matched).
// The field store, and telecine's cycle and device words with it, is used on one stream at a time: the copy stream is idle when a push returns, and
// falls in behind the session's stream's newest use of it first.
int push_woven(pfnl_stream* s, int is_device, const pfnl_surface& frame) {
    if (s->ended) return fail(PFNL_ERR_STATE, "push after pfnl_stream_end (pfnl_stream_reset starts the next sequence)");
    const int yield = s->tc_mode ? pfnl::telecine_push_yield(s->tc_mode, s->woven) : (s->woven ? pfnl::interlace_yield(s->il_mode) : 0);
    pfnl::RingCounters c = ring_counters(s);
    if (!pfnl::ring_admit_all(s->T, s->batch, s->cap, yield, &c))
        return fail(PFNL_ERR_STATE, "pop first: the session holds at most 2 * batch undelivered SR frames");
    HIPCHK(hipSetDevice(s->device));
    if (!is_device && s->il_on_s) {
        HIPCHK(hipStreamWaitEvent(s->cs, s->il_ev, 0));
        s->il_on_s = false;
    }
    pfnl_surface from = frame;
    if (!is_device)
        if (int e = stage_host(s, frame, &from)) return e;
    for (int p = 0; p < 2; ++p)
        if (int e = decode_field(s, from, p, !is_device && !s->in.staging_bytes, is_device ? s->s : s->cs)) return e;
    s->woven_mark[s->woven % 3] = s->mark;
    s->mark = false;
    ++s->woven;
    int r = 0;
    if (s->tc_mode && s->woven > 1)                   // (a matched frame is made whether or not it completes a ring frame)
        r = admit_matched(s, is_device, false);
    else if (yield)
        r = admit_woven(s, is_device);
    else if (!is_device)
        HIPCHK(hipStreamSynchronize(s->cs));          // (the caller's memory is free on return)
    if (is_device) {
        HIPCHK(hipEventRecord(s->il_ev, s->s));
        s->il_on_s = true;
    }
    return r;
}

// where both push entries end, each with its own argument checks behind it: the frame as a surface of the input route
int push_surface(pfnl_stream* s, const pfnl_surface& frame, int is_device) {
    if (s->il_mode || s->tc_mode) return push_woven(s, is_device, frame);
    return push_frame(
        s, is_device, [&](uint8_t* dst) { return decode_surface(s, frame, s->H, dst, false, s->s); },   // the kernel reads the surface where it lies
        [&](uint8_t* dst) {
            pfnl_surface from;
            if (int e = stage_host(s, frame, &from)) return e;
            return decode_surface(s, from, s->H, dst, !s->in.staging_bytes, s->cs);
        });
}

void drop_slot(StageSlot& t) {
    for (uint8_t* p : t.buf)
        if (p) (void)hipFree(p);
    t = StageSlot();
}

void release(pfnl_stream* s) {
    for (StageSlot& t : s->slot) drop_slot(t);
    for (int i = 0; i < 2; ++i) {
        if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
        if (s->info[i]) (void)hipHostFree(s->info[i]);
    }
    if (s->scene_first) (void)hipFree(s->scene_first);
    if (s->scene_ev) (void)hipEventDestroy(s->scene_ev);
    for (int32_t* p : s->bars_info)
        if (p) (void)hipHostFree(p);
    if (s->bars_box) (void)hipFree(s->bars_box);
    if (s->bars_ev) (void)hipEventDestroy(s->bars_ev);
    if (s->yin) (void)hipFree(s->yin);
    if (s->fstore) (void)hipFree(s->fstore);
    if (s->il_ev) (void)hipEventDestroy(s->il_ev);
    if (s->tc_frames) (void)hipFree(s->tc_frames);
    if (s->tc_words) (void)hipFree(s->tc_words);
    if (s->tc_host) (void)hipHostFree(s->tc_host);
    if (s->rtab) (void)hipFree(s->rtab);
    if (s->ring) (void)hipFree(s->ring);
    if (s->win) (void)hipFree(s->win);
    if (s->sr) (void)hipFree(s->sr);
    if (s->cs) (void)hipStreamDestroy(s->cs);
    delete s;
}

// The one place where a setting becomes the session's: every setter ends here, with a candidate they have validated and no frame pushed
// (`plan` NULL: the output size stays).  1. the two routes: a batch's bytes per stage, the pushed frame's ring and staging bytes; 2. everything new first - a stage slot whose capacity
// is below the need (stage 2's follows the output packing's row bytes, the staging frame the input packing's), the tap table of a new plan, the ring of another input depth, the staging frame of the first YUV in_fmt or of one at
// a wider depth or subsampling (so whichever of pfnl_stream_format, pfnl_stream_input_depth and pfnl_stream_chroma_format comes later makes it) - and where one fails, what was just made is
// freed, the session is what it was and the answer is PFNL_ERR_NOMEM with `nomem`; 3. the new buffers go in, the ones they replace and the
// slots of stages the route does not run are freed, the setting is stored.  A call that replaces or releases device memory first waits
// for the session's stream - a dropped sequence's device-pointer pops may still be reading it - and only such a call: pfnl_stream_format
// waits where a 10-bit format meets 8-bit slots or a 4:2:0 slot is no longer needed, and not where it only adds memory or changes none.
int apply_setting(pfnl_stream* s, const Setting& c, pfnl::PlacePlan* plan, const char* nomem) {
    const pfnl::PlacePlan& rp = plan ? *plan : s->rplan;
    const pfnl::OutRoute route = pfnl::out_route(c.out_fmt, s->scale * s->H, s->scale * s->W, rp.cH, rp.cW, c.out_chroma, c.out_pack);   // (the delivered frame is the canvas)
    const pfnl::InRoute in = pfnl::in_route(c.in_fmt, c.in_depth, c.in_chroma, c.in_pack, s->H, s->W);
    StageSlot fresh[pfnl::ROUTE_STAGES];              // cap != 0: the stage's slot is too small and this one takes its place
    const size_t in_bytes = in.ring_bytes, yin_need = in.staging_bytes;
    const bool regauged = c.in_depth != s->set.in_depth;   // the ring, and the field store with it, hold samples of another size
    bool frees = (plan && s->rtab) || regauged || (yin_need > s->yin_cap && s->yin);
    for (int k = 0; k < pfnl::ROUTE_STAGES; ++k) {
        const size_t need = (size_t)s->batch * route.stage_bytes[k];   // (0 for a stage that does not run)
        if (need > s->slot[k].cap) fresh[k].cap = need;
        frees = frees || (s->slot[k].cap && (fresh[k].cap || !route.runs[k]));
    }
    HIPCHK(hipSetDevice(s->device));
    if (frees) HIPCHK(hipStreamSynchronize(s->s));
    int32_t* tab = nullptr;
    uint8_t *yin = nullptr, *ring = nullptr, *fstore = nullptr, *cycle = nullptr;   // (the field store and telecine's cycle follow the ring's depth)
    bool ok = true;
    if (plan && plan->cH) {
        const std::vector<int32_t>& blob = plan->r.blob;
        ok = hipMalloc(reinterpret_cast<void**>(&tab), blob.size() * sizeof(int32_t)) == hipSuccess;
        pfnl::BlockingCopyGuard guard;                                           // (never beside another handle's graph capture: common.h)
        ok = ok && hipMemcpy(tab, blob.data(), blob.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (regauged) ok = ok && hipMalloc(reinterpret_cast<void**>(&ring), (size_t)s->cap * in_bytes) == hipSuccess;
    if (regauged && s->fstore) ok = ok && hipMalloc(reinterpret_cast<void**>(&fstore), 3 * in_bytes) == hipSuccess;
    if (regauged && s->tc_frames) ok = ok && hipMalloc(reinterpret_cast<void**>(&cycle), pfnl::TC_CYCLE * in_bytes) == hipSuccess;
    if (yin_need > s->yin_cap) ok = ok && hipMalloc(reinterpret_cast<void**>(&yin), yin_need) == hipSuccess;
    for (StageSlot& t : fresh)
        for (int i = 0; i < 2 && t.cap; ++i) ok = ok && hipMalloc(reinterpret_cast<void**>(&t.buf[i]), t.cap) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (tab) (void)hipFree(tab);
        if (yin) (void)hipFree(yin);
        if (ring) (void)hipFree(ring);
        if (fstore) (void)hipFree(fstore);
        if (cycle) (void)hipFree(cycle);
        for (StageSlot& t : fresh) drop_slot(t);
        return fail(PFNL_ERR_NOMEM, nomem);
    }
    if (plan) {
        if (s->rtab) (void)hipFree(s->rtab);
        s->rtab = tab;
        s->rplan = std::move(*plan);
    }
    if (yin) {
        if (s->yin) (void)hipFree(s->yin);
        s->yin = yin;
        s->yin_cap = yin_need;
    }
    if (ring) {
        (void)hipFree(s->ring);
        s->ring = ring;
    }
    if (fstore) {
        (void)hipFree(s->fstore);
        s->fstore = fstore;
    }
    if (cycle) {
        (void)hipFree(s->tc_frames);
        s->tc_frames = cycle;
    }
    for (int k = 0; k < pfnl::ROUTE_STAGES; ++k)
        if (fresh[k].cap || !route.runs[k]) {
            drop_slot(s->slot[k]);
            s->slot[k] = fresh[k];
        }
    s->set = c;
    s->route = route;
    s->in = in;
    // a tight v210 frame has zero bytes behind the samples of a row, and the kernel writes samples alone: the slot is cleared once, here
    for (int i = 0; i < 2 && c.out_pack == PFNL_PACK_V210; ++i) HIPCHK(hipMemsetAsync(s->slot[2].buf[i], 0, s->slot[2].cap, s->s));
    return 0;
}

}  // namespace

extern "C" {

int pfnl_stream_next_batch(int T, int batch, long long pushed, int ended, long long launched, long long* first, int* count) {
    if (!first || !count) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (T < 1 || !(T & 1) || batch < 1 || launched < 0 || pushed < launched)
        return fail(PFNL_ERR_INVALID, "next_batch: T odd, batch >= 1, 0 <= launched <= pushed");
    *first = launched;
    if (ended)
        *count = (int)(pushed - launched < batch ? pushed - launched : batch);
    else
        *count = pushed >= launched + batch + T / 2 ? batch : 0;   // the last window's newest frame, index + T/2, is present
    return 0;
}

int pfnl_stream_open(pfnl_handle* h, int H, int W, int batch, void* hip_stream, pfnl_stream** out) {
    if (!h || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (batch < 1) return fail(PFNL_ERR_INVALID, "batch must be at least 1");
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1))
        return fail(PFNL_ERR_INVALID, "H and W must be positive and even (space_to_depth(2), reference model/pfnl.py:57)");
    const pfnl_handle_view v = pfnl_internal_view(h);
    if (!v.finalized) return fail(PFNL_ERR_STATE, "pfnl_finalize_weights has not been called");
    if (*v.session) return fail(PFNL_ERR_STATE, "the handle already has an open session (a handle is not re-entrant): close it first");
    if ((long long)batch * v.num_frames > (1 << 30)) return fail(PFNL_ERR_INVALID, "batch too large");
    HIPCHK(hipSetDevice(v.device_id));
    pfnl_stream* s = new pfnl_stream();
    s->h = h;
    s->H = H;
    s->W = W;
    s->batch = batch;
    s->T = v.num_frames;
    s->scale = v.scale;
    s->device = v.device_id;
    s->s = hip_stream ? (hipStream_t)hip_stream : v.stream;
    s->lr_bytes = (size_t)H * W * 3;
    s->in = pfnl::in_route(s->set.in_fmt, s->set.in_depth, s->set.in_chroma, s->set.in_pack, H, W);   // planar RGB24: ring frames of lr_bytes
    s->sr_bytes = s->lr_bytes * v.scale * v.scale;
    // The ring keeps a batch's frames until the batch has been checked (it may have to be computed again): with two batches undelivered,
    // the oldest needed frame is launched - 2 batch - T/2, and pushes go on up to launched + batch + T/2 - 2 before the one that would
    // launch a third batch is refused: 3 batch + T - 2 frames.
    s->cap = 3 * batch + s->T - 2;
    bool ok = hipStreamCreateWithFlags(&s->cs, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&s->ring), (size_t)s->cap * s->lr_bytes) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&s->win), (size_t)batch * s->T * s->lr_bytes * sizeof(float)) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&s->sr), (size_t)batch * s->sr_bytes * sizeof(float)) == hipSuccess;
    s->route = pfnl::out_route(s->set.out_fmt, v.scale * H, v.scale * W, 0, 0);   // RGB24 at the network's raster: stage 0 alone
    s->slot[0].cap = (size_t)batch * s->route.stage_bytes[0];
    for (int i = 0; i < 2; ++i) {
        ok = ok && hipMalloc(reinterpret_cast<void**>(&s->slot[0].buf[i]), s->slot[0].cap) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        release(s);
        return fail(PFNL_ERR_NOMEM, "session allocation failed");
    }
    *v.session = s;
    *out = s;
    return 0;
}

int pfnl_stream_push(pfnl_stream* s, const uint8_t* frame, int is_device) {
    if (!s || !frame) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (s->set.in_depth == 10 && reinterpret_cast<uintptr_t>(frame) % 2) return fail(PFNL_ERR_INVALID, "push: uint16 samples are 2-byte aligned");
    if (is_device && s->set.in_pack != PFNL_PACK_NONE && reinterpret_cast<uintptr_t>(frame) % pfnl::PACK_TABLE[s->set.in_pack].align)
        return fail(PFNL_ERR_INVALID, "push: a packed frame of 32-bit words (x2rgb10, x2bgr10, v210) is 4-byte aligned");
    // (no surface_refused: a host frame of an 8-bit packing may lie at any address, and the tight pitches are the route's own)
    return push_surface(s, tight_surface(s, frame), is_device);
}

int pfnl_stream_push_surface(pfnl_stream* s, const pfnl_surface* frame, int is_device) {
    if (!s || !frame) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (const char* why = pfnl::surface_refused(frame, s->in.fmt, s->H, s->W, s->set.in_chroma, s->set.in_pack)) return fail(PFNL_ERR_INVALID, why);
    return push_surface(s, *frame, is_device);
}

int pfnl_stream_end(pfnl_stream* s) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(s->device));
    if (s->tc_mode && !s->ended && s->woven > s->woven_done) {   // the held frame and what it completes, under a push's bound
        pfnl::RingCounters c = ring_counters(s);
        if (!pfnl::ring_admit_all(s->T, s->batch, s->cap, pfnl::telecine_end_yield(s->tc_mode, s->woven, s->woven_done), &c))
            return fail(PFNL_ERR_STATE, "pop first: the session holds at most 2 * batch undelivered SR frames");
        const int r = admit_matched(s, 1, true);      // (on the session's stream: the copy stream is idle between calls)
        HIPCHK(hipEventRecord(s->il_ev, s->s));
        s->il_on_s = true;
        if (r) return r;
    }
    if (s->il_mode && !s->ended && s->woven > s->woven_done) {   // the held frame first, under a push's bound: its fields past the end repeat
        pfnl::RingCounters c = ring_counters(s);
        if (!pfnl::ring_admit_all(s->T, s->batch, s->cap, pfnl::interlace_yield(s->il_mode), &c))
            return fail(PFNL_ERR_STATE, "pop first: the session holds at most 2 * batch undelivered SR frames");
        const int r = admit_woven(s, 1);              // (on the session's stream: the copy stream is idle between calls)
        HIPCHK(hipEventRecord(s->il_ev, s->s));
        s->il_on_s = true;
        if (r) return r;
    }
    s->ended = true;
    if (int e = pump(s)) return e;
    if (s->delivered == s->pushed) return restore_options(s);   // (nothing left to pop: nothing in flight either)
    return 0;
}

int pfnl_stream_ready(pfnl_stream* s, int* frames) {
    if (!s || !frames) return fail(PFNL_ERR_INVALID, "NULL argument");
    *frames = (int)((s->ended ? s->pushed : s->launched) - s->delivered);
    return 0;
}

int pfnl_stream_pop(pfnl_stream* s, uint8_t* out, int is_device, long long* index, int* got) {
    if (!s || !out || !index || !got) return fail(PFNL_ERR_INVALID, "NULL argument");
    return pop_frame(s, is_device, index, got, [&](const uint8_t* src, size_t bytes, hipStream_t on) {
        HIPCHK(hipMemcpyAsync(out, src, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, on));
        return 0;
    });
}

int pfnl_stream_pop_surface(pfnl_stream* s, const pfnl_surface* out, int is_device, long long* index, int* got) {
    if (!s || !out || !index || !got) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (const char* why = pfnl::surface_refused(out, s->set.out_fmt, s->route.out_h, s->route.out_w, s->set.out_chroma, s->set.out_pack))
        return fail(PFNL_ERR_INVALID, why);
    const pfnl::SurfaceGeom g = pfnl::surface_geom(s->set.out_fmt, s->route.out_h, s->route.out_w, s->set.out_chroma, s->set.out_pack);
    return pop_frame(s, is_device, index, got, [&](const uint8_t* src, size_t, hipStream_t on) {
        if (s->set.out_pack != PFNL_PACK_NONE) {          // one plane; the slot's rows lie at the tight frame's pitch, and only a row's samples move
            HIPCHK(hipMemcpy2DAsync(out->plane[0], out->pitch[0], src, pfnl::pack_tight_pitch(s->set.out_pack, s->route.out_w), g.plane[0].row_bytes,
                                    g.plane[0].rows, is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, on));
            return 0;
        }
        for (int k = 0; k < g.planes; ++k) {          // the packed frame is its planes one behind the other: rows of row_bytes, nothing between
            HIPCHK(hipMemcpy2DAsync(out->plane[k], out->pitch[k], src, g.plane[k].row_bytes, g.plane[k].row_bytes, g.plane[k].rows,
                                    is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, on));
            src += g.plane[k].rows * g.plane[k].row_bytes;
        }
        return 0;
    });
}

int pfnl_stream_ensemble(pfnl_stream* s, int n) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (n != 1 && n != 2 && n != 4 && n != 8) return fail(PFNL_ERR_INVALID, "ensemble: n must be 1, 2, 4 or 8");
    if (started(s)) return fail(PFNL_ERR_STATE, "the ensemble is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    s->ensemble = n;
    return 0;
}

int pfnl_stream_tile(pfnl_stream* s, const pfnl_tiling* t) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (t)
        if (const char* why = pfnl::tiling_refused(s->H, s->W, *t)) return fail(PFNL_ERR_INVALID, why);
    if (started(s)) return fail(PFNL_ERR_STATE, "the tiling is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    s->tiled = t != nullptr;
    s->tiling = t ? *t : pfnl_tiling{};
    return 0;
}

int pfnl_stream_scenes(pfnl_stream* s, int mode, double threshold) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (mode < 0 || mode > 2) return fail(PFNL_ERR_INVALID, "scenes: mode 0 (off), 1 (marks) or 2 (marks and the detector)");
    if (mode == 2 && !(threshold > 0.0 && threshold <= 255.0))
        return fail(PFNL_ERR_INVALID, "scenes: the threshold is a mean luma difference in (0, 255]");
    if (started(s)) return fail(PFNL_ERR_STATE, "scenes are set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    if (mode && !s->scene_first) {
        HIPCHK(hipSetDevice(s->device));
        const size_t words = 2 * (size_t)s->cap + 2;  // scene_first | sad | the sum's scratch (zero between launches)
        bool ok = hipMalloc(reinterpret_cast<void**>(&s->scene_first), words * sizeof(long long)) == hipSuccess;
        // Zeroed on the copy stream and waited for: hipMemset on device memory is queued on the null stream and returns at once, and
        // neither of the session's streams waits for the null stream when the caller's is non-blocking - behind a busy null stream it
        // wiped the first frames' sums after the copy stream had written them.  The copy stream is idle here, so this waits for the fill alone.
        ok = ok && hipMemsetAsync(s->scene_first, 0, words * sizeof(long long), s->cs) == hipSuccess;
        ok = ok && hipStreamSynchronize(s->cs) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&s->scene_ev, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 2; ++i)
            ok = ok && hipHostMalloc(reinterpret_cast<void**>(&s->info[i]), 2 * (size_t)s->cap * sizeof(long long), hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            for (int i = 0; i < 2; ++i) {
                if (s->info[i]) (void)hipHostFree(s->info[i]);
                s->info[i] = nullptr;
            }
            if (s->scene_first) (void)hipFree(s->scene_first);
            if (s->scene_ev) (void)hipEventDestroy(s->scene_ev);
            s->scene_first = nullptr;
            s->scene_ev = nullptr;
            return fail(PFNL_ERR_NOMEM, "scene table allocation failed");
        }
        s->sad = reinterpret_cast<unsigned long long*>(s->scene_first) + s->cap;
    }
    s->scene_mode = mode;
    s->thr_sum = mode == 2 ? (unsigned long long)std::ceil(threshold * s->H * s->W) : 0;
    s->mark = false;
    return 0;
}

// The one check of a candidate against everything a setting must agree with, delivered at out_h x out_w: the route; both packings - a
// packing in force holds its side to the family, depth, chroma format and width it was accepted with, and the answer names the way out -;
// interlacing.  0, or PFNL_ERR_INVALID with the words of the first that refuses.  The stored setting has passed all of it, so a setter is
// refused only for what it changes.
static int candidate_refused(const pfnl_stream* s, const Setting& c, int out_h, int out_w) {
    if (const char* why = pfnl::route_refused(c.in_fmt, c.out_fmt, out_h, out_w, c.out_chroma)) return fail(PFNL_ERR_INVALID, why);
    const char* why = pfnl::pack_refused(c.in_pack, pfnl::is_yuv(c.in_fmt), c.in_depth, c.in_chroma, s->W);
    if (!why) why = pfnl::pack_refused(c.out_pack, pfnl::is_yuv(c.out_fmt), pfnl::is_10bit(c.out_fmt) ? 10 : 8, c.out_chroma, out_w);
    if (why) return fail(PFNL_ERR_INVALID, std::string(why) + " - the change contradicts a packing in force: set PFNL_PACK_NONE first (pfnl_stream_packing)");
    if (const char* no = pfnl::interlace_refused(s->il_mode, s->il_order, s->H, pfnl::is_yuv(c.in_fmt), c.in_chroma, c.in_pack))
        return fail(PFNL_ERR_INVALID, no);
    if (const char* no = pfnl::telecine_refused(s->tc_mode, s->tc_order, s->H, pfnl::is_yuv(c.in_fmt), c.in_chroma, c.in_pack, s->batch))
        return fail(PFNL_ERR_INVALID, no);
    return 0;
}

// The setters: bad arguments first (PFNL_ERR_INVALID at any time) - their own, then the stored setting with their fields changed before
// candidate_refused -, then "before the first frame", then apply_setting.

// The packing of the two edges.  The staging frame and stage 2's slot follow the row bytes, so it goes through apply_setting; each side is
// checked against what is set at the call, in words that name the side, and from then on every setter holds that side to it.
int pfnl_stream_packing(pfnl_stream* s, int in_pack, int out_pack) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    for (int v : {in_pack, out_pack})
        if (v != PFNL_PACK_NONE && !pfnl::is_packing(v)) return fail(PFNL_ERR_INVALID, "packing: PFNL_PACK_NONE .. PFNL_PACK_V210 on either side");
    Setting c = s->set;
    c.in_pack = in_pack;
    c.out_pack = out_pack;
    if (const char* why = pfnl::pack_refused(in_pack, pfnl::is_yuv(c.in_fmt), c.in_depth, c.in_chroma, s->W))
        return fail(PFNL_ERR_INVALID, std::string("input ") + why);
    if (const char* why = pfnl::pack_refused(out_pack, pfnl::is_yuv(c.out_fmt), pfnl::is_10bit(c.out_fmt) ? 10 : 8, c.out_chroma, s->route.out_w))
        return fail(PFNL_ERR_INVALID, std::string("output ") + why);
    if (int e = candidate_refused(s, c, s->route.out_h, s->route.out_w)) return e;
    if (started(s)) return fail(PFNL_ERR_STATE, "the packing is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    return apply_setting(s, c, nullptr, "packing staging allocation failed");
}

int pfnl_stream_format(pfnl_stream* s, int in_fmt, int out_fmt, int matrix, int full_range) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    Setting c = s->set;
    c.in_fmt = in_fmt;
    c.out_fmt = out_fmt;
    if (int e = candidate_refused(s, c, s->route.out_h, s->route.out_w)) return e;
    if (!pfnl::yuv_coefficients(8, matrix, full_range, &c.cin.coef) || !pfnl::yuv_coefficients(10, matrix, full_range, &c.cin.coef10))
        return fail(PFNL_ERR_INVALID, "format: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    c.cout.coef = c.cin.coef;                         // both sides' matrix and range, replacing what pfnl_stream_colour set; the primaries stay
    c.cout.coef10 = c.cin.coef10;
    if (started(s)) return fail(PFNL_ERR_STATE, "the format is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    return apply_setting(s, c, nullptr, "format staging allocation failed");
}

// The colour of each edge: matrix and range are the coefficients of that edge's YUV conversion and replace what pfnl_stream_format set for
// it; where the primaries differ, stage 0 converts (colour.hip) on the device's tables, which the first such setting finds or uploads.  No
// route and no slot depends on it.
int pfnl_stream_colour(pfnl_stream* s, const pfnl_colour* in, const pfnl_colour* out) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    Setting c = s->set;
    const pfnl_colour* const given[2] = {in, out};
    SideColour* const side[2] = {&c.cin, &c.cout};
    for (int k = 0; k < 2; ++k) {
        if (!given[k]) continue;                      // that side keeps what it has
        if (!pfnl::yuv_coefficients(8, given[k]->matrix, given[k]->full_range, &side[k]->coef) ||
            !pfnl::yuv_coefficients(10, given[k]->matrix, given[k]->full_range, &side[k]->coef10) || !pfnl::is_primaries(given[k]->primaries))
            return fail(PFNL_ERR_INVALID, "colour: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1, primaries PFNL_PRIM_BT709, PFNL_PRIM_BT601_525 or PFNL_PRIM_BT601_625");
        side[k]->prim = given[k]->primaries;
    }
    (void)pfnl::colour_matrix(c.cin.prim, c.cout.prim, &c.gamut);
    if (started(s)) return fail(PFNL_ERR_STATE, "the colour is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    if (c.cin.prim != c.cout.prim && !s->ctab[0]) {
        HIPCHK(hipSetDevice(s->device));
        if (pfnl::colour_device_tables(&s->ctab[0], &s->ctab[1]) != hipSuccess) {
            (void)hipGetLastError();
            s->ctab[0] = s->ctab[1] = nullptr;
            return fail(PFNL_ERR_NOMEM, "colour table allocation failed");
        }
    }
    return apply_setting(s, c, nullptr, "colour setting failed");
}

// The depth of the pushed samples: in_fmt keeps naming the layout.  At 10 the ring and the staging frame hold uint16 samples; decode, scene
// sums and both gathers run their uint16 bodies; everything behind the windows is what it was.
int pfnl_stream_input_depth(pfnl_stream* s, int bits) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (bits != 8 && bits != 10) return fail(PFNL_ERR_INVALID, "input depth: 8 or 10 bits");
    Setting c = s->set;
    c.in_depth = bits;
    if (int e = candidate_refused(s, c, s->route.out_h, s->route.out_w)) return e;
    if (started(s)) return fail(PFNL_ERR_STATE, "the input depth is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    return apply_setting(s, c, nullptr, "input ring allocation failed");
}

// The subsampling of the two YUV edges: in_fmt / out_fmt keep naming the layout.  The staging frame and stage 2's slot follow it, so it goes
// through apply_setting like the depth; the output size is checked against it here and by whichever of the size setters comes later.
int pfnl_stream_chroma_format(pfnl_stream* s, int in_chroma, int out_chroma) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!pfnl::is_chroma(in_chroma) || !pfnl::is_chroma(out_chroma))
        return fail(PFNL_ERR_INVALID, "chroma format: PFNL_CHROMA_420, PFNL_CHROMA_422 or PFNL_CHROMA_444 on either side");
    Setting c = s->set;
    c.in_chroma = in_chroma;
    c.out_chroma = out_chroma;
    if (int e = candidate_refused(s, c, s->route.out_h, s->route.out_w)) return e;
    if (started(s)) return fail(PFNL_ERR_STATE, "the chroma format is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    return apply_setting(s, c, nullptr, "chroma format staging allocation failed");
}

// Interlaced input: pushed frames are woven, the ring receives progressive frames (field_geom.h; deinterlace.hip).  The field store is
// allocated by the first call that turns it on, at the input depth (apply_setting makes it follow a later change of depth).
int pfnl_stream_interlace(pfnl_stream* s, int mode, int field_order) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (const char* why = pfnl::interlace_refused(mode, field_order, s->H, pfnl::is_yuv(s->set.in_fmt), s->set.in_chroma, s->set.in_pack))
        return fail(PFNL_ERR_INVALID, why);
    if (mode && s->tc_mode) return fail(PFNL_ERR_INVALID, "interlace: inverse telecine is on (pfnl_stream_telecine): the two are exclusive");
    if (started(s)) return fail(PFNL_ERR_STATE, "interlacing is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    if (mode && !s->fstore) {
        HIPCHK(hipSetDevice(s->device));
        uint8_t* store = nullptr;
        hipEvent_t ev = nullptr;
        bool ok = hipMalloc(reinterpret_cast<void**>(&store), 3 * s->in.ring_bytes) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (store) (void)hipFree(store);
            return fail(PFNL_ERR_NOMEM, "field store allocation failed");
        }
        s->fstore = store;
        s->il_ev = ev;
    }
    s->il_mode = mode;
    s->il_order = field_order;
    return 0;
}

// Inverse telecine: pushed frames are fields of film, the ring receives the film's frames (telecine_geom.h; telecine.hip).  The first call
// that turns it on allocates what it needs beside the field store, all of it or nothing.
int pfnl_stream_telecine(pfnl_stream* s, int mode, int field_order, const pfnl_telecine_params* params) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (const char* why = pfnl::telecine_refused(mode, field_order, s->H, pfnl::is_yuv(s->set.in_fmt), s->set.in_chroma, s->set.in_pack, s->batch))
        return fail(PFNL_ERR_INVALID, why);
    pfnl_telecine_params q;
    if (const char* why = pfnl::telecine_params_refused(params, s->H / 2, s->W, &q)) return fail(PFNL_ERR_INVALID, why);
    if (mode && s->il_mode) return fail(PFNL_ERR_INVALID, "telecine: interlacing is on (pfnl_stream_interlace): the two are exclusive");
    if (started(s)) return fail(PFNL_ERR_STATE, "inverse telecine is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    if (mode && !s->tc_frames) {
        HIPCHK(hipSetDevice(s->device));
        uint8_t *store = nullptr, *cycle = nullptr;
        unsigned long long *words = nullptr, *host = nullptr;
        hipEvent_t ev = nullptr;
        bool ok = s->fstore || hipMalloc(reinterpret_cast<void**>(&store), 3 * s->in.ring_bytes) == hipSuccess;
        ok = ok && (s->il_ev || hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess);
        ok = ok && hipMalloc(reinterpret_cast<void**>(&cycle), pfnl::TC_CYCLE * s->in.ring_bytes) == hipSuccess;
        ok = ok && hipMalloc(reinterpret_cast<void**>(&words), TC_WORDS * sizeof(unsigned long long)) == hipSuccess;
        // (zeroed on the copy stream and waited for, as the scene table is)
        ok = ok && hipMemsetAsync(words, 0, TC_WORDS * sizeof(unsigned long long), s->cs) == hipSuccess && hipStreamSynchronize(s->cs) == hipSuccess;
        ok = ok && hipHostMalloc(reinterpret_cast<void**>(&host), 8 * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (store) (void)hipFree(store);
            if (ev) (void)hipEventDestroy(ev);
            if (cycle) (void)hipFree(cycle);
            if (words) (void)hipFree(words);
            if (host) (void)hipHostFree(host);
            return fail(PFNL_ERR_NOMEM, "telecine store allocation failed");
        }
        if (store) s->fstore = store;
        if (ev) s->il_ev = ev;
        s->tc_frames = cycle;
        s->tc_words = words;
        s->tc_host = host;
    }
    s->tc_mode = mode;
    s->tc_order = field_order;
    s->tc_par = q;
    return 0;
}

int pfnl_stream_telecine_stats(pfnl_stream* s, long long out[5]) {
    if (!s || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    for (int k = 0; k < 5; ++k) out[k] = 0;
    if (!s->tc_words) return 0;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->s));
    HIPCHK(hipMemcpyAsync(s->tc_host + pfnl::TC_CYCLE, s->tc_words + TC_AT_STATS, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->cs));
    HIPCHK(hipStreamSynchronize(s->cs));
    for (int k = 0; k < 3; ++k) out[k] = (long long)s->tc_host[pfnl::TC_CYCLE + k];
    out[3] = s->tc_dropped;
    out[4] = s->tc_admitted;
    return 0;
}

int pfnl_telecine_deliverable(int mode, long long pushed, int ended, long long* frames) {
    if (!frames) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (mode != PFNL_TELECINE_MATCH && mode != PFNL_TELECINE_DECIMATE) return fail(PFNL_ERR_INVALID, "deliverable: mode PFNL_TELECINE_MATCH or PFNL_TELECINE_DECIMATE");
    if (pushed < 0) return fail(PFNL_ERR_INVALID, "deliverable: pushed is not negative");
    *frames = pfnl::telecine_deliverable(mode, pushed, ended != 0);
    return 0;
}

// no memory and no route depend on the sitings: they are arguments of the two conversion launches
int pfnl_stream_chroma_siting(pfnl_stream* s, int in_siting, int out_siting) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    for (int v : {in_siting, out_siting})
        if (v < PFNL_SITING_LEFT || v > PFNL_SITING_TOPLEFT)
            return fail(PFNL_ERR_INVALID, "chroma siting: PFNL_SITING_LEFT, PFNL_SITING_CENTER or PFNL_SITING_TOPLEFT on either side");
    if (started(s)) return fail(PFNL_ERR_STATE, "the chroma siting is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    s->in_siting = in_siting;
    s->out_siting = out_siting;
    return 0;
}

// pfnl_stream_resize is the placement of the whole raster on the whole canvas: one body, and place_plan keeps resize_plan's words for it
int pfnl_stream_place(pfnl_stream* s, int out_H, int out_W, const pfnl_rect* src, const pfnl_rect* dst, const uint8_t fill_rgb[3]) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int sH = s->scale * s->H, sW = s->scale * s->W;
    pfnl::PlacePlan plan;                             // (0, 0 is off: cH = cW = 0, no table, the network's raster - which is even)
    std::string why;
    if (!out_H && !out_W && (src || dst || fill_rgb)) return fail(PFNL_ERR_INVALID, "place: src, dst and a fill colour need a canvas size (0, 0 is off)");
    if ((out_H || out_W) && !pfnl::place_plan(sH, sW, out_H, out_W, src, dst, &plan, &why)) return fail(PFNL_ERR_INVALID, why);
    if (int e = candidate_refused(s, s->set, plan.cH ? plan.cH : sH, plan.cW ? plan.cW : sW)) return e;   // (the setting stays: the size changes)
    if (started(s)) return fail(PFNL_ERR_STATE, "the output size is set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    for (int k = 0; k < 3 && fill_rgb; ++k) plan.fill[k] = fill_rgb[k];
    return apply_setting(s, s->set, &plan, "resize allocation failed");
}

int pfnl_stream_resize(pfnl_stream* s, int out_H, int out_W) { return pfnl_stream_place(s, out_H, out_W, nullptr, nullptr, nullptr); }

int pfnl_stream_mark_cut(pfnl_stream* s) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!s->scene_mode) return fail(PFNL_ERR_STATE, "mark_cut: scenes are off (pfnl_stream_scenes)");
    if (started(s)) s->mark = true;                   // (frame 0 starts scene 0 and is no cut)
    return 0;
}

int pfnl_stream_pop_info(pfnl_stream* s, long long* scene_first, unsigned long long* sad) {
    if (!s || !scene_first || !sad) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!s->has_info) return fail(PFNL_ERR_STATE, "pop_info: no frame of this sequence has been popped");
    *scene_first = s->info_first;
    *sad = s->info_sad;
    return 0;
}

// The content box of every ring frame.  The boxes have the ring's slots; the kernel's scratch words lie behind them and are zero between
// launches, so they are zeroed once, here - on the copy stream and waited for, as the scene table is.
int pfnl_stream_bars(pfnl_stream* s, int mode, int limit) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (mode != 0 && mode != 1) return fail(PFNL_ERR_INVALID, "bars: mode 0 (off) or 1 (every ring frame is measured)");
    if (mode && (limit < 0 || limit > pfnl::BARS_LIMIT_MAX)) return fail(PFNL_ERR_INVALID, "bars: the limit is a mean luma in 0 .. 219");
    if (mode && !pfnl::bars_args_ok(s->H, s->W, limit)) return fail(PFNL_ERR_INVALID, "bars: H and W are at most 16384 (the sums are 32-bit)");
    if (started(s)) return fail(PFNL_ERR_STATE, "bars are set before the first frame of a sequence (pfnl_stream_reset starts the next)");
    if (mode && !s->bars_box) {
        HIPCHK(hipSetDevice(s->device));
        const size_t bytes = (4 * (size_t)s->cap + pfnl::bars_scratch_words(1, s->H, s->W)) * sizeof(int32_t);
        int32_t *box = nullptr, *info[2] = {nullptr, nullptr};
        hipEvent_t ev = nullptr;
        bool ok = hipMalloc(reinterpret_cast<void**>(&box), bytes) == hipSuccess;
        ok = ok && hipMemsetAsync(box, 0, bytes, s->cs) == hipSuccess && hipStreamSynchronize(s->cs) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 2; ++i)
            ok = ok && hipHostMalloc(reinterpret_cast<void**>(&info[i]), 4 * (size_t)s->cap * sizeof(int32_t), hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            for (int32_t* p : info)
                if (p) (void)hipHostFree(p);
            if (ev) (void)hipEventDestroy(ev);
            if (box) (void)hipFree(box);
            return fail(PFNL_ERR_NOMEM, "content box allocation failed");
        }
        s->bars_box = box;
        s->bars_info[0] = info[0];
        s->bars_info[1] = info[1];
        s->bars_ev = ev;
    }
    s->bars_mode = mode;
    s->bars_limit = mode ? limit : 0;
    return 0;
}

int pfnl_stream_pop_box(pfnl_stream* s, int32_t box[4]) {
    if (!s || !box) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!s->bars_mode) return fail(PFNL_ERR_STATE, "pop_box: bars are off (pfnl_stream_bars)");
    if (!s->has_box) return fail(PFNL_ERR_STATE, "pop_box: no frame of this sequence has been popped");
    for (int k = 0; k < 4; ++k) box[k] = s->pop_box[k];
    return 0;
}

int pfnl_stream_content_box(pfnl_stream* s, int32_t box[4], long long* frames) {
    if (!s || !box || !frames) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!s->bars_mode) return fail(PFNL_ERR_STATE, "content_box: bars are off (pfnl_stream_bars)");
    if (!s->has_box) return fail(PFNL_ERR_STATE, "content_box: no frame of this sequence has been popped");
    for (int k = 0; k < 4; ++k) box[k] = s->seq_box[k];
    *frames = s->box_frames;
    return 0;
}

int pfnl_stream_reset(pfnl_stream* s) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(s->device));
    return drop_sequence(s);
}

int pfnl_stream_close(pfnl_stream* s) {
    if (!s) return fail(PFNL_ERR_INVALID, "NULL argument");
    (void)hipSetDevice(s->device);
    const int r = drop_sequence(s);
    *pfnl_internal_view(s->h).session = nullptr;
    release(s);
    return r;
}

}  // extern "C"
