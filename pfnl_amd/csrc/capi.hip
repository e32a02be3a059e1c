// C-ABI of libpfnl_hip.so (see include/pfnl_hip.h): handle, weight repacking, the forward
// schedule of PFNL.forward (reference model/pfnl.py:39-80) as a sequence of HIP kernel launches.
#include <dlfcn.h>

#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pfnl_hip.h"
#include "capi_internal.h"
#include "common.h"
#include "conv_bf16.h"
#include "conv_split16.h"
#include "conv_small.h"
#include "launch_plan.h"
#include "tile_geom.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace

int pfnl_internal_fail(int code, const std::string& msg) { return fail(code, msg); }

namespace {

// bumped whenever a device buffer moves: captured graphs hold raw pointers.  Process-wide (DESIGN.md "What handles share"): every handle's
// DevBuf::ensure bumps it and every handle's graph check reads it, from whatever host thread drives that handle - relaxed is enough, the
// counter orders nothing: a handle only needs to see its OWN bumps, and those it made on its own thread
static std::atomic<unsigned long long> g_alloc_gen{0};

struct DevBuf {
    float* p = nullptr;
    size_t n = 0;   // floats
    int ensure(size_t count) {
        if (count <= n) return 0;
        g_alloc_gen.fetch_add(1, std::memory_order_relaxed);
        if (p) hipFree(p);
        p = nullptr;
        n = 0;
        if (hipMalloc(&p, count * sizeof(float)) != hipSuccess) return -1;
        n = count;
        return 0;
    }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        n = 0;
    }
};

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

// Pinned (page-locked) host memory of the handle: the landing / take-off strip of host-pointer forwards.
struct PinBuf {
    unsigned char* p = nullptr;
    size_t n = 0;   // bytes
    int ensure(size_t bytes) {
        if (bytes <= n) return 0;
        release();
        if (hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            return -1;
        }
        n = bytes;
        return 0;
    }
    void release() {
        if (p) hipHostFree(p);
        p = nullptr;
        n = 0;
    }
};

// A few worker threads that move bytes between a caller's PAGEABLE buffers and the pinned strip while the copy engines move the
// pinned side over PCIe (a host-pointer pfnl_forward is what the reference's sess.run timing covers, model/pfnl.py:249-253).
// One job at a time: run(n, f) hands out chunk indices 0..n-1 in order; done(i) / wait() observe completion.
struct HostPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    std::function<void(int)> fn;
    std::unique_ptr<std::atomic<int>[]> flag;
    int cap = 0, n = 0, next = 0, finished = 0, device = 0;   // (a job is only started after the previous one has been waited for)
    bool stop = false;
    void start(int k, int dev) {
        if (!th.empty()) return;
        device = dev;
        for (int i = 0; i < k; ++i) th.emplace_back([this] { loop(); });
    }
    void loop() {
        hipSetDevice(device);
        for (;;) {
            int i;
            {
                std::unique_lock<std::mutex> lk(m);
                cv_work.wait(lk, [&] { return stop || next < n; });
                if (stop) return;
                i = next++;
            }
            fn(i);
            flag[i].store(1, std::memory_order_release);
            {
                std::lock_guard<std::mutex> lk(m);
                ++finished;
            }
            cv_done.notify_all();
        }
    }
    void run(int count, std::function<void(int)> f) {
        std::lock_guard<std::mutex> lk(m);
        if (count > cap) {
            flag.reset(new std::atomic<int>[count]);
            cap = count;
        }
        for (int i = 0; i < count; ++i) flag[i].store(0, std::memory_order_relaxed);
        fn = std::move(f);
        n = count;
        next = 0;
        finished = 0;
        cv_work.notify_all();
    }
    void wait_chunk(int i) {
        while (!flag[i].load(std::memory_order_acquire)) std::this_thread::yield();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return finished >= n; });
    }
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv_work.notify_all();
        for (auto& t : th) t.join();
        th.clear();
    }
};

}  // namespace

// the weight packs of one PF block: offsets into the three device blobs, filled by pfnl_finalize_weights
struct BlockPacks {
    // fp32 blob `wdev` (floats): the direct kernel's packs, biases, conv1x1_pack_weights (c10_s), the Winograd packs (_u)
    size_t c1_w = 0, c1_b = 0, c10_w = 0, c10_b = 0, c10_s = 0, c2a_w = 0, c2b_w = 0, c2_b = 0;
    size_t c1_u = 0, c2a_u = 0, c2b_u = 0;
    // bf16 blob `wdev16` (16-bit elements): conv3x3_bf16_pack_weights, conv1x1_bf16_pack_weights; _m16: conv3x3_bf16_pack_weights16
    size_t bf_c1 = 0, bf_c10 = 0, bf_c2a = 0, bf_c2b = 0, bf_c1_m16 = 0, bf_c2b_m16 = 0;
    // split-f16 blob `wdev16s` (16-bit elements): the 3x3 / 1x1 split-f16 packs; c10f: conv10_i as conv3x3_c1c10_kernel takes it; _sf: with the
    // identity row map conv3x3_sf_kernel takes (conv_sf.hip); _m16: the order of the v_mfma_f32_16x16x32_f16 chain kernel (conv3x3_split16_pack_weights16)
    size_t s_c1 = 0, s_c2a = 0, s_c2b = 0, s_c10 = 0, s_c10f = 0, s_c2a_sf = 0, s_c2b_sf = 0, s_c2a_m16 = 0, s_c2b_m16 = 0, s_c1_m16 = 0;   // (s_c1_m16: conv1_i for conv3x3_c1c10_kernel's 16x16x32 form - rows permuted)
    // ... and the small-shape packs (conv_small.hip) in the same blob
    size_t sm_c1 = 0, sm_c10 = 0, sm_c2 = 0;
};

struct pfnl_handle {
    pfnl_config cfg;
    int ncu = 0;                                              // CUs of the device (cfg.device_id): the launch plan's thresholds and grid
    hipStream_t stream = nullptr;
    std::map<std::string, std::vector<int64_t>> expected;   // tf name -> shape
    std::map<std::string, HostTensor> host;                  // tensors received so far
    bool finalized = false;
    bool weights_external = false;                           // the device blobs came from another handle (copy / broadcast): `host` holds placeholders
    size_t wdev_used = 0, wdev16_used = 0, wdev16s_used = 0;  // floats of each blob the current weights occupy (DevBuf.n is a grow-only capacity)
    // launch-bound shapes (e.g. BASELINE.json configs[0], 1x7x32x32: ~95 launches of a few us each): the whole
    // forward is captured once per (B, H, W) into a hipGraph between the staging buffers and replayed
    struct GraphEntry {
        int B, H, W, seen;
        hipGraph_t graph;
        hipGraphExec_t exec;
        unsigned long long alloc_gen, cfg_gen;
        unsigned long long seen_cfg_gen;                          // cfg_gen at the eager run that `seen` counts
        int slot;                                                 // range-flag word the captured tail kernel writes (0 synchronous / 1 asynchronous calls)
    };
    std::vector<GraphEntry> graphs;
    unsigned long long cfg_gen = 0;                           // bumped by finalize_weights / set_option
    hipEvent_t gev = nullptr;                                  // ordering with the legacy default stream around a replay
    pfnl::Options opt;                                        // what pfnl_set_option and the environment reads of pfnl_create set (launch_plan.h)
    int merge_cstride = 48;                                   // floats per pixel of `merge` as written by the last forward
    DevBuf wdev16;                                            // bf16 packs (offsets in 16-bit elements)
    size_t off16_m1 = 0;                                      // convmerge1: T consecutive packs (cout 48 zero-padded to 64)
    size_t off16s_m1 = 0;                                     // convmerge1, split-f16 packs: T consecutive (frame, both halves) packs
    DevBuf wdev16s;                                           // split-f16 packs of the 3x3 kernels (offsets in 16-bit elements)
    size_t off16m_m1 = 0;                                     // convmerge1's small-shape pack (conv_small.hip), in the same blob
    // The f16-pipe kernels of the fp32 path have a DOMAIN (operands inside binary16's range; the non-local kernel: inputs x 2^7).
    // Beyond it an operand becomes inf and the result non-finite - the tail kernel, which every output value passes through, ORs
    // that into `rflag` (sticky device word).  Host-pointer calls read it before they return and, when it is set, redo the call on
    // the f32-MFMA kernels (no such domain: the reference's own arithmetic range); device-pointer calls stay asynchronous and
    // pfnl_sync reports PFNL_ERR_RANGE.  Option strict_fp32=on takes the f32-MFMA kernels from the start.
    // Two sticky words in pinned, device-mapped host memory (written by the tail kernel with a system-scope store, read by the host
    // without a copy once the stream is idle): [0] belongs to SYNCHRONOUS (host-pointer) calls, [1] to asynchronous (device-pointer)
    // calls and is what pfnl_sync / pfnl_range_flag report - a host-pointer call never consumes a flag an earlier asynchronous call left.
    unsigned* rflag_host = nullptr;
    unsigned* rflag_dev = nullptr;
    // host-pointer forwards: pinned strips + the threads that copy between them and the caller's pageable buffers
    PinBuf pin_in, pin_out;
    HostPool pool;
    std::vector<hipEvent_t> d2h_ev;
    bool strict_once = false, weights_f16_ok = true;
    long long range_reruns = 0;
    DevBuf p10;                                               // the small-shape trunk's conv10_i partials (small_c10) [B*T][H][W][64] fp32
    DevBuf inp0sf;                                            // the split-format copy of the block output (sf0) [B*T][H][W] x 256 B
    DevBuf c10part;                                           // split chains: conv10_i's partial sums of the parts: [slot][8][32][64] fp32

    // device weights (offsets in floats into `wdev`)
    DevBuf wdev;
    size_t off_conv0_w = 0, off_conv0_b = 0;
    std::vector<BlockPacks> blocks;                           // per PF block, offsets into all three blobs
    std::vector<size_t> off_m1_u;                             // convmerge1 per frame, Winograd pack (cout 48 padded to 64)
    size_t off_m1_w = 0, off_m1_b = 0, off_m2_w = 0, off_m2_b = 0, off_nl_w = 0, off_nl_b = 0, off_zero = 0;

    // embedded-Gaussian option of the non-local block (utils.py nltype 0): optional theta / phi projections
    std::map<std::string, std::vector<int64_t>> optional;    // tf name -> shape (all four or none)
    bool nl_theta = false;
    size_t off_nl_m = 0, off_nl_c = 0;                        // M = Wt Wp^T [CP][CP], c = bt Wp^T [CP]
    DevBuf Q;                                                 // projected queries [B][N][CP]
    DevBuf Xs;                                                // average-pooled keys / values [B][Nk][CP] (nl_sub_sample > 1)

    // workspace
    DevBuf nl16;                                              // bf16 non-local: split K / V^T operands
    DevBuf X, Xo, nlp, inp0, inp1, base, pb, merge, stage_in, stage_out, scratch;
    DevBuf ens_in, ens_y;                                     // pfnl_forward_ensemble: g_k(in) [B][T][H][W][3] and one member's output [B][sH][sW][3]
    DevBuf tile_in, tile_y;                                   // pfnl_forward_tiled: a run's tile stack [run][T][th][tw][3] and its result [run][s th][s tw][3]
    int lastB = 0, lastH = 0, lastW = 0;

    // profiling: boundary events.  One event after every kernel launch (plus one at the start of a
    // forward); a launch's time = its event - the previous event, i.e. kernel + the gap before it.
    bool prof = false;
    int prof_mode = 0;                // 1: every launch; 2: every launch outside the PF blocks + every 4th PF block; 3: the launches of one PF block only
    bool prof_gate = true;            // events are recorded for the launches issued now
    bool chain_open = false;          // an event has been recorded in the current forward
    std::vector<hipEvent_t> evs;
    std::vector<int> ev_cls;          // class of the interval ENDING at event i (-1: chain start)
    std::vector<int> ev_cnt;          // launches inside that interval (1, except in mode 4)
    // mode 4 ("class runs", for launch-bound shapes where an event per launch costs a fifth of the forward): ONE event where the class
    // of consecutive launches changes (and at the end of the forward): ~8 events per forward; the run's launches are counted
    int run_cls = -1, run_n = 0;
    size_t evs_used = 0;
    double prof_ms[PFNL_K_COUNT] = {0};
    int64_t prof_n[PFNL_K_COUNT] = {0};

    pfnl_stream* session = nullptr;   // the one open streaming session (capi_stream.hip): the handle is not re-entrant
};

pfnl_handle_view pfnl_internal_view(pfnl_handle* h) {
    return {h->cfg.num_frames, h->cfg.scale, h->cfg.device_id, h->finalized, h->stream, &h->session};
}

namespace {

using namespace pfnl;

// sampled profiling (mode 2): which PF blocks get events - two of twenty (blocks 3 and 13: an event costs the stream ~2 us and
// the blocks are identical), every 4th below ten blocks.  bench.py scales the in-block classes by num_block / (blocks sampled).
inline bool prof_sampled(int nb, int i) { return nb >= 10 ? (i % 10) == 3 : (i & 3) == 0; }

int prof_mark(pfnl_handle* h, hipStream_t s, int cls, int count = 1) {
    if (h->evs_used == h->evs.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        h->evs.push_back(e);
        h->ev_cls.push_back(-1);
        h->ev_cnt.push_back(1);
    }
    h->ev_cls[h->evs_used] = cls;
    h->ev_cnt[h->evs_used] = count;
    return hipEventRecord(h->evs[h->evs_used++], s) == hipSuccess ? 0 : -1;
}

// mode 4: closes the run of same-class launches that is open (at a class change, and where a forward ends)
void prof_flush_run(pfnl_handle* h, hipStream_t s) {
    if (h->prof && h->prof_mode == 4 && h->run_n > 0) prof_mark(h, s, h->run_cls, h->run_n);
    h->run_n = 0;
    h->run_cls = -1;
}

// roctx ranges around every kernel class (the tracing hook of this path): env PFNL_ROCTX=1 resolves
// roctxRangePushA / roctxRangePop at run time (librocprofiler-sdk-roctx, else libroctx64; never linked) - under
// `rocprofv3 --marker-trace --kernel-trace` the launches of a forward then sit inside named ranges (nl_pack, nl_attn, conv0,
// conv3x3, conv1x1, merge1, tail), per PF block in launch order.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
const Roctx* roctx() {
    static const Roctx r = [] {
        Roctx x;
        const char* e = std::getenv("PFNL_ROCTX");
        if (!e || !*e || *e == '0') return x;
        for (const char* n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4",
                              "/opt/rocm/lib/librocprofiler-sdk-roctx.so", "/opt/rocm/lib/libroctx64.so"}) {
            if (void* lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) {
                x.push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
                x.pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
                if (x.push && x.pop) break;
                x.push = nullptr;
                x.pop = nullptr;
            }
        }
        return x;
    }();
    return &r;
}
const char* const kClassNames[PFNL_K_COUNT] = {"pfnl:nl_pack", "pfnl:nl_attn", "pfnl:conv0", "pfnl:conv3x3", "pfnl:conv1x1", "pfnl:merge1", "pfnl:tail"};

struct ProfScope {
    pfnl_handle* h;
    hipStream_t s;
    int cls;
    bool ranged = false;
    ProfScope(pfnl_handle* h_, hipStream_t s_, int cls_) : h(h_), s(s_), cls(cls_) {
        if (roctx()->push && cls >= 0 && cls < PFNL_K_COUNT) {
            roctx()->push(kClassNames[cls]);
            ranged = true;
        }
        if (h && h->prof && h->prof_mode == 4 && h->run_n > 0 && h->run_cls != cls) prof_flush_run(h, s);
        if (h && h->prof && h->prof_gate && !h->chain_open) {
            prof_mark(h, s, -1);
            h->chain_open = true;
        }
    }
    ~ProfScope() {
        if (h && h->prof && h->prof_mode == 4) {
            h->run_cls = cls;
            ++h->run_n;
        } else if (h && h->prof && h->prof_gate) {
            prof_mark(h, s, cls);
        }
        if (ranged) roctx()->pop();
    }
};

int prof_collect(pfnl_handle* h) {
    for (size_t i = 0; i < h->evs_used; ++i) {
        const int cls = h->ev_cls[i];
        if (cls < 0 || i == 0) continue;
        if (hipEventSynchronize(h->evs[i]) != hipSuccess) return -1;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->evs[i - 1], h->evs[i]) != hipSuccess) return -1;
        h->prof_ms[cls] += ms;
        h->prof_n[cls] += h->ev_cnt[i];
    }
    h->evs_used = 0;
    h->chain_open = false;
    return 0;
}

int check_geometry(const pfnl_config& c) {
    if (c.num_frames != 3 && c.num_frames != 5 && c.num_frames != 7)
        return fail(PFNL_ERR_INVALID, "num_frames must be 3, 5 or 7");
    if (c.scale != 2 && c.scale != 4) return fail(PFNL_ERR_INVALID, "scale must be 2 or 4");
    if (c.mf != 64) return fail(PFNL_ERR_INVALID, "mf must be 64");
    if (c.num_block < 0 || c.num_block > 1024) return fail(PFNL_ERR_INVALID, "bad num_block");
    for (int r : c.reserved)
        if (r != 0) return fail(PFNL_ERR_INVALID, "reserved config fields must be 0");
    return 0;
}

void add_expected(pfnl_handle* h, const std::string& layer, int k, int cin, int cout) {
    h->expected["nlvsr/" + layer + "/kernel"] = {k, k, cin, cout};
    h->expected["nlvsr/" + layer + "/bias"] = {cout};
}

size_t numel(const std::vector<int64_t>& s) {
    size_t n = 1;
    for (auto d : s) n *= (size_t)d;
    return n;
}

// the launch plan of a forward (launch_plan.h) for a shape under the handle's current options and weights
TrunkPlan trunk_plan(const pfnl_handle* h, int B, int H, int W, int Hfull) {
    const PlanFacts facts{h->cfg.num_frames, h->ncu, h->nl_theta, h->strict_once, h->weights_f16_ok};
    return trunk_plan(h->opt, facts, B, H, W, Hfull, nl_f16_fits_one_launch(B, (Hfull / 2) * (W / 2)));
}

// what every stage of one forward reads
struct Fwd {
    pfnl_handle* h;
    const TrunkPlan& pl;
    hipStream_t s;
    int B, T, F, H, W;         // F = B * T frames; H: the rows the trunk buffers hold
    const float* wd;           // the fp32 blob
    const uint16_t* w16;       // the bf16 packs
    const uint16_t* w16s;      // the split-f16 and small-shape packs
};

// the split-chain geometry of a chained launch; `partial`: where its parts leave their sums (null: the launch leaves none)
template <class P>
void set_split_chains(P& q, const TrunkPlan& pl, float* partial) {
    q.n_full = pl.n_full;
    q.split_s = pl.split_s;
    q.split_q = pl.split_q;
    q.partial = pl.split_s ? partial : nullptr;
}

// launch_c10_finalize(_bf16): the parts' raw sums in c10part -> the chains that were cut (the caller sets the output, bias and act)
template <class P>
P split_finalize_params(const Fwd& f) {
    P q{};
    q.H = f.H;
    q.W = f.W;
    q.items = f.F;
    q.add_div = f.T;
    set_split_chains(q, f.pl, f.h->c10part.p);
    return q;
}

// a launch of the direct kernel (conv_mfma.hip) over 64-channel frames, `frames` of them per item (1: per frame, T: over their concat)
ConvParams direct_params(const Fwd& f, const float* in, const float* wpack, const float* bias, float* out, int cout, int frames, int act) {
    ConvParams p{};
    p.in = in;
    p.wpack = wpack;
    p.bias = bias;
    p.out = out;
    p.H = f.H;
    p.W = f.W;
    p.in_cstride = 64;
    p.out_cstride = cout;
    p.cout = cout;
    p.chunks_per_frame = 64 / CONV_CK;
    p.frames_per_item = frames;
    p.nchunks = frames * p.chunks_per_frame;
    p.add_div = 1;
    p.act = act;
    return p;
}

int ensure_workspace(pfnl_handle* h, const TrunkPlan& pl, int B, int H, int W, int N) {
    const int T = h->cfg.num_frames, C = 12 * T, CP = nl_padded_ch(C);
    const size_t P = (size_t)H * W;
    if (h->X.ensure((size_t)B * N * CP) || h->Xo.ensure((size_t)B * N * CP) ||     // (N: the FULL frame - keys are global)
        h->nlp.ensure(nl_partial_floats(B, N, C)) ||
        h->inp0.ensure((size_t)B * T * P * 64) || h->inp1.ensure((size_t)B * T * P * 64) ||
        h->base.ensure((size_t)B * P * 64) || h->pb.ensure((size_t)B * P * 64) ||
        h->merge.ensure((size_t)B * P * 64))
        return fail(PFNL_ERR_NOMEM, "workspace allocation failed");
    h->lastB = B;
    h->lastH = H;
    h->lastW = W;
    if (h->p10.ensure(h->cfg.num_block > 0 ? pl.p10_floats : 0) || h->inp0sf.ensure(pl.inp0sf_floats) || h->c10part.ensure(pl.c10part_floats))
        return fail(PFNL_ERR_NOMEM, "workspace allocation failed");
    return 0;
}

// model/pfnl.py:55-60 (+ utils.py:18-71): x -> Xo; queries [q0, q1) against all keys
int nonlocal_block(const Fwd& f, const float* in, int Hfull, int q0, int q1) {
    pfnl_handle* const h = f.h;
    const TrunkPlan& pl = f.pl;
    const int B = f.B, T = f.T, W = f.W, N = (Hfull / 2) * (W / 2), C = 12 * T, CP = nl_padded_ch(C), nlt = pl.nltype;
    const float* const wd = f.wd;
    const hipStream_t s = f.s;
    if ((pl.nl_family == 1 || pl.nl_family == 2) && h->nl16.ensure((nl_f16_scratch_halfs(B, N) + 1) / 2))
        return fail(PFNL_ERR_NOMEM, "workspace allocation failed");
    {
        ProfScope ps(h, s, PFNL_K_NL_PACK);
        if (pl.nl_fused_pack) HIPCHK(launch_nl_pack_fused(in, h->X.p, reinterpret_cast<uint16_t*>(h->nl16.p), B, T, Hfull, W, s));
        else HIPCHK(launch_nl_pack(in, h->X.p, B, T, Hfull, W, s));
    }
    ProfScope ps(h, s, PFNL_K_NL_ATTN);
    if ((nlt == 0 || nlt == 2) && !h->nl_theta)
        return fail(PFNL_ERR_STATE, "nl_type 0 / 2 need the nlblock_0 theta / phi variables (reference utils.py:31-42)");
    if (pl.nl_family == 0) {
        // the general form of utils.NonLocalBlock (nltype 0 / 2: queries X M + c; sub_sample: keys = values = avg-pooled X) on
        // the f32-MFMA kernel in both precisions; PFNL's own call (nltype 1, sub_sample 1) takes the branches below
        const float* Kx = h->X.p;
        int Nk = N;
        if (h->opt.nl_sub > 1) {
            const int h2 = Hfull / 2, w2 = W / 2;
            if (h2 / h->opt.nl_sub < 1 || w2 / h->opt.nl_sub < 1) return fail(PFNL_ERR_INVALID, "nl_sub_sample larger than the space_to_depth grid");
            Nk = (h2 / h->opt.nl_sub) * (w2 / h->opt.nl_sub);
            if (h->Xs.ensure((size_t)B * Nk * CP)) return fail(PFNL_ERR_NOMEM, "workspace allocation failed");
            HIPCHK(launch_nl_pool(h->X.p, h->Xs.p, B, h2, w2, h->opt.nl_sub, C, s));
            Kx = h->Xs.p;
        }
        const float* Qp = nullptr;
        if (nlt != 1) {
            if (h->Q.ensure((size_t)B * N * CP)) return fail(PFNL_ERR_NOMEM, "workspace allocation failed");
            HIPCHK(launch_nl_qproj(h->X.p, wd + h->off_nl_m, wd + h->off_nl_c, h->Q.p, B, N, C, s, nlt == 2));
            Qp = h->Q.p;
        }
        HIPCHK(launch_nl_attn_general(h->X.p, Kx, Nk, h->Xo.p, wd + h->off_nl_w, wd + h->off_nl_b, h->nlp.p, B, N, C, s, Qp, q0, q1, nlt == 2));
    } else if (pl.nl_family == 1 || pl.nl_family == 2) {
        // the f16 pipe: fp32 precision with exactly split operands (1), 16-bit operands throughout - the hi parts only (2)
        HIPCHK(launch_nl_attn_f16(h->X.p, h->Xo.p, wd + h->off_nl_w, wd + h->off_nl_b, h->nlp.p, reinterpret_cast<uint16_t*>(h->nl16.p), B, N, C, s,
                                  q0, q1, pl.nl_family == 1, pl.nl_fused_pack));
    } else {
        HIPCHK(launch_nl_attn(h->X.p, h->Xo.p, wd + h->off_nl_w, wd + h->off_nl_b, h->nlp.p, B, N, C, s, nullptr, q0, q1));
    }
    return 0;
}

// ---- the PF blocks (model/pfnl.py:65-71), one function per trunk family

// bf16 trunk (conv_bf16.hip): activations bf16 in the same workspace buffers, fp32 accumulation and biases.  MID shapes (bmid): the chained
// launches - conv1_i + conv10_i, the per-frame half of conv2_i - would leave most CUs idle for T tile times; conv10_i then runs as its own
// launch and the per-frame half deals out single tiles (bit-identical: this kernel has one summation order)
int block_bf16(const Fwd& f, const BlockPacks& k) {
    pfnl_handle* const h = f.h;
    const TrunkPlan& pl = f.pl;
    const hipStream_t s = f.s;
    const float* const wd = f.wd;
    uint16_t* const a0 = reinterpret_cast<uint16_t*>(h->inp0.p);
    uint16_t* const a1 = reinterpret_cast<uint16_t*>(h->inp1.p);
    uint16_t* const ab = reinterpret_cast<uint16_t*>(h->base.p);
    uint16_t* const ap = reinterpret_cast<uint16_t*>(h->pb.p);
    {   // conv1_i (+ conv10_i from the LDS scratch its tiles pass through: conv_bf16.hip MODE 2)
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        ConvBf16Params q{a0, f.w16 + k.bf_c1, wd + k.c1_b, nullptr, nullptr, a1, f.H, f.W, f.F, 1, 1};
        if (pl.fuse10) {
            q.add_div = f.T;
            q.x_w = f.w16 + k.bf_c10;
            q.x_bias = wd + k.c10_b;
            q.x_out = ab;
            set_split_chains(q, pl, h->c10part.p);
        }
        if (pl.mfma == 16) q.wpack16 = f.w16 + k.bf_c1_m16;   // (used where the launch goes to the third-generation kernel)
        HIPCHK(launch_conv3x3_bf16(q, s));
    }
    if (pl.fuse10 && pl.split_s) {   // split chains: the parts' raw conv10_i sums -> base (+ bias, leaky-relu, bf16) for the chains that were cut
        ProfScope ps(h, s, PFNL_K_CONV1X1);
        ConvBf16Params q = split_finalize_params<ConvBf16Params>(f);
        q.x_bias = wd + k.c10_b;
        q.x_out = ab;
        HIPCHK(launch_c10_finalize_bf16(q, s));
    }
    if (!pl.fuse10) {   // conv10_i as a launch of its own
        ProfScope ps(h, s, PFNL_K_CONV1X1);
        HIPCHK(launch_conv1x1_bf16(a1, f.w16 + k.bf_c10, wd + k.c10_b, ab, f.B, f.T, f.H * f.W, 1, s));
    }
    {   // conv2_i, shared half (raw, once per clip)
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        ConvBf16Params q{ab, f.w16 + k.bf_c2a, wd + h->off_zero, nullptr, nullptr, ap, f.H, f.W, f.B, 1, 0};
        HIPCHK(launch_conv3x3_bf16(q, s));
    }
    {   // conv2_i, per-frame half + shared half + bias, lrelu, residual
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        ConvBf16Params q{a1, f.w16 + k.bf_c2b, wd + k.c2_b, ap, a0, a0, f.H, f.W, f.F, f.T, 1};
        q.flat = pl.bmid ? 1 : 0;
        set_split_chains(q, pl, nullptr);
        if (pl.mfma == 16) q.wpack16 = f.w16 + k.bf_c2b_m16;
        HIPCHK(launch_conv3x3_bf16(q, s));
    }
    return 0;
}

// small shapes (BASELINE.json configs[0], configs[4]): the trunk through conv_small.hip - conv2_i as the reference writes it (3x3 over
// concat([base, f])).  small_c10: two launches per block, conv10_i rides in the conv1_i launch as per-frame partials (W10_t^T . inp1_t), which
// conv2_i's prologue adds up (+ bias, leaky-relu) into its `base` source - no 1x1 launch, no inter-workgroup traffic inside a launch
int block_small(const Fwd& f, const BlockPacks& k) {
    pfnl_handle* const h = f.h;
    const hipStream_t s = f.s;
    const float* const wd = f.wd;
    const int H = f.H, W = f.W, F = f.F, T = f.T;
    {   // conv1_i (:66) (+ this frame's part of conv10_i, :67-68)
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        ConvSmallParams q{nullptr, h->inp0.p, 0, 1, 1, 1, f.w16s + k.sm_c1, wd + k.c1_b, nullptr, h->inp1.p, H, W, F, 1, 3};
        if (f.pl.small_c10) {
            q.x_wpack = f.w16s + k.sm_c10;
            q.x_out = h->p10.p;
            q.x_T = T;
        }
        HIPCHK(launch_conv_small(q, s));
    }
    if (!f.pl.small_c10) {   // conv10_i (:67-68)
        ProfScope ps(h, s, PFNL_K_CONV1X1);
        ConvSmallParams q{nullptr, h->inp1.p, 0, 1, T, T, f.w16s + k.sm_c10, wd + k.c10_b, nullptr, h->base.p, H, W, f.B, 1, 1};
        HIPCHK(launch_conv_small(q, s));
    }
    {   // conv2_i over concat([base, inp1_t]) + lrelu + residual (:69-71); small_c10: base = lrelu(sum of the T partials + bias)
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        ConvSmallParams q{f.pl.small_c10 ? h->p10.p : h->base.p, h->inp1.p, 1, T, 1, 2, f.w16s + k.sm_c2, wd + k.c2_b, h->inp0.p, h->inp0.p, H, W, F, 1, 3};
        if (f.pl.small_c10) {
            q.a_nsum = T;
            q.a_bias = wd + k.c10_b;
        }
        HIPCHK(launch_conv_small(q, s));
    }
    return 0;
}

// the fp32 trunk (every structure but small): inp0 -> inp1 (conv1_i), base (conv10_i), inp0 += conv2_i; `last`: the forward's last block
int block_fp32(const Fwd& f, const BlockPacks& k, bool first, bool last) {
    pfnl_handle* const h = f.h;
    const TrunkPlan& pl = f.pl;
    const hipStream_t s = f.s;
    const float* const wd = f.wd;
    const int H = f.H, W = f.W, F = f.F, T = f.T, B = f.B, algo = pl.algo;
    const bool sf = pl.sf;                                          // inp1 and base in the split format (conv_split16.h)
    // chain2_sf0 (round 6): blocks 1 .. nb-1 read the split-format copy of inp0 the previous block's chain kernel wrote (halo by
    // LDS-DMA); block 0 reads conv0's fp32 output, the last block writes no copy (convmerge1 reads fp32).  Bit-identical to chain2.
    const bool in_sf0 = pl.sf0 && !first, out_sf0 = pl.sf0 && !last;
    if (pl.c10_fused) {
        // conv1_i AND conv10_i in one launch (conv_split16.hip, conv3x3_c1c10_kernel): per (clip, tile) the T frame tiles of conv1_i
        // leave as split-format lines through LDS, where conv10_i picks them up as MFMA operands; inp1 is written, never read back
        {
            ProfScope ps(h, s, PFNL_K_CONV3X3);
            ConvSplitParams q{in_sf0 ? h->inp0sf.p : h->inp0.p, f.w16s + k.s_c1, wd + k.c1_b, nullptr, nullptr, h->inp1.p, H, W, F, T, 1};
            q.in_sf = in_sf0 ? 1 : 0;
            q.wpack2 = f.w16s + k.s_c10f;
            q.bias2 = wd + k.c10_b;
            q.out2 = h->base.p;
            set_split_chains(q, pl, h->c10part.p);
            if (pl.c1_mfma == 16) q.wpack_m16 = f.w16s + k.s_c1_m16;  // (trunk_plan: whole rounds with a chain per CU, fp32 input)
            HIPCHK(launch_conv3x3_c1c10(q, s));
        }
        if (pl.split_s) {   // split chains: the parts' raw conv10_i sums -> base (+ leaky-relu, split format) for the chains that were cut
            ProfScope ps(h, s, PFNL_K_CONV1X1);
            ConvSplitParams q = split_finalize_params<ConvSplitParams>(f);
            q.act = 1;
            q.out2 = h->base.p;
            HIPCHK(launch_c10_finalize(q, s));
        }
    } else {
        {   // conv1_i: per frame 3x3 64->64 + lrelu                       (:66)
            ProfScope ps(h, s, PFNL_K_CONV3X3);
            if (algo == 4) {
                ConvSplitParams q{h->inp0.p, f.w16s + k.s_c1, wd + k.c1_b, nullptr, nullptr, h->inp1.p, H, W, F, 1, 1};
                q.out_sf = sf ? 1 : 0;                              // inp1 in the split format: it only feeds conv10_i and conv2_i's MFMA operands
                HIPCHK(launch_conv3x3_split16(q, s));
            } else if (algo == 1 || algo == 3) {
                WinoParams wp{h->inp0.p, wd + k.c1_u, wd + k.c1_b, nullptr, nullptr, h->inp1.p, H, W, 1, 1, F};
                HIPCHK(algo == 3 ? launch_conv_wino_ws(wp, s) : launch_conv_wino(wp, s));
            } else {
                HIPCHK(launch_conv_mfma(direct_params(f, h->inp0.p, wd + k.c1_w, wd + k.c1_b, h->inp1.p, 64, 1, 1), 3, F, s));
            }
        }
        {   // conv10_i: 1x1 over the concat of T frames -> base + lrelu    (:67-68)
            ProfScope ps(h, s, PFNL_K_CONV1X1);
            if (pl.conv1x1_algo == 2)
                HIPCHK(launch_conv1x1_split16(h->inp1.p, f.w16s + k.s_c10, wd + k.c10_b, h->base.p, B, T, H * W, 1, s, sf, sf));
            else if (pl.conv1x1_algo == 1)
                HIPCHK(launch_conv1x1_stream(h->inp1.p, wd + k.c10_s, wd + k.c10_b, h->base.p, B, T, H * W, 1, s));
            else
                HIPCHK(launch_conv_mfma(direct_params(f, h->inp1.p, wd + k.c10_w, wd + k.c10_b, h->base.p, 64, T, 1), 1, B, s));
        }
    }
    if (pl.conv2_grouped) {
        // the whole of conv2_i in one launch: per (clip, tile) the shared half stays in LDS (conv_wino_ws MODE 2)
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        WinoParams wp{h->inp1.p, wd + k.c2b_u, wd + k.c2_b, nullptr, h->inp0.p, h->inp0.p, H, W, T, 1, F};
        wp.in2 = h->base.p;
        wp.upack2 = wd + k.c2a_u;
        HIPCHK(launch_conv_wino_ws(wp, s));
        return 0;
    }
    if (pl.chain) {
        // the whole of conv2_i in one launch (conv_sf.hip, conv3x3_sf_chain_kernel): per (clip, tile) the shared half stays in
        // registers as the initial C of the T frame tiles; in place on inp0 (residual)
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        ConvSplitParams q{h->inp1.p, f.w16s + k.s_c2b_sf, wd + k.c2_b, nullptr, h->inp0.p, h->inp0.p, H, W, F, T, 1};
        q.in2 = h->base.p;
        q.wpack2 = f.w16s + k.s_c2a_sf;
        q.out2 = out_sf0 ? h->inp0sf.p : nullptr;
        set_split_chains(q, pl, nullptr);
        if (pl.mfma == 16) {                                        // (trunk_plan: whole rounds with a chain per CU)
            q.wpack_m16 = f.w16s + k.s_c2b_m16;
            q.wpack2_m16 = f.w16s + k.s_c2a_m16;
        }
        HIPCHK(launch_conv3x3_sf_chain(q, s));
        return 0;
    }
    {   // conv2_i, shared half: 3x3 over `base` (kernel rows 0..63), once per clip, raw
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        if (algo == 4) {
            ConvSplitParams q{h->base.p, f.w16s + (sf ? k.s_c2a_sf : k.s_c2a), wd + h->off_zero, nullptr, nullptr, h->pb.p, H, W, B, 1, 0};
            HIPCHK(sf ? launch_conv3x3_sf(q, s) : launch_conv3x3_split16(q, s));
        } else if (algo == 1 || algo == 3) {
            WinoParams wp{h->base.p, wd + k.c2a_u, wd + h->off_zero, nullptr, nullptr, h->pb.p, H, W, 1, 0, B};
            HIPCHK(algo == 3 ? launch_conv_wino_ws(wp, s) : launch_conv_wino(wp, s));
        } else {
            HIPCHK(launch_conv_mfma(direct_params(f, h->base.p, wd + k.c2a_w, wd + h->off_zero, h->pb.p, 64, 1, 0), 3, B, s));
        }
    }
    {   // conv2_i, per-frame half (kernel rows 64..127) + shared half + bias, lrelu, residual (:69-71)
        // MID shapes (mid): the block deals out single tiles here - a launch with fewer (clip, tile) chains than CUs would leave most of the chip
        // idle for T + 2 tile times (1 clip of 128x128: 64 chains - 3.06 ms for a quarter of configs[1]'s work)
        ProfScope ps(h, s, PFNL_K_CONV3X3);
        if (algo == 4) {
            ConvSplitParams q{h->inp1.p, f.w16s + (sf ? k.s_c2b_sf : k.s_c2b), wd + k.c2_b, h->pb.p, h->inp0.p, h->inp0.p, H, W, F, T, 1};
            q.flat = pl.mid ? 1 : 0;
            HIPCHK(sf ? launch_conv3x3_sf(q, s) : launch_conv3x3_split16(q, s));
        } else if (algo == 1 || algo == 3) {
            WinoParams wp{h->inp1.p, wd + k.c2b_u, wd + k.c2_b, h->pb.p, h->inp0.p, h->inp0.p, H, W, T, 1, F};
            HIPCHK(algo == 3 ? launch_conv_wino_ws(wp, s) : launch_conv_wino(wp, s));
        } else {
            ConvParams p = direct_params(f, h->inp1.p, wd + k.c2b_w, wd + k.c2_b, h->inp0.p, 64, 1, 1);
            p.addend = h->pb.p;
            p.add_div = T;
            p.resid = h->inp0.p;
            HIPCHK(launch_conv_mfma(p, 3, F, s));
        }
    }
    return 0;
}

// convmerge1 (model/pfnl.py:73-74): the trunk [B*T][H][W] -> merge [B][H][W][merge_stride], lrelu
int convmerge1(const Fwd& f) {
    pfnl_handle* const h = f.h;
    const TrunkPlan& pl = f.pl;
    const hipStream_t s = f.s;
    const float* const wd = f.wd;
    const int H = f.H, W = f.W, F = f.F, T = f.T;
    h->merge_cstride = pl.merge_stride;
    if (pl.merge1 == M1_SPLIT16 || pl.merge1 == M1_SPLIT16_CUT) {
        // on the f16 pipe: the accumulating mode of conv3x3_split16_kernel (the T frame tiles of a clip run through the same accumulators, every
        // unit with its own weights; cout zero-padded to 64; one epilogue per clip tile).  Cut: convmerge1's chains are the trunk's - the same
        // last, partial round is cut by frames, the parts' raw sums meet in c10_finalize_kernel (+ bias, leaky-relu); c10part is free behind the last block
        {
            ProfScope ps(h, s, PFNL_K_MERGE1);
            ConvSplitParams q{h->inp0.p, f.w16s + h->off16s_m1, wd + h->off_m1_b, nullptr, nullptr, h->merge.p, H, W, F, T, 1, 1};
            set_split_chains(q, pl, h->c10part.p);
            HIPCHK(launch_conv3x3_split16(q, s));
        }
        if (pl.merge1 == M1_SPLIT16_CUT) {
            ProfScope ps(h, s, PFNL_K_MERGE1);
            ConvSplitParams q = split_finalize_params<ConvSplitParams>(f);
            q.act = 1;
            q.bias = wd + h->off_m1_b;
            q.out = h->merge.p;
            HIPCHK(launch_c10_finalize(q, s));
        }
        return 0;
    }
    ProfScope ps(h, s, PFNL_K_MERGE1);
    switch (pl.merge1) {
    case M1_SMALL: {   // T sources, cout 48 zero-padded to 64
        ConvSmallParams q{nullptr, h->inp0.p, 0, 1, T, T, f.w16s + h->off16m_m1, wd + h->off_m1_b, nullptr, h->merge.p, H, W, f.B, 1, 3};
        HIPCHK(launch_conv_small(q, s));
        return 0;
    }
    case M1_BF16: {    // the accumulating mode of the bf16 3x3 kernel, fp32 out for the tail
        ConvBf16Params q{reinterpret_cast<const uint16_t*>(h->inp0.p), f.w16 + h->off16_m1, wd + h->off_m1_b, nullptr, nullptr, nullptr, H, W, F, T, 1};
        q.out_f32 = h->merge.p;
        HIPCHK(launch_conv3x3_bf16(q, s));
        return 0;
    }
    case M1_WINOGRAD: {
        // one launch of the persistent Winograd kernel in its accumulating mode (cout zero-padded to 64; the T frame tiles of a clip add into
        // the same accumulators, one epilogue per clip tile)
        WinoParams wp{h->inp0.p, wd + h->off_m1_u[0], wd + h->off_m1_b, nullptr, nullptr, h->merge.p, H, W, T, 1, F};
        wp.upack_stride = T > 1 ? (long long)(h->off_m1_u[1] - h->off_m1_u[0]) : 0;
        wp.accum = 1;
        HIPCHK(launch_conv_wino_ws(wp, s));
        return 0;
    }
    default:           // 3x3 over the concat of T frames -> 48
        HIPCHK(launch_conv_mfma(direct_params(f, h->inp0.p, wd + h->off_m1_w, wd + h->off_m1_b, h->merge.p, 48, T, 1), 3, f.B, s));
        return 0;
    }
}

// forward over device buffers on `s`; flag_slot: the range-flag word its tail kernel writes (0: synchronous call, 1: asynchronous)
// `strip` != null: only LR rows [strip->yoff + core0, strip->yoff + core1) of the result are produced (single-clip sharding,
// pfnl_forward_strip): the non-local block runs its queries [strip->q0, strip->q1) against ALL keys, the trunk runs on the strip + halo.
int forward_device(pfnl_handle* h, const float* in, float* out, int B, int Hfull, int W, hipStream_t s, int flag_slot,
                   const StripGeom* strip = nullptr) {
    const pfnl_config& c = h->cfg;
    const int T = c.num_frames;
    const int H = strip ? strip->Hs : Hfull;                       // rows the trunk buffers hold
    const TrunkPlan pl = trunk_plan(h, B, H, W, Hfull);
    if (pl.bf16 && (long long)T * H * W * 128 >= 0x7fffffffLL) return fail(PFNL_ERR_INVALID, "frame too large for the bf16 trunk");
    if (int e = ensure_workspace(h, pl, B, H, W, (Hfull / 2) * (W / 2))) return e;
    const Fwd f{h, pl, s, B, T, B * T, H, W, h->wdev.p, reinterpret_cast<const uint16_t*>(h->wdev16.p), reinterpret_cast<const uint16_t*>(h->wdev16s.p)};
    const float* const wd = h->wdev.p;

    if (int e = nonlocal_block(f, in, Hfull, strip ? strip->q0 : 0, strip ? strip->q1 : -1)) return e;
    {   // model/pfnl.py:61-62
        ProfScope ps(h, s, PFNL_K_CONV0);
        if (pl.bf16)
            HIPCHK(launch_conv0_bf16(h->Xo.p, wd + h->off_conv0_w, wd + h->off_conv0_b, reinterpret_cast<uint16_t*>(h->inp0.p), B, T, Hfull, W, s, strip));
        else
            HIPCHK(launch_conv0(h->Xo.p, wd + h->off_conv0_w, wd + h->off_conv0_b, h->inp0.p, B, T, Hfull, W, s, strip, pl.strict));
    }
    for (int i = 0; i < c.num_block; ++i) {   // model/pfnl.py:65-71
        if (h->prof_mode == 2) {          // sampled profiling: see prof_sampled; each sampled block with a fresh event chain
            h->prof_gate = prof_sampled(c.num_block, i);
            h->chain_open = false;
        } else if (h->prof_mode == 3) {   // the dominant class only: the launches of ONE block (3 events per forward)
            h->prof_gate = i == c.num_block / 2;
            h->chain_open = false;
        }
        const BlockPacks& k = h->blocks[i];
        const int e = pl.bf16 ? block_bf16(f, k) : pl.small ? block_small(f, k) : block_fp32(f, k, i == 0, i + 1 == c.num_block);
        if (e) return e;
    }
    h->prof_gate = h->prof_mode != 3;
    if (h->prof_mode == 2 || h->prof_mode == 3) h->chain_open = false;
    if (int e = convmerge1(f)) return e;
    {   // model/pfnl.py:63,76-80
        // The range fence is armed only when a kernel with a binary16 DOMAIN runs (fp32 precision off the strict path: split-f16 trunk,
        // non-local block and conv0; bf16 precision: its non-local block and conv0) and a non-finite value cannot be the reference's
        // own result (nltype 2 divides 0 by 0 for a query without a positive affinity, utils.py:59-62).
        unsigned* const rflag = (pl.strict || pl.nltype == 2) ? nullptr : h->rflag_dev + flag_slot;
        ProfScope ps(h, s, PFNL_K_TAIL);
        HIPCHK(launch_tail(h->merge.p, in, wd + h->off_m2_w, wd + h->off_m2_b, out, B, T, Hfull, W, c.scale, pl.merge_stride, s, strip, rflag));
    }
    prof_flush_run(h, s);
    h->chain_open = false;
    return 0;
}

}  // namespace

void pfnl_nl_fold_gw(const float* wg, const float* bg, const float* ww, const float* bw, int C, int CP, float* Wf, float* bf) {
    for (int ci = 0; ci < C; ++ci)
        for (int co = 0; co < C; ++co) {
            double acc = 0.0;
            for (int cm = 0; cm < C; ++cm) acc += (double)wg[(size_t)ci * C + cm] * (double)ww[(size_t)cm * C + co];
            Wf[(size_t)ci * CP + co] = (float)acc;
        }
    for (int co = 0; co < C; ++co) {
        double acc = bw[co];
        for (int cm = 0; cm < C; ++cm) acc += (double)bg[cm] * (double)ww[(size_t)cm * C + co];
        bf[co] = (float)acc;
    }
}

void pfnl_nl_fold_theta_phi(const float* wt, const float* bt, const float* wp, const float* bp, int C, int CP, float* Mf, float* cf) {
    for (int ci = 0; ci < C; ++ci)
        for (int cj = 0; cj < C; ++cj) {
            double acc = 0.0;
            for (int cm = 0; cm < C; ++cm) acc += (double)wt[(size_t)ci * C + cm] * (double)wp[(size_t)cj * C + cm];
            Mf[(size_t)ci * CP + cj] = (float)acc;
        }
    for (int cj = 0; cj < C; ++cj) {
        double acc = 0.0;
        for (int cm = 0; cm < C; ++cm) acc += (double)bt[cm] * (double)wp[(size_t)cj * C + cm];
        cf[cj] = (float)acc;
    }
    if (!bp) return;
    double d0 = 0.0;
    for (int cm = 0; cm < C; ++cm) d0 += (double)bt[cm] * (double)bp[cm];
    cf[C] = (float)d0;
    for (int ci = 0; ci < C; ++ci) {
        double acc = 0.0;
        for (int cm = 0; cm < C; ++cm) acc += (double)wt[(size_t)ci * C + cm] * (double)bp[cm];
        Mf[(size_t)ci * CP + C] = (float)acc;
    }
}

extern "C" {

const char* pfnl_last_error(void) { return g_err.c_str(); }
int pfnl_version(void) { return 4; }

int pfnl_device_count(int* count) {
    if (!count) return fail(PFNL_ERR_INVALID, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return 0;
}

int pfnl_create(const pfnl_config* cfg, pfnl_handle** out) {
    if (!cfg || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (int e = check_geometry(*cfg)) return e;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(PFNL_ERR_NODEVICE, "no HIP device visible: libpfnl_hip has no CPU fallback");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(PFNL_ERR_INVALID, "bad device_id");
    HIPCHK(hipSetDevice(cfg->device_id));
    pfnl_handle* h = new pfnl_handle();
    h->cfg = *cfg;
    h->ncu = pfnl::device_cu_count();
    if (const char* e = std::getenv("PFNL_SF_MID_CHAINS")) h->opt.sf_mid_chains = std::atoi(e);   // (threshold sweeps)
    if (const char* e = std::getenv("PFNL_CONV3X3")) {
        const std::string v(e);
        h->opt.conv_algo = v == "direct" ? 0 : (v == "winograd_tile" ? 1 : (v == "split16" ? 4 : (v == "winograd" ? 3 : 5)));
    }
    // A BLOCKING stream: it is implicitly ordered with the legacy null stream (= torch's default stream) in both
    // directions, so host-pointer calls and graph replays on it are ordered with the caller's default-stream work.
    if (hipStreamCreateWithFlags(&h->stream, hipStreamDefault) != hipSuccess) {
        delete h;
        return fail(PFNL_ERR_HIP, "hipStreamCreate failed");
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&h->rflag_host), 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->rflag_dev), h->rflag_host, 0) != hipSuccess) {
        if (h->rflag_host) hipHostFree(h->rflag_host);
        hipStreamDestroy(h->stream);
        delete h;
        return fail(PFNL_ERR_NOMEM, "allocation failed");
    }
    std::memset(h->rflag_host, 0, 64);
    if (const char* e = std::getenv("PFNL_STRICT_FP32")) h->opt.strict = std::string(e) != "0" && std::string(e) != "off";
    const int T = cfg->num_frames, C = 12 * T;
    add_expected(h, "conv0", 5, 3, 64);
    for (int i = 0; i < cfg->num_block; ++i) {
        add_expected(h, "conv1_" + std::to_string(i), 3, 64, 64);
        add_expected(h, "conv10_" + std::to_string(i), 1, 64 * T, 64);
        add_expected(h, "conv2_" + std::to_string(i), 3, 128, 64);
    }
    add_expected(h, "convmerge1", 3, 64 * T, 48);
    add_expected(h, "convmerge2", 3, 12, cfg->scale == 4 ? 12 : 3);
    add_expected(h, "nlblock_0/g/g", 1, C, C);
    add_expected(h, "nlblock_0/w/w", 1, C, C);
    // utils.py:31-42: nltype 0 / 2 create theta and phi 1x1 convs; PFNL calls the block with nltype 1, where they hold
    // no variables - accepted when a caller supplies all four (embedded Gaussian), absent otherwise
    for (const char* n : {"theta/theta", "phi/phi"}) {
        h->optional[std::string("nlvsr/nlblock_0/") + n + "/kernel"] = {1, 1, C, C};
        h->optional[std::string("nlvsr/nlblock_0/") + n + "/bias"] = {C};
    }
    *out = h;
    return 0;
}

int pfnl_destroy(pfnl_handle* h) {
    if (!h) return 0;
    if (h->session) pfnl_stream_close(h->session);               // (its buffers and events; the options die with the handle)
    hipSetDevice(h->cfg.device_id);
    if (h->stream) {
        hipStreamSynchronize(h->stream);
        hipStreamDestroy(h->stream);
    }
    for (auto& e : h->evs) hipEventDestroy(e);
    if (h->gev) hipEventDestroy(h->gev);
    for (auto& g : h->graphs) {
        if (g.exec) hipGraphExecDestroy(g.exec);
        if (g.graph) hipGraphDestroy(g.graph);
    }
    h->pool.shutdown();
    for (auto& e : h->d2h_ev) hipEventDestroy(e);
    h->pin_in.release();
    h->pin_out.release();
    if (h->rflag_host) hipHostFree(h->rflag_host);
    for (DevBuf* b : {&h->p10, &h->Xs, &h->Q, &h->wdev16s, &h->wdev, &h->wdev16, &h->nl16, &h->X, &h->Xo, &h->nlp, &h->inp0, &h->inp0sf, &h->c10part, &h->inp1, &h->base, &h->pb, &h->merge,
                      &h->stage_in, &h->stage_out, &h->scratch, &h->ens_in, &h->ens_y, &h->tile_in, &h->tile_y})
        b->release();
    delete h;
    return 0;
}

int pfnl_set_weight(pfnl_handle* h, const char* tf_name, const float* host, const int64_t* shape,
                    int rank) {
    if (!h || !tf_name || !host || !shape) return fail(PFNL_ERR_INVALID, "NULL argument");
    std::string name(tf_name);
    // tolerate a ":0" suffix and a missing "nlvsr/" prefix (checkpoint readers differ)
    if (name.size() > 2 && name.compare(name.size() - 2, 2, ":0") == 0) name.resize(name.size() - 2);
    auto it = h->expected.find(name);
    if (it == h->expected.end()) it = h->expected.find("nlvsr/" + name);
    if (it == h->expected.end()) {
        it = h->optional.find(name);
        if (it == h->optional.end()) it = h->optional.find("nlvsr/" + name);
        if (it == h->optional.end()) return fail(PFNL_ERR_INVALID, "unknown tensor name: " + name);
    }
    if ((int)it->second.size() != rank) return fail(PFNL_ERR_INVALID, "rank mismatch for " + name);
    for (int i = 0; i < rank; ++i)
        if (shape[i] != it->second[i]) return fail(PFNL_ERR_INVALID, "shape mismatch for " + name);
    if (h->weights_external) {        // the placeholders of a received replica are not weights: a caller that sets one tensor sets them all
        h->host.clear();
        h->weights_external = false;
    }
    HostTensor t;
    t.shape = it->second;
    t.data.assign(host, host + numel(t.shape));
    h->host[it->first] = std::move(t);
    h->finalized = false;
    return 0;
}

int pfnl_set_option(pfnl_handle* h, const char* key, const char* value) {
    if (!h || !key || !value) return fail(PFNL_ERR_INVALID, "NULL argument");
    const std::string k(key), v(value);
    ++h->cfg_gen;
    if (k == "nl_sub_sample") {
        const int n = atoi(v.c_str());
        if (n < 1 || n > 64) return fail(PFNL_ERR_INVALID, "nl_sub_sample: an integer >= 1");
        h->opt.nl_sub = n;
        return 0;
    }
    if (k == "bf16_nonlocal") {   // (the split-bf16 kernel of round 1 left the library in round 4: tools/experiments/nonlocal_bf16.hip)
        if (v != "f16") return fail(PFNL_ERR_INVALID, "bf16_nonlocal must be f16");
        return 0;
    }
    const OptionSpec* o = find_option(k);
    if (!o) return fail(PFNL_ERR_INVALID, "unknown option " + k);
    return o->set_named(h->opt, v) ? 0 : fail(PFNL_ERR_INVALID, o->refusal);
}

// the CURRENT value of an option as pfnl_set_option would take it back - whatever set it (pfnl_set_option, an environment variable read by
// pfnl_create, the default): a caller that changes options temporarily restores from here, not from a mirror of its own calls
int pfnl_get_option(pfnl_handle* h, const char* key, char* buf, size_t buflen) {
    if (!h || !key || !buf || buflen < 1) return fail(PFNL_ERR_INVALID, "NULL argument");
    const std::string k(key);
    std::string v;
    if (k == "nl_sub_sample") v = std::to_string(h->opt.nl_sub);
    else if (k == "bf16_nonlocal") v = "f16";
    else if (const OptionSpec* o = find_option(k)) v = o->name_in(h->opt);
    else return fail(PFNL_ERR_INVALID, "unknown option " + k);
    if (v.size() + 1 > buflen) return fail(PFNL_ERR_INVALID, "buffer too small");
    std::memcpy(buf, v.c_str(), v.size() + 1);
    return 0;
}

int pfnl_missing_weights(pfnl_handle* h, int* count) {
    if (!h || !count) return fail(PFNL_ERR_INVALID, "NULL argument");
    int n = 0;
    for (auto& kv : h->expected)
        if (!h->host.count(kv.first)) ++n;
    *count = n;
    return 0;
}

int pfnl_finalize_weights(pfnl_handle* h) {
    if (!h) return fail(PFNL_ERR_INVALID, "NULL handle");
    for (auto& kv : h->expected)
        if (!h->host.count(kv.first)) return fail(PFNL_ERR_STATE, "missing tensor " + kv.first);
    HIPCHK(hipSetDevice(h->cfg.device_id));
    const int T = h->cfg.num_frames, nb = h->cfg.num_block, C = 12 * T, CP = pfnl::nl_padded_ch(C);
    std::vector<float> blob;
    auto W = [&](const std::string& l) -> const std::vector<float>& { return h->host["nlvsr/" + l + "/kernel"].data; };
    auto Bv = [&](const std::string& l) -> const std::vector<float>& { return h->host["nlvsr/" + l + "/bias"].data; };
    auto reserve = [&](size_t n) {
        size_t off = (blob.size() + 63) / 64 * 64;   // 256-byte aligned segments
        blob.resize(off + n, 0.f);
        return off;
    };
    auto put_bias = [&](const std::vector<float>& b) {
        size_t off = reserve(64);
        std::memcpy(&blob[off], b.data(), b.size() * sizeof(float));
        return off;
    };
    auto put_wino = [&](const std::vector<float>& k, int cin_total, int cin_begin) {
        size_t off = reserve(pfnl::wino_pack_floats());
        pfnl::wino_pack_weights(k.data(), cin_total, cin_begin, &blob[off]);
        return off;
    };
    auto put_pack = [&](const std::vector<float>& k, int ks, int cin_total, int cin_begin, int cin, int cout) {
        size_t off = reserve(pfnl::conv_pack_floats(ks, cin));
        pfnl::conv_pack_weights(k.data(), ks, cin_total, cin_begin, cin, cout, &blob[off]);
        return off;
    };

    h->off_zero = reserve(64);
    h->off_conv0_w = reserve(75 * 64);
    std::memcpy(&blob[h->off_conv0_w], W("conv0").data(), 75 * 64 * sizeof(float));
    h->off_conv0_b = put_bias(Bv("conv0"));
    h->blocks.assign(nb, BlockPacks{});
    for (int i = 0; i < nb; ++i) {
        const std::string s = std::to_string(i);
        BlockPacks& k = h->blocks[i];
        k.c1_w = put_pack(W("conv1_" + s), 3, 64, 0, 64, 64);
        k.c1_b = put_bias(Bv("conv1_" + s));
        k.c10_w = put_pack(W("conv10_" + s), 1, 64 * T, 0, 64 * T, 64);
        k.c10_b = put_bias(Bv("conv10_" + s));
        k.c10_s = reserve(pfnl::conv1x1_pack_floats(T));
        pfnl::conv1x1_pack_weights(W("conv10_" + s).data(), T, &blob[k.c10_s]);
        // conv2_i input = concat([base, inp1_t]) (model/pfnl.py:69): rows 0..63 see `base`.
        k.c2a_w = put_pack(W("conv2_" + s), 3, 128, 0, 64, 64);
        k.c2b_w = put_pack(W("conv2_" + s), 3, 128, 64, 64, 64);
        k.c2_b = put_bias(Bv("conv2_" + s));
        k.c1_u = put_wino(W("conv1_" + s), 64, 0);
        k.c2a_u = put_wino(W("conv2_" + s), 128, 0);
        k.c2b_u = put_wino(W("conv2_" + s), 128, 64);
    }
    h->off_m1_w = put_pack(W("convmerge1"), 3, 64 * T, 0, 64 * T, 48);
    h->off_m1_b = put_bias(Bv("convmerge1"));
    h->off_m1_u.assign(T, 0);
    for (int f = 0; f < T; ++f) {
        h->off_m1_u[f] = reserve(pfnl::wino_pack_floats());
        pfnl::wino_pack_weights(W("convmerge1").data(), 64 * T, 64 * f, &blob[h->off_m1_u[f]], 48);
    }
    {
        const auto& k = W("convmerge2");
        h->off_m2_w = reserve(k.size());
        std::memcpy(&blob[h->off_m2_w], k.data(), k.size() * sizeof(float));
        h->off_m2_b = put_bias(Bv("convmerge2"));
    }
    {   // fold the two 1x1 projections of the non-local block: W' = Wg Ww, b' = bg Ww + bw
        h->off_nl_w = reserve((size_t)CP * CP);
        h->off_nl_b = reserve(CP);
        pfnl_nl_fold_gw(W("nlblock_0/g/g").data(), Bv("nlblock_0/g/g").data(), W("nlblock_0/w/w").data(), Bv("nlblock_0/w/w").data(), C, CP,
                        &blob[h->off_nl_w], &blob[h->off_nl_b]);
    }
    {   // optional embedded-Gaussian projections: M = Wt Wp^T, c = bt Wp^T and column C (see nl_qproj_kernel)
        int have = 0;
        for (auto& kv : h->optional) have += (int)h->host.count(kv.first);
        if (have != 0 && have != (int)h->optional.size())
            return fail(PFNL_ERR_STATE, "nlblock_0 theta/phi: all four tensors (two kernels, two biases) or none");
        h->nl_theta = have != 0;
        if (h->nl_theta) {
            h->off_nl_m = reserve((size_t)CP * CP);
            h->off_nl_c = reserve(CP);
            pfnl_nl_fold_theta_phi(W("nlblock_0/theta/theta").data(), Bv("nlblock_0/theta/theta").data(), W("nlblock_0/phi/phi").data(),
                                   Bv("nlblock_0/phi/phi").data(), C, CP, &blob[h->off_nl_m], &blob[h->off_nl_c]);
        }
    }
    {   // bf16 packs of the trunk (precision=bf16)
        std::vector<uint16_t> b16;
        auto reserve16 = [&](size_t n) {
            size_t off = (b16.size() + 127) / 128 * 128;
            b16.resize(off + n, 0);
            return off;
        };
        for (int i = 0; i < nb; ++i) {
            const std::string s = std::to_string(i);
            BlockPacks& k = h->blocks[i];
            k.bf_c1 = reserve16(pfnl::conv3x3_bf16_pack_halfs());
            pfnl::conv3x3_bf16_pack_weights(W("conv1_" + s).data(), 64, 0, &b16[k.bf_c1]);
            k.bf_c10 = reserve16(pfnl::conv1x1_bf16_pack_halfs(T));
            pfnl::conv1x1_bf16_pack_weights(W("conv10_" + s).data(), T, &b16[k.bf_c10]);
            k.bf_c2a = reserve16(pfnl::conv3x3_bf16_pack_halfs());
            pfnl::conv3x3_bf16_pack_weights(W("conv2_" + s).data(), 128, 0, &b16[k.bf_c2a]);
            k.bf_c2b = reserve16(pfnl::conv3x3_bf16_pack_halfs());
            pfnl::conv3x3_bf16_pack_weights(W("conv2_" + s).data(), 128, 64, &b16[k.bf_c2b]);
            k.bf_c1_m16 = reserve16(pfnl::conv3x3_bf16_pack_halfs());
            pfnl::conv3x3_bf16_pack_weights16(W("conv1_" + s).data(), 64, 0, &b16[k.bf_c1_m16]);
            k.bf_c2b_m16 = reserve16(pfnl::conv3x3_bf16_pack_halfs());
            pfnl::conv3x3_bf16_pack_weights16(W("conv2_" + s).data(), 128, 64, &b16[k.bf_c2b_m16]);
        }
        h->off16_m1 = reserve16((size_t)T * pfnl::conv3x3_bf16_pack_halfs());
        for (int f = 0; f < T; ++f)
            pfnl::conv3x3_bf16_pack_weights(W("convmerge1").data(), 64 * T, 64 * f, &b16[h->off16_m1 + (size_t)f * pfnl::conv3x3_bf16_pack_halfs()], 48);
        b16.resize((b16.size() + 1) / 2 * 2 + 2, 0);
        h->wdev16_used = b16.size() / 2;
        if (h->wdev16.ensure(b16.size() / 2)) return fail(PFNL_ERR_NOMEM, "weight allocation failed");
        { pfnl::BlockingCopyGuard guard; HIPCHK(hipMemcpy(h->wdev16.p, b16.data(), b16.size() * sizeof(uint16_t), hipMemcpyHostToDevice)); }
    }
    {   // split-f16 packs of the 3x3 64->64 kernels (conv3x3=split16)
        std::vector<uint16_t> b16;
        const size_t n3 = pfnl::conv3x3_split16_pack_halfs(), n1 = pfnl::conv1x1_split16_pack_halfs(T);
        const size_t blk = 8 * n3 + n1 + pfnl::conv1x1_c10_pack_halfs(T);   // (5 packs of the 32x32x16 kernels + 2 of the 16x16x32 chain kernel + conv1_i's for the 16x16x32 c1c10 form)
        h->off16s_m1 = (size_t)nb * blk;
        const size_t m3 = pfnl::conv_small_pack_halfs(3, 1), m10 = pfnl::conv_small_pack_halfs(1, T);
        const size_t small_base = (size_t)nb * blk + (size_t)T * n3;
        h->off16m_m1 = small_base + (size_t)nb * (3 * m3 + m10);
        b16.resize(h->off16m_m1 + (size_t)T * m3 + 2, 0);
        pfnl::conv_small_pack_weights(W("convmerge1").data(), 3, T, 48, &b16[h->off16m_m1]);
        for (int f = 0; f < T; ++f)
            pfnl::conv3x3_split16_pack_weights(W("convmerge1").data(), 64 * T, 64 * f, &b16[h->off16s_m1 + (size_t)f * n3], 48);
        for (int i = 0; i < nb; ++i) {
            const std::string s = std::to_string(i);
            BlockPacks& k = h->blocks[i];
            k.s_c1 = (size_t)i * blk;
            k.s_c2a = k.s_c1 + n3;
            k.s_c2b = k.s_c1 + 2 * n3;
            k.s_c10 = k.s_c1 + 3 * n3;
            k.s_c2a_sf = k.s_c10 + n1;
            k.s_c2b_sf = k.s_c2a_sf + n3;
            k.s_c10f = k.s_c2b_sf + n3;
            k.s_c2a_m16 = k.s_c10f + pfnl::conv1x1_c10_pack_halfs(T);
            k.s_c2b_m16 = k.s_c2a_m16 + n3;
            k.s_c1_m16 = k.s_c2b_m16 + n3;
            pfnl::conv3x3_split16_pack_weights16(W("conv1_" + s).data(), 64, 0, &b16[k.s_c1_m16], true);
            pfnl::conv3x3_split16_pack_weights16(W("conv2_" + s).data(), 128, 0, &b16[k.s_c2a_m16]);
            pfnl::conv3x3_split16_pack_weights16(W("conv2_" + s).data(), 128, 64, &b16[k.s_c2b_m16]);
            pfnl::conv1x1_c10_pack_weights(W("conv10_" + s).data(), T, &b16[k.s_c10f]);
            pfnl::conv3x3_split16_pack_weights(W("conv2_" + s).data(), 128, 0, &b16[k.s_c2a_sf], 64, true);
            pfnl::conv3x3_split16_pack_weights(W("conv2_" + s).data(), 128, 64, &b16[k.s_c2b_sf], 64, true);
            k.sm_c1 = small_base + (size_t)i * (3 * m3 + m10);
            k.sm_c2 = k.sm_c1 + m3;
            k.sm_c10 = k.sm_c1 + 3 * m3;
            pfnl::conv_small_pack_weights(W("conv1_" + s).data(), 3, 1, 64, &b16[k.sm_c1]);
            pfnl::conv_small_pack_weights(W("conv2_" + s).data(), 3, 2, 64, &b16[k.sm_c2]);
            pfnl::conv_small_pack_weights(W("conv10_" + s).data(), 1, T, 64, &b16[k.sm_c10]);
            pfnl::conv1x1_split16_pack_weights(W("conv10_" + s).data(), T, &b16[k.s_c10]);
            pfnl::conv3x3_split16_pack_weights(W("conv1_" + s).data(), 64, 0, &b16[k.s_c1]);
            pfnl::conv3x3_split16_pack_weights(W("conv2_" + s).data(), 128, 0, &b16[k.s_c2a]);
            pfnl::conv3x3_split16_pack_weights(W("conv2_" + s).data(), 128, 64, &b16[k.s_c2b]);
        }
        h->wdev16s_used = b16.size() / 2;
        if (h->wdev16s.ensure(b16.size() / 2)) return fail(PFNL_ERR_NOMEM, "weight allocation failed");
        { pfnl::BlockingCopyGuard guard; HIPCHK(hipMemcpy(h->wdev16s.p, b16.data(), b16.size() / 2 * 2 * sizeof(uint16_t), hipMemcpyHostToDevice)); }
    }
    {   // the f16-pipe kernels split the weights into binary16 pairs: a weight beyond that range sends the handle to the f32-MFMA kernels
        float wmax = 0.f;
        for (const auto& kv : h->host)
            for (float v : kv.second.data) wmax = std::fmax(wmax, std::fabs(v));
        h->weights_f16_ok = wmax < 65504.0f;
    }
    h->wdev_used = blob.size();
    if (h->wdev.ensure(blob.size())) return fail(PFNL_ERR_NOMEM, "weight allocation failed");
    { pfnl::BlockingCopyGuard guard; HIPCHK(hipMemcpy(h->wdev.p, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice)); }
    h->finalized = true;
    ++h->cfg_gen;
    return 0;
}

int pfnl_workspace_bytes(pfnl_handle* h, int B, int H, int W, size_t* bytes) {
    if (!h || !bytes) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "bad shape");
    // the same expressions forward_device / pfnl_forward allocate with (every buffer a call with these arguments can
    // touch under the current options, the host-pointer staging pair included)
    const size_t T = h->cfg.num_frames, P = (size_t)H * W, N = P / 4, sc = h->cfg.scale;
    const int C = 12 * (int)T;
    const size_t CP = pfnl::nl_padded_ch(C);
    size_t f = 2 * B * N * CP                                   // X, Xo
             + pfnl::nl_partial_floats(B, (int)N, C)            // nlp
             + 2 * B * T * P * 64                               // inp0, inp1
             + 3 * B * P * 64                                   // base, pb, merge (64 floats per pixel)
             + (size_t)B * T * P * 3 + (size_t)B * P * sc * sc * 3;   // stage_in, stage_out
    if (h->opt.bf16 || h->opt.nl_algo != 0) f += (pfnl::nl_f16_scratch_halfs(B, (int)N) + 1) / 2;   // split K / V^T operands (bf16 or f16)
    if (h->nl_theta) f += (size_t)B * N * CP;                   // projected queries (nltype 0 / 2)
    if (h->opt.nl_sub > 1) f += (size_t)B * ((H / 2) / h->opt.nl_sub) * ((W / 2) / h->opt.nl_sub) * CP;   // pooled keys
    const TrunkPlan pl = trunk_plan(h, B, H, W, H);
    f += pl.p10_floats + pl.inp0sf_floats + pl.c10part_floats;   // the buffers that depend on the launch plan
    *bytes = f * sizeof(float);
    return 0;
}

int pfnl_plan(pfnl_handle* h, int B, int H, int W, char* buf, size_t buflen) {
    if (!h || !buf || buflen < 1) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "bad shape");
    const std::string text = pfnl::plan_text(trunk_plan(h, B, H, W, H));
    if (text.size() + 1 > buflen) return fail(PFNL_ERR_INVALID, "buffer too small");
    std::memcpy(buf, text.c_str(), text.size() + 1);
    return 0;
}

// reads and clears a sticky range flag (pinned, device-mapped host memory).  One atomic exchange: pfnl_range_flag is documented for use
// while later forwards are in flight, and with a plain read followed by a plain write of 0 a device store of 1 landing between the two
// would be lost.  A returned 1 may therefore also cover a forward that is still running.
static int range_flag_take(pfnl_handle* h, int slot, int* flagged) {
    unsigned* const f = h->rflag_host + slot;
    *flagged = __atomic_exchange_n(f, 0u, __ATOMIC_ACQ_REL) != 0;
    return 0;
}

int pfnl_range_reruns(pfnl_handle* h, long long* count) {
    if (!h || !count) return fail(PFNL_ERR_INVALID, "NULL argument");
    *count = h->range_reruns;
    return 0;
}

// ---- host-pointer forwards: what moves between the caller's buffers and HBM (the reference times exactly this inside sess.run,
// model/pfnl.py:249-253: feed_dict copy in, fetch copy out).  Pageable buffers go through the handle's pinned strips chunk by
// chunk: worker threads copy host <-> pinned while the copy engine moves the pinned side over PCIe, so neither the runtime's own
// single-threaded pageable staging (measured 6 GB/s: 2.95 ms of a 7.55 ms call at configs[1]) nor a whole-buffer memcpy is on
// the critical path; buffers that are already page-locked (hipHostMalloc / hipHostRegister / torch pin_memory) are DMA targets as
// they are.
namespace {
constexpr size_t STAGE_POOL_MIN = 512u << 10;     // below: one memcpy on the calling thread
constexpr int STAGE_MAX_CHUNKS = 32;

bool host_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();                   // (an ordinary malloc'ed pointer is "invalid value" to the runtime: not an error here)
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

void ensure_pool(pfnl_handle* h) {
    if (!h->pool.th.empty()) return;
    int k = 4;
    if (const char* e = std::getenv("PFNL_HOST_THREADS")) k = std::atoi(e);
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 1 && k > hw - 1) k = hw - 1;
    k = k < 1 ? 1 : (k > 16 ? 16 : k);
    h->pool.start(k, h->cfg.device_id);
}

size_t stage_chunk_bytes(size_t bytes) {
    size_t c = (bytes + STAGE_MAX_CHUNKS - 1) / STAGE_MAX_CHUNKS;
    if (c < (1u << 20)) c = 1u << 20;
    return (c + 4095) & ~(size_t)4095;
}

// caller's host buffer -> device, asynchronous on `s` (the pinned strip is free again once `s` has passed the copies)
int stage_h2d(pfnl_handle* h, float* dst, const void* src, size_t bytes, hipStream_t s) {
    if (host_is_pinned(src)) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        return 0;
    }
    if (h->pin_in.ensure(bytes)) return fail(PFNL_ERR_NOMEM, "pinned staging allocation failed");
    unsigned char* const pin = h->pin_in.p;
    if (bytes < STAGE_POOL_MIN) {
        std::memcpy(pin, src, bytes);
        HIPCHK(hipMemcpyAsync(dst, pin, bytes, hipMemcpyHostToDevice, s));
        return 0;
    }
    ensure_pool(h);
    const size_t csz = stage_chunk_bytes(bytes);
    const int n = (int)((bytes + csz - 1) / csz);
    const unsigned char* const sp = static_cast<const unsigned char*>(src);
    h->pool.run(n, [=](int i) {
        const size_t off = (size_t)i * csz;
        std::memcpy(pin + off, sp + off, std::min(csz, bytes - off));
    });
    hipError_t err = hipSuccess;
    for (int i = 0; i < n; ++i) {
        h->pool.wait_chunk(i);
        const size_t off = (size_t)i * csz;
        if (err == hipSuccess)
            err = hipMemcpyAsync(reinterpret_cast<unsigned char*>(dst) + off, pin + off, std::min(csz, bytes - off), hipMemcpyHostToDevice, s);
    }
    h->pool.wait();
    if (err != hipSuccess) return fail(PFNL_ERR_HIP, std::string("H2D staging: ") + hipGetErrorString(err));
    return 0;
}

// device -> caller's host buffer; returns when `dst` is filled (`s` is idle then)
int stage_d2h(pfnl_handle* h, void* dst, const float* src, size_t bytes, hipStream_t s) {
    if (host_is_pinned(dst)) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    }
    if (h->pin_out.ensure(bytes)) return fail(PFNL_ERR_NOMEM, "pinned staging allocation failed");
    unsigned char* const pin = h->pin_out.p;
    if (bytes < STAGE_POOL_MIN) {
        HIPCHK(hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::memcpy(dst, pin, bytes);
        return 0;
    }
    ensure_pool(h);
    const size_t csz = stage_chunk_bytes(bytes);
    const int n = (int)((bytes + csz - 1) / csz);
    while ((int)h->d2h_ev.size() < n) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->d2h_ev.push_back(e);
    }
    for (int i = 0; i < n; ++i) {
        const size_t off = (size_t)i * csz;
        HIPCHK(hipMemcpyAsync(pin + off, reinterpret_cast<const unsigned char*>(src) + off, std::min(csz, bytes - off), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(h->d2h_ev[i], s));
    }
    HIPCHK(hipEventSynchronize(h->d2h_ev[0]));     // (the forward itself: waited for here, not by every worker)
    unsigned char* const dp = static_cast<unsigned char*>(dst);
    hipEvent_t* const ev = h->d2h_ev.data();
    h->pool.run(n, [=](int i) {
        const size_t off = (size_t)i * csz;
        (void)hipEventSynchronize(ev[i]);
        std::memcpy(dp + off, pin + off, std::min(csz, bytes - off));
    });
    h->pool.wait();
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

const char* const RANGE_MSG_FP32 =
    "a device-pointer forward since the last check produced non-finite values: an operand left the range of the f16-pipe kernels "
    "(|x| < 65504; the non-local block: inputs on a [0,1] scale) or the input was not finite. Re-run with "
    "pfnl_set_option(h, \"strict_fp32\", \"on\") (f32-MFMA kernels: the reference's range), or use host pointers";
const char* const RANGE_MSG_BF16 =
    "a precision=bf16 forward produced non-finite values: the input was not finite, or it left the range of the binary16 operands of "
    "this precision's non-local block and conv0 (inputs on a [0,1] scale, |x| < ~350). precision=fp32 covers the whole fp32 range";
}  // namespace

// ---- the call frame: what a call of pfnl_forward, pfnl_forward_ensemble or pfnl_forward_tiled does around its body

static int refuse_shape(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(PFNL_ERR_INVALID, "B, H, W must be positive");
    if ((H & 1) || (W & 1))
        return fail(PFNL_ERR_INVALID, "H and W must be even (space_to_depth(2), reference model/pfnl.py:57)");
    return 0;
}

// what pfnl_forward and pfnl_forward_ensemble refuse, in the order they report it (pfnl_forward_tiled: the shape and the tiling before the handle)
static int refuse_call(const pfnl_handle* h, const void* in, const void* out, int B, int H, int W) {
    if (!h || !in || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!h->finalized) return fail(PFNL_ERR_STATE, "pfnl_finalize_weights has not been called");
    return refuse_shape(B, H, W);
}

namespace {
// the forwards enqueued in this scope run on the f32-MFMA kernels (trunk_plan reads the handle's strict_once); cleared on every way out
struct StrictOnce {
    pfnl_handle* const h;
    explicit StrictOnce(pfnl_handle* h_) : h(h_) { h->strict_once = true; }
    ~StrictOnce() { h->strict_once = false; }
};

// One call.  body(din, dout, s, slot) enqueues its work on `s` over device pointers; its tail kernels write range-flag word `slot`.
//  - the stream: the caller's if given.  Else a device-pointer call runs on the LEGACY NULL STREAM itself (what a caller that passes
//    torch.cuda.current_stream().cuda_stream == 0 means: same-stream ordering with everything it has enqueued and will enqueue) and a call
//    with a host pointer on the handle's stream.
//  - a host pointer makes the call synchronous: the input goes through stage_in, the result through stage_out, and the call returns with
//    `out` filled and the caller's host buffers free.  It owns flag word 0 and reads it once, behind everything the body enqueued
//    (all members, all runs).  Set = the f16-pipe domain was left somewhere, or the input itself was non-finite: the whole body once more on
//    the f32-MFMA kernels, whose range is the reference's (the fence is not armed there: still non-finite = so is the reference's result),
//    one rerun counted; precision=bf16 has no such kernels and returns PFNL_ERR_RANGE.
//  - a device-pointer call is asynchronous: its body gets the caller's pointers as they are, writes flag word 1 - which pfnl_sync and
//    pfnl_range_flag read - and the frame neither reads a flag nor blocks.
extern "C++" template <class Body>
int run_call(pfnl_handle* h, const void* in, int in_is_device, void* out, int out_is_device, int B, int H, int W, void* stream, Body body) {
    HIPCHK(hipSetDevice(h->cfg.device_id));
    const int T = h->cfg.num_frames, sc = h->cfg.scale;
    const size_t n_in = (size_t)B * T * H * W * 3, n_out = (size_t)B * H * W * sc * sc * 3;
    const bool sync_call = !in_is_device || !out_is_device;
    const int slot = sync_call ? 0 : 1;
    const hipStream_t s = stream ? (hipStream_t)stream : (sync_call ? h->stream : (hipStream_t) nullptr);
    const float* din = (const float*)in;
    float* dout = (float*)out;
    if (!in_is_device) {
        if (h->stage_in.ensure(n_in)) return fail(PFNL_ERR_NOMEM, "staging allocation failed");
        if (int e = stage_h2d(h, h->stage_in.p, in, n_in * sizeof(float), s)) return e;
        din = h->stage_in.p;
    }
    if (!out_is_device) {
        if (h->stage_out.ensure(n_out)) return fail(PFNL_ERR_NOMEM, "staging allocation failed");
        dout = h->stage_out.p;
    }
    if (int e = body(din, dout, s, slot)) return e;
    if (!sync_call) return 0;
    const auto deliver = [&]() -> int {
        if (!out_is_device) return stage_d2h(h, out, dout, n_out * sizeof(float), s);
        HIPCHK(hipStreamSynchronize(s));   // the caller may reuse its host buffer on return
        return 0;
    };
    if (int e = deliver()) return e;
    int flagged = 0;
    if (int e = range_flag_take(h, 0, &flagged)) return e;
    if (!flagged) return 0;
    if (h->opt.bf16) return fail(PFNL_ERR_RANGE, RANGE_MSG_BF16);
    if (h->opt.strict || !h->weights_f16_ok) return 0;   // (these run the f32-MFMA kernels from the start, and arm no fence)
    {
        StrictOnce strict(h);
        if (int e = body(din, dout, s, 0)) return e;
    }
    ++h->range_reruns;
    return deliver();
}
}  // namespace

// ---- graphs: launch-bound shapes replay the plain forward from a hipGraph captured between the staging buffers (pfnl_handle::GraphEntry)

// *exec: the executable graph of the forward at (B, H, W) whose tail kernel writes flag word `slot`, or null - not yet, run eagerly: the
// first call at a shape runs eagerly (workspaces allocated, kernel attributes set), the second captures on `s` and replays
static int graph_for(pfnl_handle* h, int B, int H, int W, int slot, hipStream_t s, hipGraphExec_t* exec) {
    const int T = h->cfg.num_frames, sc = h->cfg.scale;
    if (h->stage_in.ensure((size_t)B * T * H * W * 3) || h->stage_out.ensure((size_t)B * H * W * sc * sc * 3))
        return fail(PFNL_ERR_NOMEM, "staging allocation failed");
    pfnl_handle::GraphEntry* ge = nullptr;
    for (auto& g : h->graphs)
        if (g.B == B && g.H == H && g.W == W && g.slot == slot) ge = &g;
    if (!ge) {
        h->graphs.push_back({B, H, W, 0, nullptr, nullptr, 0, 0, h->cfg_gen, slot});
        ge = &h->graphs.back();
    }
    if (ge->exec && (ge->alloc_gen != g_alloc_gen.load(std::memory_order_relaxed) || ge->cfg_gen != h->cfg_gen)) {   // buffers moved / weights or options changed
        // a replay of this graph may still be running on the stream (an asynchronous device-pointer call followed by pfnl_set_option):
        // whether the runtime defers the destruction of an executing graph depends on its version - wait for it
        HIPCHK(hipStreamSynchronize(s));
        hipGraphExecDestroy(ge->exec);
        hipGraphDestroy(ge->graph);
        ge->exec = nullptr;
        ge->graph = nullptr;
        ge->seen = 0;
    }
    if (!ge->exec && ge->seen_cfg_gen != h->cfg_gen) {   // options / weights changed since the eager run: the path to be
        ge->seen = 0;                                     // captured has not allocated its workspaces / set its attributes yet
        ge->seen_cfg_gen = h->cfg_gen;
    }
    if (!ge->exec && ge->seen >= 1) {
        // (no other thread's blocking copy while the capture is open - it would fail and invalidate the capture: common.h CaptureGuard)
        int fe = 0;
        hipGraph_t g = nullptr;
        hipError_t ce = hipSuccess;
        {
            pfnl::CaptureGuard guard;
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            fe = forward_device(h, h->stage_in.p, h->stage_out.p, B, H, W, s, slot);
            ce = hipStreamEndCapture(s, &g);
        }
        if (fe) return fe;
        if (ce != hipSuccess || !g) return fail(PFNL_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(ce));
        hipGraphExec_t ex = nullptr;
        const hipError_t ie = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        if (ie != hipSuccess) {
            hipGraphDestroy(g);
            return fail(PFNL_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(ie));
        }
        ge->graph = g;
        ge->exec = ex;
        ge->alloc_gen = g_alloc_gen.load(std::memory_order_relaxed);
        ge->cfg_gen = h->cfg_gen;
    }
    if (!ge->exec) ge->seen++;
    *exec = ge->exec;
    return 0;
}

// a replay as a body of the frame: device pointers of the caller's are copied into and out of the staging buffers around the launch.
// null_order: no stream was given.  The eager path relies on the legacy default stream's implicit ordering with the handle's (blocking)
// stream; a graph launch does not take part in it, so order explicitly in both directions (a synchronous call waits for `s` itself).
static int graph_replay(pfnl_handle* h, hipGraphExec_t exec, const float* din, float* dout, int B, int H, int W, hipStream_t s, int slot,
                        bool null_order) {
    const int T = h->cfg.num_frames, sc = h->cfg.scale;
    if (null_order) {
        if (!h->gev && hipEventCreateWithFlags(&h->gev, hipEventDisableTiming) != hipSuccess)
            return fail(PFNL_ERR_HIP, "event creation failed");
        HIPCHK(hipEventRecord(h->gev, nullptr));
        HIPCHK(hipStreamWaitEvent(s, h->gev, 0));
    }
    if (din != h->stage_in.p)
        HIPCHK(hipMemcpyAsync(h->stage_in.p, din, (size_t)B * T * H * W * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipGraphLaunch(exec, s));
    if (dout != h->stage_out.p)
        HIPCHK(hipMemcpyAsync(dout, h->stage_out.p, (size_t)B * H * W * sc * sc * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (null_order && slot == 1) {
        HIPCHK(hipEventRecord(h->gev, s));
        HIPCHK(hipStreamWaitEvent(nullptr, h->gev, 0));
    }
    h->lastB = B;                                             // (forward_device has not run: pfnl_debug_tap reads these)
    h->lastH = H;
    h->lastW = W;
    return 0;
}

int pfnl_forward(pfnl_handle* h, const void* in, int in_is_device, void* out, int out_is_device, int B,
                 int H, int W, void* stream) {
    if (int e = refuse_call(h, in, out, B, H, W)) return e;
    const bool want_graph = !h->prof && (h->opt.graph_mode == 2 || (h->opt.graph_mode == 1 && (size_t)B * h->cfg.num_frames * H * W <= 65536));
    // (a capture cannot run on the null stream: a call that wants a graph and names no stream runs on the handle's, whatever its pointers)
    return run_call(h, in, in_is_device, out, out_is_device, B, H, W, (stream || !want_graph) ? stream : (void*)h->stream,
                    [&](const float* din, float* dout, hipStream_t s, int slot) -> int {
                        hipGraphExec_t exec = nullptr;
                        if (want_graph && !h->strict_once)   // (the rerun of a flagged call is eager and is not captured)
                            if (int e = graph_for(h, B, H, W, slot, s, &exec)) return e;
                        return exec ? graph_replay(h, exec, din, dout, B, H, W, s, slot, !stream)
                                    : forward_device(h, din, dout, B, H, W, s, slot);
                    });
}

// ---- self-ensemble (include/pfnl_hip.h SELF-ENSEMBLE; the rule: pfnl_amd/ensemble.py): the loop around forward_device

// Everything the members of one ensemble touch, sized before the first of them is enqueued: the two ensemble buffers and the workspace of
// both geometries (ensure_workspace only grows; the plan-dependent buffers differ between H x W and W x H, the others - and what
// nonlocal_block sizes by B and the key count - do not)
static int ensemble_presize(pfnl_handle* h, int B, int H, int W, int n) {
    const int T = h->cfg.num_frames, sc = h->cfg.scale;
    if (h->ens_in.ensure((size_t)B * T * H * W * 3) || h->ens_y.ensure((size_t)B * H * W * sc * sc * 3))
        return fail(PFNL_ERR_NOMEM, "ensemble buffer allocation failed");
    if (n > 4)
        if (int e = ensure_workspace(h, trunk_plan(h, B, W, H, W), B, W, H, (W / 2) * (H / 2))) return e;
    return ensure_workspace(h, trunk_plan(h, B, H, W, H), B, H, W, (H / 2) * (W / 2));
}

// members 0 .. n-1 on `s`: din [B][T][H][W][3] -> dout [B][sH][sW][3] (device pointers); under the handle's current strict_once
static int ensemble_device(pfnl_handle* h, const float* din, float* dout, int B, int H, int W, int n, hipStream_t s, int slot) {
    const int T = h->cfg.num_frames, sc = h->cfg.scale;
    if (int e = ensemble_presize(h, B, H, W, n)) return e;
    if (int e = forward_device(h, din, dout, B, H, W, s, slot)) return e;   // member 0 writes acc
    for (int k = 1; k < n; ++k) {
        const bool t = (k & 4) != 0;
        HIPCHK(launch_dihedral(din, h->ens_in.p, B * T, H, W, k, 1.0f, s));
        if (int e = forward_device(h, h->ens_in.p, h->ens_y.p, B, t ? W : H, t ? H : W, s, slot)) return e;
        HIPCHK(launch_dihedral_accum(dout, h->ens_y.p, B, sc * H, sc * W, k, k == n - 1 ? 1.0f / (float)n : 1.0f, s));
    }
    return 0;
}

int pfnl_forward_ensemble(pfnl_handle* h, const void* in, int in_is_device, void* out, int out_is_device, int B, int H, int W, int n,
                          void* stream) {
    if (n != 1 && n != 2 && n != 4 && n != 8) return fail(PFNL_ERR_INVALID, "ensemble: n must be 1, 2, 4 or 8");
    if (n == 1) return pfnl_forward(h, in, in_is_device, out, out_is_device, B, H, W, stream);
    if (int e = refuse_call(h, in, out, B, H, W)) return e;
    return run_call(h, in, in_is_device, out, out_is_device, B, H, W, stream, [&](const float* din, float* dout, hipStream_t s, int slot) {
        return ensemble_device(h, din, dout, B, H, W, n, s, slot);
    });
}

// ---- tiles (include/pfnl_hip.h TILES; the rule: pfnl_amd/tiles.py; the geometry: tile_geom.h): the loop of runs around the forward

int pfnl_tile_axis(int n, int tile, int pad, int* count, int32_t* origin, int32_t* own_first, int32_t* own_count) {
    if (!count) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (const char* why = pfnl::tile_axis_refused(n, tile, pad)) return fail(PFNL_ERR_INVALID, why);
    const pfnl::TileAxis a = pfnl::tile_axis(n, tile, pad);
    *count = a.count;
    for (int i = 0; i < a.count; ++i) {
        if (origin) origin[i] = pfnl::tile_origin(a, i);
        if (own_first) own_first[i] = pfnl::tile_own_first(a, i);
        if (own_count) own_count[i] = pfnl::tile_own_end(a, i) - pfnl::tile_own_first(a, i);
    }
    return 0;
}

// Everything the runs of one tiled call touch, sized before the first of them is enqueued: the two tile buffers at the full run, and for
// both run sizes - the full run and the short last one, whose plans may differ - what the forward of a run needs (ensure_workspace only
// grows; an ensemble adds its own buffers and, for n == 8, the workspace of the transposed tile)
static int tiled_presize(pfnl_handle* h, const pfnl::TileGrid& g, int total, int run, int n) {
    const int T = h->cfg.num_frames, sc = h->cfg.scale, th = g.y.extent, tw = g.x.extent;
    if (h->tile_in.ensure((size_t)run * T * th * tw * 3) || h->tile_y.ensure((size_t)run * th * tw * sc * sc * 3))
        return fail(PFNL_ERR_NOMEM, "tile buffer allocation failed");
    for (const int r : {run, total % run}) {
        if (!r) continue;
        if (int e = n > 1 ? ensemble_presize(h, r, th, tw, n) : ensure_workspace(h, trunk_plan(h, r, th, tw, th), r, th, tw, (th / 2) * (tw / 2)))
            return e;
    }
    return 0;
}

// all runs on `s`: din [B][T][H][W][3] -> dout [B][sH][sW][3] (device pointers); under the handle's current strict_once
static int tiled_device(pfnl_handle* h, const float* din, float* dout, const pfnl::TileGrid& g, int total, int run, int n, hipStream_t s,
                        int slot) {
    const int T = h->cfg.num_frames, sc = h->cfg.scale, th = g.y.extent, tw = g.x.extent;
    if (int e = tiled_presize(h, g, total, run, n)) return e;
    for (int first = 0; first < total; first += run) {
        const int count = total - first < run ? total - first : run;
        HIPCHK(launch_tile_gather(din, h->tile_in.p, g, T, first, count, s));
        if (int e = n > 1 ? ensemble_device(h, h->tile_in.p, h->tile_y.p, count, th, tw, n, s, slot)
                          : forward_device(h, h->tile_in.p, h->tile_y.p, count, th, tw, s, slot))
            return e;
        HIPCHK(launch_tile_scatter(h->tile_y.p, dout, g, sc, first, count, s));
    }
    return 0;
}

int pfnl_forward_tiled(pfnl_handle* h, const void* in, int in_is_device, void* out, int out_is_device, int B, int H, int W,
                       const pfnl_tiling* t, int n, void* stream) {
    if (n != 1 && n != 2 && n != 4 && n != 8) return fail(PFNL_ERR_INVALID, "ensemble: n must be 1, 2, 4 or 8");
    if (!t) return pfnl_forward_ensemble(h, in, in_is_device, out, out_is_device, B, H, W, n, stream);
    if (!h || !in || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (int e = refuse_shape(B, H, W)) return e;
    if (const char* why = pfnl::tiling_refused(H, W, *t)) return fail(PFNL_ERR_INVALID, why);
    const pfnl::TileGrid g = pfnl::tile_grid(H, W, *t);
    const int total = pfnl::tile_total(g, B);
    if (!total) return fail(PFNL_ERR_INVALID, "tile: the tile count overflows a 32-bit integer");
    const int run = pfnl::tile_run(total, t->batch);
    if (g.y.count == 1 && g.x.count == 1 && run == total)       // one tile per clip, one run: the forward itself
        return pfnl_forward_ensemble(h, in, in_is_device, out, out_is_device, B, H, W, n, stream);
    if (!h->finalized) return fail(PFNL_ERR_STATE, "pfnl_finalize_weights has not been called");
    return run_call(h, in, in_is_device, out, out_is_device, B, H, W, stream, [&](const float* din, float* dout, hipStream_t s, int slot) {
        return tiled_device(h, din, dout, g, total, run, n, s, slot);
    });
}

// Single-clip multi-GPU sharding: one rank's horizontal strip of the SR frame.
int pfnl_forward_strip(pfnl_handle* h, const void* in, void* out, int B, int H, int W, int row0, int nrows, void* stream) {
    if (!h || !in || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!h->finalized) return fail(PFNL_ERR_STATE, "pfnl_finalize_weights has not been called");
    if (B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "B, H, W must be positive, H and W even");
    if (row0 < 0 || nrows < 1 || row0 + nrows > H) return fail(PFNL_ERR_INVALID, "strip rows out of range");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    // receptive field of an output row in LR rows: tail conv (1) + convmerge1 (1) + 2 per progressive-fusion block + conv0 (2)
    const int halo = 4 + 2 * h->cfg.num_block;
    int a = row0 - halo, b = row0 + nrows + halo;
    a = a < 0 ? 0 : (a & ~1);                                    // even: space_to_depth(2) rows, Winograd tiles
    b = b > H ? H : ((b + 1) & ~1);
    // non-local block: queries = the packed rows conv0 reads (2 LR rows of margin for its 5x5), keys = the whole frame
    const int W2 = W / 2, H2 = H / 2;
    int qa = (a - 2) >> 1, qb = (b + 2 + 1) >> 1;
    qa = qa < 0 ? 0 : qa;
    qb = qb > H2 ? H2 : qb;
    const StripGeom g{a, b - a, row0 - a, row0 - a + nrows, qa * W2, qb * W2};
    return forward_device(h, (const float*)in, (float*)out, B, H, W, (hipStream_t)stream, 1 /* asynchronous: the flag word pfnl_sync reads */, &g);
}

int pfnl_sync(pfnl_handle* h) {
    if (!h) return fail(PFNL_ERR_INVALID, "NULL handle");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(nullptr));                     // device-pointer calls with stream == NULL run on the null stream
    // (a device-pointer call on a stream of the caller's: the caller synchronises that stream before pfnl_sync)
    int flagged = 0;
    if (int e = range_flag_take(h, 1, &flagged)) return e;
    if (flagged) return fail(PFNL_ERR_RANGE, h->opt.bf16 ? RANGE_MSG_BF16 : RANGE_MSG_FP32);
    return 0;
}

// Page-locked host memory for a caller's input / output buffers (hipHostMalloc): a host-pointer pfnl_forward lets the copy engine read /
// write such a buffer directly instead of staging it through the handle's pinned strips.  Process-wide (no handle: a result may outlive
// the handle that filled it); the caller frees every block it took.
int pfnl_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return fail(PFNL_ERR_INVALID, "bad host allocation");
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess || !p) {
        (void)hipGetLastError();
        return fail(PFNL_ERR_NOMEM, "hipHostMalloc failed");
    }
    *out = p;
    return 0;
}

int pfnl_host_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PFNL_ERR_HIP, "hipHostFree failed");
    }
    return 0;
}

int pfnl_range_flag(pfnl_handle* h, int* flagged) {
    if (!h || !flagged) return fail(PFNL_ERR_INVALID, "NULL argument");
    return range_flag_take(h, 1, flagged);
}

// Weight replica over RCCL (comm.hip holds the communicator): the packed device blobs root -> all.
// A handle that is about to RECEIVE packed weights (broadcast / copy): the blob layout depends on the geometry only, so it
// is built from zeros and the sender's bytes go over it.  Everything data-dependent lives in the three device blobs.
static int prepare_to_receive_weights(pfnl_handle* h) {
    if (h->finalized) return 0;
    for (auto& kv : h->expected)
        if (!h->host.count(kv.first)) {
            HostTensor t;
            t.shape = kv.second;
            t.data.assign(numel(t.shape), 0.f);
            h->host[kv.first] = std::move(t);
        }
    const int e = pfnl_finalize_weights(h);
    if (!e) h->weights_external = true;                         // placeholders: a later pfnl_set_weight starts from an empty set
    return e;
}

int pfnl_copy_weights(pfnl_handle* dst, pfnl_handle* src) {
    if (!dst || !src) return fail(PFNL_ERR_INVALID, "NULL handle");
    if (dst == src) return 0;
    if (!src->finalized) return fail(PFNL_ERR_STATE, "the source handle has no finalized weights");
    if (src->nl_theta) return fail(PFNL_ERR_INVALID, "theta/phi handles carry host-side state: load them through pfnl_set_weight");
    if (int e = prepare_to_receive_weights(dst)) return e;
    if (dst->wdev_used != src->wdev_used || dst->wdev16_used != src->wdev16_used || dst->wdev16s_used != src->wdev16s_used)
        return fail(PFNL_ERR_STATE, "the handles differ in geometry (weight blob sizes)");
    HIPCHK(hipSetDevice(dst->cfg.device_id));
    pfnl::BlockingCopyGuard guard;
    HIPCHK(hipMemcpy(dst->wdev.p, src->wdev.p, src->wdev_used * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(dst->wdev16.p, src->wdev16.p, src->wdev16_used * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(dst->wdev16s.p, src->wdev16s.p, src->wdev16s_used * sizeof(float), hipMemcpyDefault));
    dst->weights_f16_ok = src->weights_f16_ok;                  // (the range of the weights travels with them)
    dst->weights_external = true;
    ++dst->cfg_gen;
    return 0;
}

int pfnl_comm_bcast_weights(pfnl_comm* c, pfnl_handle* h, int root) {
    if (!c || !h) return fail(PFNL_ERR_INVALID, "NULL argument");
    int rank = 0, nranks = 0;
    if (int e = pfnl_comm_rank(c, &rank, &nranks)) return e;
    if (root < 0 || root >= nranks) return fail(PFNL_ERR_INVALID, "bad root");
    if (rank == root && !h->finalized) return fail(PFNL_ERR_STATE, "root has no finalized weights");
    // a rank whose local preparation fails still takes part in the agreement below (status rides in v[6]: the others must not be
    // left waiting inside the collective), then every rank returns the same verdict
    const int prep = rank != root ? prepare_to_receive_weights(h) : 0;
    const std::string prep_msg = prep ? std::string(pfnl_last_error()) : std::string();
    double v[8] = {(double)h->wdev_used, -(double)h->wdev_used, (double)h->wdev16_used, -(double)h->wdev16_used,
                   (double)h->wdev16s_used, -(double)h->wdev16s_used, prep ? 1.0 : 0.0, (rank == root && !h->weights_f16_ok) ? 1.0 : 0.0};
    if (int e = pfnl_comm_allreduce_f64(c, v, 8, PFNL_COMM_MAX)) return e;
    if (v[6] != 0.0) return prep ? fail(prep, prep_msg) : fail(PFNL_ERR_STATE, "another rank could not prepare to receive the weights");
    if (v[0] != -v[1] || v[2] != -v[3] || v[4] != -v[5]) return fail(PFNL_ERR_STATE, "ranks disagree on the weight blob size (geometry / theta-phi option)");
    if (int e = pfnl_comm_bcast(c, h->wdev.p, h->wdev_used * sizeof(float), root)) return e;
    if (int e = pfnl_comm_bcast(c, h->wdev16.p, h->wdev16_used * sizeof(float), root)) return e;
    if (int e = pfnl_comm_bcast(c, h->wdev16s.p, h->wdev16s_used * sizeof(float), root)) return e;
    if (rank != root) {
        h->weights_f16_ok = v[7] == 0.0;                            // (the root's verdict on the range of the weights travels with them)
        h->weights_external = true;
    }
    ++h->cfg_gen;
    return 0;
}

int pfnl_profile_enable(pfnl_handle* h, int enable) {
    if (!h) return fail(PFNL_ERR_INVALID, "NULL handle");
    if (!enable && h->prof) {
        if (prof_collect(h)) return fail(PFNL_ERR_HIP, "event collection failed");
    }
    h->prof = enable != 0;
    h->prof_mode = enable == 2 ? 2 : enable == 3 ? 3 : enable == 4 ? 4 : (enable ? 1 : 0);
    h->prof_gate = h->prof_mode != 3;
    h->run_n = 0;
    h->run_cls = -1;
    return 0;
}

int pfnl_profile_reset(pfnl_handle* h) {
    if (!h) return fail(PFNL_ERR_INVALID, "NULL handle");
    if (prof_collect(h)) return fail(PFNL_ERR_HIP, "event collection failed");
    for (int i = 0; i < PFNL_K_COUNT; ++i) {
        h->prof_ms[i] = 0;
        h->prof_n[i] = 0;
    }
    return 0;
}

int pfnl_profile_read(pfnl_handle* h, double* ms, int64_t* launches) {
    if (!h || !ms || !launches) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (prof_collect(h)) return fail(PFNL_ERR_HIP, "event collection failed");
    for (int i = 0; i < PFNL_K_COUNT; ++i) {
        ms[i] = h->prof_ms[i];
        launches[i] = h->prof_n[i];
    }
    return 0;
}

int pfnl_debug_tap(pfnl_handle* h, const char* name, float* host_dst, size_t count) {
    if (!h || !name || !host_dst) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!h->lastB) return fail(PFNL_ERR_STATE, "no forward has run");
    HIPCHK(hipSetDevice(h->cfg.device_id));
    pfnl::BlockingCopyGuard guard;                                 // (the device-wide wait and the blocking copies below)
    HIPCHK(hipDeviceSynchronize());
    const int B = h->lastB, H = h->lastH, W = h->lastW, T = h->cfg.num_frames;
    const std::string n(name);
    const float* src = nullptr;
    size_t need = 0;
    if (n == "nl_out") {
        need = (size_t)B * H * W * 3 * T;
        if (h->scratch.ensure(need)) return fail(PFNL_ERR_NOMEM, "scratch allocation failed");
        HIPCHK(pfnl::launch_nl_unpack(h->Xo.p, h->scratch.p, B, T, H, W, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        src = h->scratch.p;
    } else if (n == "trunk") {
        need = (size_t)B * T * H * W * 64;
        src = h->inp0.p;
        if (h->opt.bf16) {                                              // bf16 trunk: cast on demand
            if (h->scratch.ensure(need)) return fail(PFNL_ERR_NOMEM, "scratch allocation failed");
            HIPCHK(pfnl::launch_cast_bf16_f32(reinterpret_cast<const uint16_t*>(h->inp0.p), h->scratch.p, need, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            src = h->scratch.p;
        }
    } else if (n == "merge1") {
        need = (size_t)B * H * W * 48;
        if (count != need) return fail(PFNL_ERR_INVALID, "tap size mismatch");
        HIPCHK(hipMemcpy2D(host_dst, 48 * sizeof(float), h->merge.p, h->merge_cstride * sizeof(float), 48 * sizeof(float),
                           (size_t)B * H * W, hipMemcpyDeviceToHost));
        return 0;
    } else {
        return fail(PFNL_ERR_INVALID, "unknown tap " + n);
    }
    if (count != need) return fail(PFNL_ERR_INVALID, "tap size mismatch");
    HIPCHK(hipMemcpy(host_dst, src, need * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
