// Single-op hooks of the C-ABI (include/pfnl_hip.h): one kernel form each, with the weights packed on the host as the forward packs them,
// for the per-op parity tests (pfnl_amd/ops.py).  None of them is on the forward's path.
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pfnl_hip.h"
#include "bars_geom.h"
#include "capi_internal.h"
#include "colour_geom.h"
#include "common.h"
#include "conv_bf16.h"
#include "conv_small.h"
#include "conv_split16.h"
#include "surface_geom.h"
#include "telecine_geom.h"
#include "tile_geom.h"

namespace {

int fail(int code, const std::string& msg) { return pfnl_internal_fail(code, msg); }

// The device side of one hook: its weight pack, its scratch tensors and its launches.  The first failing step is kept and every later
// step does nothing (an allocation or upload then returns null); the buffers are freed when the hook returns, after finish() has
// synchronised the stream or after an early return.
class OpStage {
  public:
    explicit OpStage(void* stream) : s(static_cast<hipStream_t>(stream)) {}
    OpStage(const OpStage&) = delete;
    OpStage& operator=(const OpStage&) = delete;
    ~OpStage() {
        for (void* p : bufs) (void)hipFree(p);
    }

    const hipStream_t s;

    bool ok() const { return e == hipSuccess; }

    template <class T>
    T* alloc(size_t n) {
        void* p = nullptr;
        if (ok()) e = hipMalloc(&p, n * sizeof(T));
        if (!ok()) return nullptr;
        bufs.push_back(p);
        return static_cast<T*>(p);
    }

    // `pack` at the start of a new buffer of pack.size() + extra elements (the extra ones: scratch behind the pack)
    template <class T>
    T* upload(const std::vector<T>& pack, size_t extra = 0) {
        T* d = alloc<T>(pack.size() + extra);
        if (d) {
            pfnl::BlockingCopyGuard guard;                                       // (never beside another handle's graph capture: common.h)
            e = hipMemcpy(d, pack.data(), pack.size() * sizeof(T), hipMemcpyHostToDevice);
        }
        return ok() ? d : nullptr;
    }

    template <class F>
    void run(F&& step) {
        if (ok()) e = step();
    }

    // synchronise, then 0 or PFNL_ERR_HIP with `what` ("<name> op: ") in front of the first error
    int finish(const char* what) {
        run([&] { return hipStreamSynchronize(s); });
        return ok() ? 0 : fail(PFNL_ERR_HIP, what + std::string(hipGetErrorString(e)));
    }

  private:
    hipError_t e = hipSuccess;
    std::vector<void*> bufs;
};

// the persistent kernels address a frame with 32-bit byte offsets: `bpp` bytes per pixel
int frame_too_large(int H, int W, int bpp, const char* kernel = "persistent") {
    if ((long long)H * W * bpp < 0x7fffffffLL) return 0;
    return fail(PFNL_ERR_INVALID, std::string("frame too large for the ") + kernel + " kernel");
}

// the fused epilogues take `addend` and `resid` together or neither
bool paired(const void* addend, const void* resid) { return (addend == nullptr) == (resid == nullptr); }

}  // namespace

// ---- the C-ABI v4 hooks' split-chain arguments: split_s = 0 is no cut (n_full, split_q ignored); otherwise the geometry every split launch
// checks (split_geometry_ok) on the grid of the current device, tested before any allocation or launch
static bool split_args_ok(int H, int W, int items, int T, int n_full, int split_s, int split_q) {
    if (split_s == 0) return true;
    return pfnl::split_geometry_ok(H, W, items, T, n_full, split_s, split_q, pfnl::persistent_grid(pfnl::device_cu_count()));
}
// floats of the parts' raw sums: one [8][32][64] tile per part of every cut chain
static size_t split_partial_floats(int H, int W, int items, int T, int n_full, int split_s) {
    const size_t nchains = (size_t)((W + 31) / 32) * ((H + 7) / 8) * (items / T);
    return (nchains - (size_t)n_full) * split_s * 8 * 32 * 64;
}

static int op_conv3x3_accum_split16(const float* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                                    int frames_per_clip, int H, int W, int cout, int act, void* stream, int n_full = 0, int split_s = 0,
                                    int split_q = 0) {
    OpStage st(stream);
    const int T = frames_per_clip;
    const size_t nh = pfnl::conv3x3_split16_pack_halfs();
    std::vector<uint16_t> pack((size_t)T * nh + 128, 0);
    for (int f = 0; f < T; ++f) pfnl::conv3x3_split16_pack_weights(kernel_host, 64 * T, 64 * f, pack.data() + (size_t)f * nh, cout);
    if (bias_host) std::memcpy(&pack[(size_t)T * nh], bias_host, cout * sizeof(float));
    uint16_t* dw = st.upload(pack);
    float* part = split_s ? st.alloc<float>(split_partial_floats(H, W, clips * T, T, n_full, split_s)) : nullptr;
    st.run([&] {
        pfnl::ConvSplitParams q{in, dw, reinterpret_cast<const float*>(dw + (size_t)T * nh), nullptr, nullptr, out, H, W, clips * T, T, act, 1};
        q.n_full = n_full;
        q.split_s = split_s;
        q.split_q = split_q;
        q.partial = part;
        return pfnl::launch_conv3x3_split16(q, st.s);
    });
    if (split_s) st.run([&] {                                           // the cut chains: the parts' raw sums + bias, act -> out
        pfnl::ConvSplitParams f{};
        f.H = H;
        f.W = W;
        f.items = clips * T;
        f.add_div = T;
        f.act = act;
        f.n_full = n_full;
        f.split_s = split_s;
        f.split_q = split_q;
        f.partial = part;
        f.bias = reinterpret_cast<const float*>(dw + (size_t)T * nh);
        f.out = out;
        return pfnl::launch_c10_finalize(f, st.s);
    });
    return st.finish("accumulating conv (split16) op: ");
}

// the split-format ("SF", conv_split16.h) variants of the split-f16 kernels, op by op.  The hooks take and return fp32
// tensors: fp32 -> SF and SF -> fp32 (hi + lo' 2^-11) conversions bracket the kernel under test, so that each of them is checked
// against the fp64 spec at its own scale and not only inside the forward.
//   which = 0: conv3x3_sf_kernel (input SF by LDS-DMA, epilogue from registers; plain or fused with addend + resid)
//   which = 1: conv3x3_split16_kernel<0, OSF> (conv1_i: fp32 in, SF out)
static int op_conv2_chain(const float* in, const float* kernel_host, const float* bias_host, const float* addend, int add_div, const float* resid,
                          float* out, uint16_t* out_sf, int items, int H, int W, int act, void* stream,
                          int mfma = 32, int n_full = 0, int split_s = 0, int split_q = 0) {
    OpStage st(stream);
    const size_t nh2 = pfnl::conv3x3_split16_pack_halfs();
    const bool m16 = mfma == 16;
    std::vector<uint16_t> pk((m16 ? 4 : 2) * nh2 + 128, 0);
    pfnl::conv3x3_split16_pack_weights(kernel_host, 128, 0, pk.data(), 64, true);
    pfnl::conv3x3_split16_pack_weights(kernel_host, 128, 64, pk.data() + nh2, 64, true);
    if (bias_host) std::memcpy(&pk[2 * nh2], bias_host, 64 * sizeof(float));
    if (m16) {                                                          // conv3x3_sf_chain16_kernel's packs behind the bias, halves as the forward's
        pfnl::conv3x3_split16_pack_weights16(kernel_host, 128, 0, pk.data() + 2 * nh2 + 128);
        pfnl::conv3x3_split16_pack_weights16(kernel_host, 128, 64, pk.data() + 3 * nh2 + 128);
    }
    const size_t npf = (size_t)items * H * W, npb = (size_t)(items / add_div) * H * W;
    uint16_t* dw2 = st.upload(pk);
    uint16_t* tf = st.alloc<uint16_t>(npf * 128);
    uint16_t* tb = st.alloc<uint16_t>(npb * 128);
    st.run([&] { return pfnl::launch_sf_from_f32(in, tf, npf, st.s); });
    st.run([&] { return pfnl::launch_sf_from_f32(addend, tb, npb, st.s); });
    if (out != resid) st.run([&] { return hipMemcpyAsync(out, resid, npf * 256, hipMemcpyDeviceToDevice, st.s); });   // the kernel works in place
    st.run([&] {
        pfnl::ConvSplitParams q{reinterpret_cast<const float*>(tf), dw2 + nh2, reinterpret_cast<const float*>(dw2 + 2 * nh2), nullptr, out, out, H, W, items, add_div, act};
        q.in2 = reinterpret_cast<const float*>(tb);
        q.wpack2 = dw2;
        q.out2 = reinterpret_cast<float*>(out_sf);                      // (null: no split-format copy)
        q.n_full = n_full;
        q.split_s = split_s;
        q.split_q = split_q;
        if (m16) {
            q.wpack_m16 = dw2 + 3 * nh2 + 128;
            q.wpack2_m16 = dw2 + 2 * nh2 + 128;
        }
        return pfnl::launch_conv3x3_sf_chain(q, st.s);
    });
    return st.finish("conv2 chain op: ");
}

// conv1_i + conv10_i as ONE launch (conv3x3_c1c10_kernel): in fp32 [clips*T][H][W][64] -> out1 = inp1 [clips*T][H][W][64], base [clips][H][W][64];
// the kernel writes both in the split format, the hook hands them back as fp32 (hi + lo' 2^-11: what the consumers' MFMAs see)
static int op_conv1_conv10_split16(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                   const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                   void* stream, bool in_sf, int n_full = 0, int split_s = 0, int split_q = 0, bool m16 = false) {
    if (!in || !k1_host || !k10_host || !out1 || !base) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int T = frames_per_clip;
    if (clips < 1 || T < 1 || T > 7 || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const size_t n3 = pfnl::conv3x3_split16_pack_halfs(), n1 = pfnl::conv1x1_c10_pack_halfs(T);
    // [3x3 pack | conv10_i pack | bias | conv10_i bias | m16: the 3x3 pack of the 16x16x32 form]
    std::vector<uint16_t> pack(n3 + n1 + 256 + (m16 ? n3 : 0), 0);
    pfnl::conv3x3_split16_pack_weights(k1_host, 64, 0, pack.data());
    if (m16) pfnl::conv3x3_split16_pack_weights16(k1_host, 64, 0, pack.data() + n3 + n1 + 256, true);
    pfnl::conv1x1_c10_pack_weights(k10_host, T, pack.data() + n3);
    if (b1_host) std::memcpy(&pack[n3 + n1], b1_host, 64 * sizeof(float));
    if (b10_host) std::memcpy(&pack[n3 + n1 + 128], b10_host, 64 * sizeof(float));
    const size_t np1 = (size_t)clips * T * H * W, npb = (size_t)clips * H * W;
    uint16_t* dw = st.upload(pack);
    uint16_t* t1 = st.alloc<uint16_t>(np1 * 128);
    uint16_t* tb = st.alloc<uint16_t>(npb * 128);
    uint16_t* ti = in_sf ? st.alloc<uint16_t>(np1 * 128) : nullptr;
    float* part = split_s ? st.alloc<float>(split_partial_floats(H, W, clips * T, T, n_full, split_s)) : nullptr;
    if (in_sf) st.run([&] { return pfnl::launch_sf_from_f32(in, ti, np1, st.s); });   // (the same split the chain kernel's epilogue applies: sf_split4)
    st.run([&] {
        pfnl::ConvSplitParams q{in_sf ? reinterpret_cast<const float*>(ti) : in, dw, reinterpret_cast<const float*>(dw + n3 + n1), nullptr, nullptr, reinterpret_cast<float*>(t1), H, W, clips * T, T, 1};
        q.in_sf = in_sf ? 1 : 0;
        q.wpack2 = dw + n3;
        q.bias2 = reinterpret_cast<const float*>(dw + n3 + n1 + 128);
        q.out2 = reinterpret_cast<float*>(tb);
        q.n_full = n_full;
        q.split_s = split_s;
        q.split_q = split_q;
        q.partial = part;
        if (m16) q.wpack_m16 = dw + n3 + n1 + 256;
        return pfnl::launch_conv3x3_c1c10(q, st.s);
    });
    if (split_s) st.run([&] {                                           // the cut chains' base from the parts' raw conv10_i sums
        pfnl::ConvSplitParams f{};
        f.H = H;
        f.W = W;
        f.items = clips * T;
        f.add_div = T;
        f.act = 1;
        f.n_full = n_full;
        f.split_s = split_s;
        f.split_q = split_q;
        f.partial = part;
        f.out2 = reinterpret_cast<float*>(tb);
        return pfnl::launch_c10_finalize(f, st.s);
    });
    st.run([&] { return pfnl::launch_sf_to_f32(t1, out1, np1, st.s); });
    st.run([&] { return pfnl::launch_sf_to_f32(tb, base, npb, st.s); });
    return st.finish("conv1+conv10 split16 op: ");
}

// the bf16 chained modes on the third-generation kernel, called directly (PFNL_BF16_V3 does not apply); mfma = 16 adds the M16 pack
static int op_bf16_v3(int mode, const uint16_t* in, const float* k_host, const float* b_host, const uint16_t* addend, int add_div,
                      const uint16_t* resid, uint16_t* out, const float* k10_host, const float* b10_host, uint16_t* base, int items, int H,
                      int W, int act, int mfma, int n_full, int split_s, int split_q, void* stream) {
    OpStage st(stream);
    const int T = add_div;
    const size_t n3 = pfnl::conv3x3_bf16_pack_halfs(), n1 = mode == 2 ? pfnl::conv1x1_bf16_pack_halfs(T) : 0;
    // [3x3 pack | M16 pack | conv10_i pack | bias | conv10_i bias]
    std::vector<uint16_t> pack(2 * n3 + n1 + 256, 0);
    pfnl::conv3x3_bf16_pack_weights(k_host, 64, 0, pack.data());
    pfnl::conv3x3_bf16_pack_weights16(k_host, 64, 0, pack.data() + n3);
    if (mode == 2) pfnl::conv1x1_bf16_pack_weights(k10_host, T, pack.data() + 2 * n3);
    if (b_host) std::memcpy(&pack[2 * n3 + n1], b_host, 64 * sizeof(float));
    if (b10_host) std::memcpy(&pack[2 * n3 + n1 + 128], b10_host, 64 * sizeof(float));
    uint16_t* dw = st.upload(pack);
    float* part = mode == 2 && split_s ? st.alloc<float>(split_partial_floats(H, W, items, T, n_full, split_s)) : nullptr;
    if (!st.ok()) return st.finish("bf16 v3 op: ");
    const float* const db = reinterpret_cast<const float*>(dw + 2 * n3 + n1);
    pfnl::ConvBf16Params q{in, dw, db, addend, resid, out, H, W, items, T, act};
    if (mode == 2) {
        q.x_w = dw + 2 * n3;
        q.x_bias = db + 64;
        q.x_out = base;
    }
    q.n_full = n_full;
    q.split_s = split_s;
    q.split_q = split_q;
    q.partial = part;
    if (mfma == 16) q.wpack16 = dw + n3;
    st.run([&] { return pfnl::launch_conv3x3_bf16_v3(q, mode, st.s); });
    if (mode == 2 && split_s) st.run([&] { return pfnl::launch_c10_finalize_bf16(q, st.s); });
    return st.finish("bf16 v3 op: ");
}

static int op_conv3x3_wino(bool ws, const float* in, const float* kernel_host, const float* bias_host,
                           const float* addend, int add_div, const float* resid, float* out, int items, int H,
                           int W, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "winograd conv needs even H, W");
    if (!paired(addend, resid)) return fail(PFNL_ERR_INVALID, "addend and resid must be given together or not at all");
    if (addend && add_div < 1) return fail(PFNL_ERR_INVALID, "add_div must be >= 1");
    OpStage st(stream);
    std::vector<float> pack(pfnl::wino_pack_floats() + 64, 0.f);
    pfnl::wino_pack_weights(kernel_host, 64, 0, pack.data());
    const size_t boff = pack.size() - 64;
    if (bias_host) std::memcpy(&pack[boff], bias_host, 64 * sizeof(float));
    float* dw = st.upload(pack);
    if (!st.ok()) return st.finish("winograd conv op: ");
    pfnl::WinoParams wp{in, dw, dw + boff, addend, resid, out, H, W, addend ? add_div : 1, act, items};
    st.run([&] { return ws ? pfnl::launch_conv_wino_ws(wp, st.s) : pfnl::launch_conv_wino(wp, st.s); });
    return st.finish("winograd conv op: ");
}

static int op_nonlocal(int bf16 /* 0 f32, 2 f16 split, 3 f16 (hi parts only) */, const float* x, const float* wg, const float* bg, const float* ww, const float* bw,
                       float* out, int B, int T, int H, int W, void* stream) {
    if (!x || !wg || !bg || !ww || !bw || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if ((T != 3 && T != 5 && T != 7) || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1))
        return fail(PFNL_ERR_INVALID, "unsupported non-local geometry");
    OpStage st(stream);
    const int C = 12 * T, CP = pfnl::nl_padded_ch(C), N = (H / 2) * (W / 2);
    // blob: W' [CP][CP] | b' [CP]
    std::vector<float> blob((size_t)CP * CP + CP, 0.f);
    pfnl_nl_fold_gw(wg, bg, ww, bw, C, CP, blob.data(), blob.data() + (size_t)CP * CP);
    const size_t nX = (size_t)B * N * CP;
    const size_t nP = pfnl::nl_partial_floats(B, N, C);
    const size_t n16 = bf16 ? (pfnl::nl_f16_scratch_halfs(B, N) + 1) / 2 : 0;   // in floats
    float* d = st.upload(blob, 2 * nX + nP + n16 + 64);
    if (!d) return st.finish("nonlocal op: ");
    float* dX = d + blob.size();
    float* dXo = dX + nX;
    float* dP = nP ? dXo + nX : nullptr;
    uint16_t* d16 = reinterpret_cast<uint16_t*>(d + (blob.size() + 2 * nX + nP + 63) / 64 * 64);
    st.run([&] { return pfnl::launch_nl_pack(x, dX, B, T, H, W, st.s); });
    st.run([&] {
        return bf16 >= 2 ? pfnl::launch_nl_attn_f16(dX, dXo, d, d + (size_t)CP * CP, dP, d16, B, N, C, st.s, 0, -1, bf16 == 2)
                         : pfnl::launch_nl_attn(dX, dXo, d, d + (size_t)CP * CP, dP, B, N, C, st.s);
    });
    st.run([&] { return pfnl::launch_nl_unpack(dXo, out, B, T, H, W, st.s); });
    return st.finish("nonlocal op: ");
}

// utils.NonLocalBlock in its general form (reference utils.py:18-71: nltype 0 embedded Gaussian, 1 Gaussian, 2 dot product; sub_sample)
// + the stack / space_to_depth / depth_to_space / residual of model/pfnl.py:55-60.  The 1x1 convolutions are folded on the host in fp64
// as pfnl_finalize_weights folds them (capi_internal.h), column C of M / c only for nltype 2; average pooling commutes with the 1x1
// convolutions of g and phi.
static int op_nonlocal_block(const float* x, const float* wg, const float* bg, const float* ww, const float* bw, const float* wt,
                             const float* bt, const float* wp, const float* bp, int nltype, int sub, float* out, int B, int T, int H,
                             int W, void* stream) {
    if (!x || !wg || !bg || !ww || !bw || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (nltype < 0 || nltype > 2) return fail(PFNL_ERR_INVALID, "nltype: 0 | 1 | 2 (3, 'concat', builds no graph in the reference either)");
    if (nltype != 1 && (!wt || !bt || !wp || !bp)) return fail(PFNL_ERR_INVALID, "nltype 0 / 2 need the theta and phi projections");
    if ((T != 3 && T != 5 && T != 7) || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1))
        return fail(PFNL_ERR_INVALID, "unsupported non-local geometry");
    if (sub < 1 || (H / 2) / sub < 1 || (W / 2) / sub < 1) return fail(PFNL_ERR_INVALID, "sub_sample out of range for this geometry");
    OpStage st(stream);
    const int C = 12 * T, CP = pfnl::nl_padded_ch(C), N = (H / 2) * (W / 2);
    const int Nk = sub > 1 ? ((H / 2) / sub) * ((W / 2) / sub) : N;
    // blob: W' [CP][CP] | b' [CP] | M [CP][CP] | c [CP]
    std::vector<float> blob(2 * ((size_t)CP * CP + CP), 0.f);
    float* Wf = blob.data();
    float* bf = Wf + (size_t)CP * CP;
    float* Mf = bf + CP;
    float* cf = Mf + (size_t)CP * CP;
    pfnl_nl_fold_gw(wg, bg, ww, bw, C, CP, Wf, bf);
    if (nltype != 1) pfnl_nl_fold_theta_phi(wt, bt, wp, nltype == 2 ? bp : nullptr, C, CP, Mf, cf);
    const size_t nX = (size_t)B * N * CP, nK = sub > 1 ? (size_t)B * Nk * CP : 0, nP = pfnl::nl_partial_floats(B, N, C);
    float* d = st.upload(blob, 3 * nX + nK + nP);
    if (!d) return st.finish("non-local block op: ");
    float* dX = d + blob.size();
    float* dXo = dX + nX;
    float* dQ = dXo + nX;
    float* dK = dQ + nX;
    float* dP = nP ? dK + nK : nullptr;
    st.run([&] { return pfnl::launch_nl_pack(x, dX, B, T, H, W, st.s); });
    if (nltype != 1)
        st.run([&] { return pfnl::launch_nl_qproj(dX, d + (size_t)CP * CP + CP, d + 2 * (size_t)CP * CP + CP, dQ, B, N, C, st.s, nltype == 2); });
    if (sub > 1) st.run([&] { return pfnl::launch_nl_pool(dX, dK, B, H / 2, W / 2, sub, C, st.s); });
    st.run([&] {
        return pfnl::launch_nl_attn_general(dX, sub > 1 ? dK : dX, Nk, dXo, d, d + (size_t)CP * CP, dP, B, N, C, st.s, nltype != 1 ? dQ : nullptr,
                                            0, -1, nltype == 2);
    });
    st.run([&] { return pfnl::launch_nl_unpack(dXo, out, B, T, H, W, st.s); });
    return st.finish("non-local block op: ");
}

// BARS: the kernel on its own, at either depth
template <typename T>
static int op_content_box(const T* frames, int n, int H, int W, int limit, int32_t* box_dev, uint32_t* rows_dev, uint32_t* cols_dev, void* stream) {
    if (!frames || !box_dev) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (n < 1) return fail(PFNL_ERR_INVALID, "content box: n >= 1");
    if (H < 1 || H > pfnl::BARS_MAX_SIDE || W < 1 || W > pfnl::BARS_MAX_SIDE) return fail(PFNL_ERR_INVALID, "content box: H and W in 1 .. 16384");
    if (limit < 0 || limit > pfnl::BARS_LIMIT_MAX) return fail(PFNL_ERR_INVALID, "content box: limit in 0 .. 219");
    if (reinterpret_cast<uintptr_t>(frames) % sizeof(T)) return fail(PFNL_ERR_INVALID, "content box: uint16 samples are 2-byte aligned");
    if ((reinterpret_cast<uintptr_t>(box_dev) | reinterpret_cast<uintptr_t>(rows_dev) | reinterpret_cast<uintptr_t>(cols_dev)) % 4)
        return fail(PFNL_ERR_INVALID, "content box: box_dev, rows_dev and cols_dev must be 4-byte aligned");
    OpStage st(stream);
    uint32_t* const scratch = st.alloc<uint32_t>(pfnl::bars_scratch_words(n, H, W));
    st.run([&] { return hipMemsetAsync(scratch, 0, (size_t)n * ((size_t)W + 1) * sizeof(uint32_t), st.s); });   // the column sums and the tickets
    st.run([&] { return pfnl::launch_content_box(frames, n, H, W, limit, scratch, pfnl::BarsOut{box_dev, rows_dev, cols_dev}, st.s); });
    return st.finish("content box op: ");
}

extern "C" {

int pfnl_op_conv2d(const float* in, const float* kernel_host, const float* bias_host, const float* addend,
                   int add_div, const float* resid, float* out, int items, int frames_per_item, int H, int W,
                   int ksize, int cout, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if ((ksize != 1 && ksize != 3) || cout < 1 || cout > 64 || items < 1 || frames_per_item < 1 || H < 1 || W < 1)
        return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (!paired(addend, resid))
        return fail(PFNL_ERR_INVALID, "addend and resid must be given together (fused conv2 epilogue) or not at all");
    if (addend && add_div < 1) return fail(PFNL_ERR_INVALID, "add_div must be >= 1");
    if (addend && cout != 64) return fail(PFNL_ERR_INVALID, "fused epilogue needs cout == 64");
    OpStage st(stream);
    const int cin = 64 * frames_per_item;
    std::vector<float> pack(pfnl::conv_pack_floats(ksize, cin) + 64, 0.f);
    pfnl::conv_pack_weights(kernel_host, ksize, cin, 0, cin, cout, pack.data());
    const size_t boff = pack.size() - 64;
    if (bias_host) std::memcpy(&pack[boff], bias_host, cout * sizeof(float));
    float* dw = st.upload(pack);
    st.run([&] {
        pfnl::ConvParams p{};
        p.in = in;
        p.wpack = dw;
        p.bias = dw + boff;   // zeros when bias_host is NULL
        p.addend = addend;
        p.resid = resid;
        p.out = out;
        p.H = H;
        p.W = W;
        p.in_cstride = 64;
        p.out_cstride = cout;
        p.cout = cout;
        p.chunks_per_frame = 64 / pfnl::CONV_CK;
        p.frames_per_item = frames_per_item;
        p.nchunks = frames_per_item * p.chunks_per_frame;
        p.add_div = addend ? add_div : 1;
        p.act = act;
        return pfnl::launch_conv_mfma(p, ksize, items, st.s);
    });
    return st.finish("conv op: ");
}

int pfnl_op_conv2_grouped(const float* in, const float* base, const float* kernel_host, const float* bias_host,
                          const float* resid, float* out, int clips, int frames_per_clip, int H, int W, int act,
                          void* stream) {
    if (!in || !base || !kernel_host || !resid || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (clips < 1 || frames_per_clip < 1 || H < 2 || W < 2 || (H & 1) || (W & 1))
        return fail(PFNL_ERR_INVALID, "grouped conv2 needs even H, W");
    if (int r = frame_too_large(H, W, 256, "grouped")) return r;
    OpStage st(stream);
    const size_t pf = pfnl::wino_pack_floats();
    std::vector<float> pack(2 * pf + 64, 0.f);
    pfnl::wino_pack_weights(kernel_host, 128, 0, pack.data());            // rows 0..63 multiply `base`
    pfnl::wino_pack_weights(kernel_host, 128, 64, pack.data() + pf);      // rows 64..127 multiply the frame
    if (bias_host) std::memcpy(&pack[2 * pf], bias_host, 64 * sizeof(float));
    float* dw = st.upload(pack);
    st.run([&] {
        pfnl::WinoParams wp{};
        wp.in = in;
        wp.in2 = base;
        wp.upack = dw + pf;
        wp.upack2 = dw;
        wp.bias = dw + 2 * pf;
        wp.resid = resid;
        wp.out = out;
        wp.H = H;
        wp.W = W;
        wp.add_div = frames_per_clip;
        wp.act = act;
        wp.items = clips * frames_per_clip;
        return pfnl::launch_conv_wino_ws(wp, st.s);
    });
    return st.finish("grouped conv2 op: ");
}

int pfnl_op_conv3x3_accum(const float* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                          int frames_per_clip, int H, int W, int cout, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (clips < 1 || frames_per_clip < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || cout < 1 || cout > 64)
        return fail(PFNL_ERR_INVALID, "accumulating conv needs even H, W and cout <= 64");
    if (int r = frame_too_large(H, W, 256)) return r;
    OpStage st(stream);
    const int T = frames_per_clip;
    const size_t pf = pfnl::wino_pack_floats();
    std::vector<float> pack(T * pf + 64, 0.f);
    for (int f = 0; f < T; ++f) pfnl::wino_pack_weights(kernel_host, 64 * T, 64 * f, pack.data() + f * pf, cout);
    if (bias_host) std::memcpy(&pack[T * pf], bias_host, cout * sizeof(float));
    float* dw = st.upload(pack);
    st.run([&] {
        pfnl::WinoParams wp{};
        wp.in = in;
        wp.upack = dw;
        wp.upack_stride = (long long)pf;
        wp.accum = 1;
        wp.bias = dw + T * pf;
        wp.out = out;
        wp.H = H;
        wp.W = W;
        wp.add_div = T;
        wp.act = act;
        wp.items = clips * T;
        return pfnl::launch_conv_wino_ws(wp, st.s);
    });
    return st.finish("accumulating conv op: ");
}

int pfnl_op_conv3x3_accum_split16(const float* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                                  int frames_per_clip, int H, int W, int cout, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (clips < 1 || frames_per_clip < 1 || H < 1 || W < 1 || cout < 1 || cout > 64) return fail(PFNL_ERR_INVALID, "accumulating conv needs cout <= 64");
    if (int r = frame_too_large(H, W, 256)) return r;
    return op_conv3x3_accum_split16(in, kernel_host, bias_host, out, clips, frames_per_clip, H, W, cout, act, stream);
}

int pfnl_op_conv3x3_bf16(const uint16_t* in, const float* kernel_host, const float* bias_host, const uint16_t* addend,
                         int add_div, const uint16_t* resid, uint16_t* out, int items, int H, int W, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || H < 1 || W < 1 || !paired(addend, resid)) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const size_t nh = pfnl::conv3x3_bf16_pack_halfs();
    std::vector<uint16_t> pack(nh + 128, 0);
    pfnl::conv3x3_bf16_pack_weights(kernel_host, 64, 0, pack.data());
    if (bias_host) std::memcpy(&pack[nh], bias_host, 64 * sizeof(float));
    uint16_t* dw = st.upload(pack);
    st.run([&] {
        pfnl::ConvBf16Params q{in, dw, reinterpret_cast<const float*>(dw + nh), addend, resid, out, H, W, items, add_div < 1 ? 1 : add_div, act};
        return pfnl::launch_conv3x3_bf16(q, st.s);
    });
    return st.finish("conv3x3 bf16 op: ");
}

int pfnl_op_conv3x3_split16(const float* in, const float* kernel_host, const float* bias_host, const float* addend, int add_div,
                            const float* resid, float* out, int items, int H, int W, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || H < 1 || W < 1 || !paired(addend, resid)) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (addend && (add_div < 1 || items % add_div)) return fail(PFNL_ERR_INVALID, "items must be a multiple of add_div");
    OpStage st(stream);
    const size_t nh = pfnl::conv3x3_split16_pack_halfs();
    std::vector<uint16_t> pack(nh + 128, 0);
    pfnl::conv3x3_split16_pack_weights(kernel_host, 64, 0, pack.data());
    if (bias_host) std::memcpy(&pack[nh], bias_host, 64 * sizeof(float));
    uint16_t* dw = st.upload(pack);
    st.run([&] {
        pfnl::ConvSplitParams q{in, dw, reinterpret_cast<const float*>(dw + nh), addend, resid, out, H, W, items, add_div < 1 ? 1 : add_div, act};
        return pfnl::launch_conv3x3_split16(q, st.s);
    });
    return st.finish("conv3x3 split16 op: ");
}

int pfnl_op_conv1_conv10_bf16(const uint16_t* in, const float* k1_host, const float* b1_host, const float* k10_host,
                              const float* b10_host, uint16_t* out1, uint16_t* base, int clips, int frames_per_clip, int H, int W,
                              void* stream) {
    if (!in || !k1_host || !k10_host || !out1 || !base) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int T = frames_per_clip;
    if (clips < 1 || (T != 3 && T != 5 && T != 7) || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const size_t n3 = pfnl::conv3x3_bf16_pack_halfs(), n1 = pfnl::conv1x1_bf16_pack_halfs(T);
    std::vector<uint16_t> pack(n3 + n1 + 256, 0);
    pfnl::conv3x3_bf16_pack_weights(k1_host, 64, 0, pack.data());
    pfnl::conv1x1_bf16_pack_weights(k10_host, T, pack.data() + n3);
    if (b1_host) std::memcpy(&pack[n3 + n1], b1_host, 64 * sizeof(float));
    if (b10_host) std::memcpy(&pack[n3 + n1 + 128], b10_host, 64 * sizeof(float));
    uint16_t* dw = st.upload(pack);
    st.run([&] {
        pfnl::ConvBf16Params q{in, dw, reinterpret_cast<const float*>(dw + n3 + n1), nullptr, nullptr, out1, H, W, clips * T, T, 1,
                               dw + n3, reinterpret_cast<const float*>(dw + n3 + n1 + 128), base};
        return pfnl::launch_conv3x3_bf16(q, st.s);
    });
    return st.finish("conv1+conv10 bf16 op: ");
}

int pfnl_op_conv3x3_accum_bf16(const uint16_t* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                               int frames_per_clip, int H, int W, int cout, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int T = frames_per_clip;
    if (clips < 1 || T < 1 || T > 7 || H < 1 || W < 1 || cout < 1 || cout > 64) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const size_t nh = pfnl::conv3x3_bf16_pack_halfs();
    std::vector<uint16_t> pack((size_t)T * nh + 128, 0);
    for (int f = 0; f < T; ++f) pfnl::conv3x3_bf16_pack_weights(kernel_host, 64 * T, 64 * f, &pack[(size_t)f * nh], cout);
    if (bias_host) std::memcpy(&pack[(size_t)T * nh], bias_host, cout * sizeof(float));
    uint16_t* dw = st.upload(pack);
    st.run([&] {
        pfnl::ConvBf16Params q{in, dw, reinterpret_cast<const float*>(dw + (size_t)T * nh), nullptr, nullptr, nullptr, H, W, clips * T, T, act};
        q.out_f32 = out;
        return pfnl::launch_conv3x3_bf16(q, st.s);
    });
    return st.finish("conv3x3 accum bf16 op: ");
}

int pfnl_op_conv1x1_bf16(const uint16_t* in, const float* kernel_host, const float* bias_host, uint16_t* out, int items,
                         int frames_per_item, int HW, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int T = frames_per_item;
    if (items < 1 || (T != 3 && T != 5 && T != 7) || HW < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const size_t nh = pfnl::conv1x1_bf16_pack_halfs(T);
    std::vector<uint16_t> pack(nh + 128, 0);
    pfnl::conv1x1_bf16_pack_weights(kernel_host, T, pack.data());
    if (bias_host) std::memcpy(&pack[nh], bias_host, 64 * sizeof(float));
    uint16_t* dw = st.upload(pack);
    st.run([&] { return pfnl::launch_conv1x1_bf16(in, dw, reinterpret_cast<const float*>(dw + nh), out, items, T, HW, act, st.s); });
    return st.finish("conv1x1 bf16 op: ");
}

int pfnl_op_conv1x1_split16(const float* in, const float* kernel_host, const float* bias_host, float* out, int items,
                            int frames_per_item, int HW, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || frames_per_item < 1 || HW < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const int T = frames_per_item;
    const size_t nh = pfnl::conv1x1_split16_pack_halfs(T);
    std::vector<uint16_t> pack(nh + 128, 0);
    pfnl::conv1x1_split16_pack_weights(kernel_host, T, pack.data());
    if (bias_host) std::memcpy(&pack[nh], bias_host, 64 * sizeof(float));
    uint16_t* dw = st.upload(pack);
    st.run([&] { return pfnl::launch_conv1x1_split16(in, dw, reinterpret_cast<const float*>(dw + nh), out, items, T, HW, act, st.s); });
    return st.finish("conv1x1 split16 op: ");
}

// The small-shape trunk kernel (conv_small.hip; ConvSmallParams in conv_small.h says which tensor each source comes from):
// out[i] = act(sum_s conv_ks(src(i, s); kernel rows [64 s, 64 s + 64)) + bias) (+ resid[i]); kernel HWIO [ks, ks, 64 nsrc, cout]
int pfnl_op_conv_small(const float* a, const float* b, int nA, int a_div, int b_mul, int nsrc, const float* kernel_host,
                       const float* bias_host, const float* resid, float* out, int items, int H, int W, int ks, int cout, int act,
                       void* stream) {
    if (!b || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || H < 1 || W < 1 || nsrc < 1 || nsrc > 16 || (ks != 1 && ks != 3) || cout < 1 || cout > 64 || nA < 0 || nA > nsrc || (nA && !a))
        return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const size_t nh = pfnl::conv_small_pack_halfs(ks, nsrc);
    std::vector<uint16_t> pack(nh + 128, 0);
    pfnl::conv_small_pack_weights(kernel_host, ks, nsrc, cout, pack.data());
    if (bias_host) std::memcpy(&pack[nh], bias_host, cout * sizeof(float));
    uint16_t* dw = st.upload(pack);
    st.run([&] {
        pfnl::ConvSmallParams q{a, b, nA, a_div < 1 ? 1 : a_div, b_mul < 1 ? 1 : b_mul, nsrc, dw, reinterpret_cast<const float*>(dw + nh), resid, out, H, W, items, act, ks};
        return pfnl::launch_conv_small(q, st.s);
    });
    return st.finish("conv_small op: ");
}

// One progressive-fusion block on the small-shape kernels as the forward launches it since round 4 (two launches, conv_small.h):
// inp1 = lrelu(conv3x3(x; k1) + b1) together with the per-frame partials of conv10_i; out = x + lrelu(conv3x3(concat([base, inp1_t]); k2)
// + b2) with base = lrelu(sum_t partial_t + b10) built in the second launch's prologue (reference model/pfnl.py:66-71).
int pfnl_op_conv_small_pf_block(const float* x, const float* k1_host, const float* b1_host, const float* k10_host, const float* b10_host,
                                const float* k2_host, const float* b2_host, float* inp1, float* out, int clips, int T, int H, int W,
                                void* stream) {
    if (!x || !k1_host || !k10_host || !k2_host || !inp1 || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (clips < 1 || T < 1 || T > 7 || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const size_t n1 = pfnl::conv_small_pack_halfs(3, 1), n10 = pfnl::conv_small_pack_halfs(1, T), n2 = pfnl::conv_small_pack_halfs(3, 2);
    std::vector<uint16_t> pack(n1 + n10 + n2 + 3 * 128, 0);
    pfnl::conv_small_pack_weights(k1_host, 3, 1, 64, pack.data());
    pfnl::conv_small_pack_weights(k10_host, 1, T, 64, pack.data() + n1);
    pfnl::conv_small_pack_weights(k2_host, 3, 2, 64, pack.data() + n1 + n10);
    uint16_t* const bh = pack.data() + n1 + n10 + n2;
    if (b1_host) std::memcpy(bh, b1_host, 64 * sizeof(float));
    if (b10_host) std::memcpy(bh + 128, b10_host, 64 * sizeof(float));
    if (b2_host) std::memcpy(bh + 256, b2_host, 64 * sizeof(float));
    const size_t F = (size_t)clips * T, tensor = F * H * W * 64;
    uint16_t* dw = st.upload(pack);
    float* part = st.alloc<float>(tensor);
    if (dw && !part) return fail(PFNL_ERR_NOMEM, "allocation failed");   // (the partials: the one scratch failure reported as NOMEM)
    if (!st.ok()) return st.finish("conv_small block op: ");
    const float* const db = reinterpret_cast<const float*>(dw + n1 + n10 + n2);
    st.run([&] {
        pfnl::ConvSmallParams q{nullptr, x, 0, 1, 1, 1, dw, db, nullptr, inp1, H, W, (int)F, 1, 3};
        q.x_wpack = dw + n1;
        q.x_out = part;
        q.x_T = T;
        return pfnl::launch_conv_small(q, st.s);
    });
    st.run([&] {
        pfnl::ConvSmallParams q{part, inp1, 1, T, 1, 2, dw + n1 + n10, db + 128, x, out, H, W, (int)F, 1, 3};
        q.a_nsum = T;
        q.a_bias = db + 64;
        return pfnl::launch_conv_small(q, st.s);
    });
    return st.finish("conv_small block op: ");
}

// the whole of conv2_i in one launch WITH the split-format copy of its output (conv3x3_sf_chain_kernel<true>, option split16_sf0):
// out as pfnl_op_conv3x3_split16_sf(which = 2); out_sf [items][H][W][128] binary16 bit patterns (device) = the split format of `out`
int pfnl_op_conv2_chain_sf0(const float* in, const float* kernel_host, const float* bias_host, const float* base, int add_div, const float* resid,
                            float* out, uint16_t* out_sf, int items, int H, int W, int act, void* stream) {
    if (!in || !kernel_host || !out || !out_sf || !base || !resid) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || H < 1 || W < 1 || add_div < 1 || items % add_div) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    return op_conv2_chain(in, kernel_host, bias_host, base, add_div, resid, out, out_sf, items, H, W, act, stream);
}

int pfnl_op_conv3x3_split16_sf(int which, const float* in, const float* kernel_host, const float* bias_host, const float* addend,
                               int add_div, const float* resid, float* out, int items, int H, int W, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (which < 0 || which > 2 || items < 1 || H < 1 || W < 1 || !paired(addend, resid)) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (addend && ((which != 0 && which != 2) || add_div < 1 || items % add_div)) return fail(PFNL_ERR_INVALID, "fused mode: which = 0 or 2, items a multiple of add_div");
    if (which == 2) {   // the whole of conv2_i (conv3x3_sf_chain_kernel): kernel_host = HWIO [3,3,128,64], `addend` = base [items/add_div][H][W][64] fp32
        if (!addend) return fail(PFNL_ERR_INVALID, "which = 2 needs base (addend argument) and resid");
        return op_conv2_chain(in, kernel_host, bias_host, addend, add_div, resid, out, nullptr, items, H, W, act, stream);
    }
    OpStage st(stream);
    const size_t nh = pfnl::conv3x3_split16_pack_halfs();
    std::vector<uint16_t> pack(nh + 128, 0);
    pfnl::conv3x3_split16_pack_weights(kernel_host, 64, 0, pack.data(), 64, which == 0);
    if (bias_host) std::memcpy(&pack[nh], bias_host, 64 * sizeof(float));
    const size_t npix = (size_t)items * H * W;
    uint16_t* dw = st.upload(pack);
    uint16_t* tmp = st.alloc<uint16_t>(npix * 128);
    if (which == 0) {
        st.run([&] { return pfnl::launch_sf_from_f32(in, tmp, npix, st.s); });
        st.run([&] {
            pfnl::ConvSplitParams q{reinterpret_cast<const float*>(tmp), dw, reinterpret_cast<const float*>(dw + nh), addend, resid, out, H, W, items, add_div < 1 ? 1 : add_div, act};
            return pfnl::launch_conv3x3_sf(q, st.s);
        });
    } else {
        st.run([&] {
            pfnl::ConvSplitParams q{in, dw, reinterpret_cast<const float*>(dw + nh), nullptr, nullptr, reinterpret_cast<float*>(tmp), H, W, items, 1, act};
            q.out_sf = 1;
            return pfnl::launch_conv3x3_split16(q, st.s);
        });
        st.run([&] { return pfnl::launch_sf_to_f32(tmp, out, npix, st.s); });
    }
    return st.finish("conv3x3 split16 SF op: ");
}

int pfnl_op_conv1_conv10_split16(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                 const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                 void* stream) {
    return op_conv1_conv10_split16(in, k1_host, b1_host, k10_host, b10_host, out1, base, clips, frames_per_clip, H, W, stream, false);
}
// ... with the input converted to the split format first and the halo taken from there by LDS-DMA (conv3x3_c1c10_kernel<true>, option
// split16_sf0): the same operands in the same order - bit-identical to pfnl_op_conv1_conv10_split16
int pfnl_op_conv1_conv10_split16_sf0(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                     const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                     void* stream) {
    return op_conv1_conv10_split16(in, k1_host, b1_host, k10_host, b10_host, out1, base, clips, frames_per_clip, H, W, stream, true);
}

// ---- C-ABI v4: the chained launches with the MFMA shape and the split-chain geometry chosen by the caller instead of trunk_plan, so that the
// 16x16x32 forms and every cut of a chain can be compared with the spec op by op (include/pfnl_hip.h)
int pfnl_op_conv2_chain_ex(const float* in, const float* kernel_host, const float* bias_host, const float* base, int add_div, const float* resid,
                           float* out, int items, int H, int W, int act, int mfma, int n_full, int split_s, int split_q, void* stream) {
    if (!in || !kernel_host || !out || !base || !resid) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || H < 1 || W < 1 || add_div < 1 || items % add_div) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (int r = frame_too_large(H, W, 256)) return r;
    if (mfma != 16 && mfma != 32) return fail(PFNL_ERR_INVALID, "mfma must be 16 or 32");
    if (mfma == 16 && split_s) return fail(PFNL_ERR_INVALID, "split chains run on the 32x32x16 kernel only");
    if (!split_args_ok(H, W, items, add_div, n_full, split_s, split_q)) return fail(PFNL_ERR_INVALID, "invalid split-chain geometry");
    return op_conv2_chain(in, kernel_host, bias_host, base, add_div, resid, out, nullptr, items, H, W, act, stream, mfma, n_full, split_s, split_q);
}

int pfnl_op_conv1_conv10_split16_ex(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                    const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                    int n_full, int split_s, int split_q, void* stream) {
    if (!in || !k1_host || !k10_host || !out1 || !base) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int T = frames_per_clip;
    if (clips < 1 || T < 1 || T > 7 || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (int r = frame_too_large(H, W, 256)) return r;
    if (!split_args_ok(H, W, clips * T, T, n_full, split_s, split_q)) return fail(PFNL_ERR_INVALID, "invalid split-chain geometry");
    return op_conv1_conv10_split16(in, k1_host, b1_host, k10_host, b10_host, out1, base, clips, T, H, W, stream, false, n_full, split_s, split_q);
}

// ... with the MFMA shape of conv1_i's 3x3 stage chosen by the caller: 16 = conv3x3_c1c10_kernel's 16x16x32 form (whole rounds only), 32 = the hook above
int pfnl_op_conv1_conv10_split16_mfma(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                      const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                      int mfma, int n_full, int split_s, int split_q, void* stream) {
    if (mfma != 16 && mfma != 32) return fail(PFNL_ERR_INVALID, "mfma must be 16 or 32");
    if (mfma == 16 && split_s) return fail(PFNL_ERR_INVALID, "split chains run on the 32x32x16 kernel only");
    if (mfma == 32) return pfnl_op_conv1_conv10_split16_ex(in, k1_host, b1_host, k10_host, b10_host, out1, base, clips, frames_per_clip, H, W, n_full, split_s, split_q, stream);
    if (!in || !k1_host || !k10_host || !out1 || !base) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int T = frames_per_clip;
    if (clips < 1 || T < 1 || T > 7 || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (int r = frame_too_large(H, W, 256)) return r;
    if (!split_args_ok(H, W, clips * T, T, n_full, split_s, split_q)) return fail(PFNL_ERR_INVALID, "invalid split-chain geometry");
    return op_conv1_conv10_split16(in, k1_host, b1_host, k10_host, b10_host, out1, base, clips, T, H, W, stream, false, n_full, 0, split_q, true);
}

int pfnl_op_conv3x3_accum_split16_ex(const float* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                                     int frames_per_clip, int H, int W, int cout, int act, int n_full, int split_s, int split_q, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (clips < 1 || frames_per_clip < 1 || H < 1 || W < 1 || cout < 1 || cout > 64) return fail(PFNL_ERR_INVALID, "accumulating conv needs cout <= 64");
    if (int r = frame_too_large(H, W, 256)) return r;
    if (!split_args_ok(H, W, clips * frames_per_clip, frames_per_clip, n_full, split_s, split_q)) return fail(PFNL_ERR_INVALID, "invalid split-chain geometry");
    return op_conv3x3_accum_split16(in, kernel_host, bias_host, out, clips, frames_per_clip, H, W, cout, act, stream, n_full, split_s, split_q);
}

int pfnl_op_conv3x3_bf16_ex(const uint16_t* in, const float* kernel_host, const float* bias_host, const uint16_t* addend, int add_div,
                            const uint16_t* resid, uint16_t* out, int items, int H, int W, int act, int mfma, int n_full, int split_s,
                            int split_q, void* stream) {
    if (!in || !kernel_host || !addend || !resid || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || H < 1 || W < 1 || add_div < 1 || items % add_div) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (int r = frame_too_large(H, W, 128)) return r;
    if (mfma != 16 && mfma != 32) return fail(PFNL_ERR_INVALID, "mfma must be 16 or 32");
    if (!split_args_ok(H, W, items, add_div, n_full, split_s, split_q)) return fail(PFNL_ERR_INVALID, "invalid split-chain geometry");
    return op_bf16_v3(1, in, kernel_host, bias_host, addend, add_div, resid, out, nullptr, nullptr, nullptr, items, H, W, act, mfma, n_full,
                      split_s, split_q, stream);
}

int pfnl_op_conv1_conv10_bf16_ex(const uint16_t* in, const float* k1_host, const float* b1_host, const float* k10_host, const float* b10_host,
                                 uint16_t* out1, uint16_t* base, int clips, int frames_per_clip, int H, int W, int mfma, int n_full, int split_s,
                                 int split_q, void* stream) {
    if (!in || !k1_host || !k10_host || !out1 || !base) return fail(PFNL_ERR_INVALID, "NULL argument");
    const int T = frames_per_clip;
    if (clips < 1 || (T != 3 && T != 5 && T != 7) || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    if (int r = frame_too_large(H, W, 128)) return r;
    if (mfma != 16 && mfma != 32) return fail(PFNL_ERR_INVALID, "mfma must be 16 or 32");
    if (!split_args_ok(H, W, clips * T, T, n_full, split_s, split_q)) return fail(PFNL_ERR_INVALID, "invalid split-chain geometry");
    return op_bf16_v3(2, in, k1_host, b1_host, nullptr, T, nullptr, out1, k10_host, b10_host, base, clips * T, H, W, 1, mfma, n_full, split_s,
                      split_q, stream);
}

// conv10_i with its input and / or output in the split format (fp32 at the hook's interface, see above)
int pfnl_op_conv1x1_split16_sf(const float* in, const float* kernel_host, const float* bias_host, float* out, int items,
                               int frames_per_item, int HW, int act, int in_sf, int out_sf, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || frames_per_item < 1 || HW < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const int T = frames_per_item;
    const size_t nh = pfnl::conv1x1_split16_pack_halfs(T);
    std::vector<uint16_t> pack(nh + 128, 0);
    pfnl::conv1x1_split16_pack_weights(kernel_host, T, pack.data());
    if (bias_host) std::memcpy(&pack[nh], bias_host, 64 * sizeof(float));
    const size_t npin = (size_t)items * T * HW, npout = (size_t)items * HW;
    uint16_t* dw = st.upload(pack);
    uint16_t* tin = st.alloc<uint16_t>(npin * 128);
    uint16_t* tout = st.alloc<uint16_t>(npout * 128);
    if (in_sf) st.run([&] { return pfnl::launch_sf_from_f32(in, tin, npin, st.s); });
    st.run([&] {
        return pfnl::launch_conv1x1_split16(in_sf ? reinterpret_cast<const float*>(tin) : in, dw, reinterpret_cast<const float*>(dw + nh),
                                            out_sf ? reinterpret_cast<float*>(tout) : out, items, T, HW, act, st.s, in_sf != 0, out_sf != 0);
    });
    if (out_sf) st.run([&] { return pfnl::launch_sf_to_f32(tout, out, npout, st.s); });
    return st.finish("conv1x1 split16 SF op: ");
}

int pfnl_op_conv1x1_stream(const float* in, const float* kernel_host, const float* bias_host, float* out, int items,
                           int frames_per_item, int HW, int act, void* stream) {
    if (!in || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (items < 1 || frames_per_item < 1 || HW < 1) return fail(PFNL_ERR_INVALID, "unsupported conv geometry");
    OpStage st(stream);
    const int T = frames_per_item;
    std::vector<float> pack(pfnl::conv1x1_pack_floats(T) + 64, 0.f);
    pfnl::conv1x1_pack_weights(kernel_host, T, pack.data());
    const size_t boff = pack.size() - 64;
    if (bias_host) std::memcpy(&pack[boff], bias_host, 64 * sizeof(float));
    float* dw = st.upload(pack);
    st.run([&] { return pfnl::launch_conv1x1_stream(in, dw, dw + boff, out, items, T, HW, act, st.s); });
    return st.finish("conv1x1 op: ");
}

int pfnl_op_conv3x3_winograd(const float* in, const float* kernel_host, const float* bias_host,
                             const float* addend, int add_div, const float* resid, float* out, int items, int H,
                             int W, int act, void* stream) {
    return op_conv3x3_wino(false, in, kernel_host, bias_host, addend, add_div, resid, out, items, H, W, act, stream);
}

int pfnl_op_conv3x3_winograd_ws(const float* in, const float* kernel_host, const float* bias_host,
                                const float* addend, int add_div, const float* resid, float* out, int items, int H,
                                int W, int act, void* stream) {
    return op_conv3x3_wino(true, in, kernel_host, bias_host, addend, add_div, resid, out, items, H, W, act, stream);
}

int pfnl_op_nonlocal(const float* x, const float* wg, const float* bg, const float* ww, const float* bw,
                     float* out, int B, int T, int H, int W, void* stream) {
    return op_nonlocal(0, x, wg, bg, ww, bw, out, B, T, H, W, stream);
}

int pfnl_op_nonlocal_split16(const float* x, const float* wg, const float* bg, const float* ww, const float* bw,
                             float* out, int B, int T, int H, int W, void* stream) {
    return op_nonlocal(2, x, wg, bg, ww, bw, out, B, T, H, W, stream);
}

int pfnl_op_nonlocal_f16(const float* x, const float* wg, const float* bg, const float* ww, const float* bw,
                         float* out, int B, int T, int H, int W, void* stream) {
    return op_nonlocal(3, x, wg, bg, ww, bw, out, B, T, H, W, stream);
}

int pfnl_op_nonlocal_embedded(const float* x, const float* wg, const float* bg, const float* ww, const float* bw,
                              const float* wt, const float* bt, const float* wp, const float* bp, float* out, int B, int T,
                              int H, int W, void* stream) {
    if (!wt || !bt || !wp || !bp) return fail(PFNL_ERR_INVALID, "NULL argument");
    return op_nonlocal_block(x, wg, bg, ww, bw, wt, bt, wp, bp, 0, 1, out, B, T, H, W, stream);
}

int pfnl_op_nonlocal_block(const float* x, const float* wg, const float* bg, const float* ww, const float* bw, const float* wt,
                           const float* bt, const float* wp, const float* bp, int nltype, int sub_sample, float* out, int B, int T,
                           int H, int W, void* stream) {
    return op_nonlocal_block(x, wg, bg, ww, bw, wt, bt, wp, bp, nltype, sub_sample, out, B, T, H, W, stream);
}

int pfnl_op_conv0_ex(const float* x, const float* kernel_host, const float* bias_host, float* out, int B, int T, int H, int W,
                     int f32, void* stream) {
    if (!x || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if ((T != 3 && T != 5 && T != 7) || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "unsupported conv0 geometry");
    OpStage st(stream);
    const int CP = pfnl::nl_padded_ch(12 * T), N = (H / 2) * (W / 2);
    std::vector<float> wb(75 * 64 + 64, 0.f);
    std::memcpy(wb.data(), kernel_host, 75 * 64 * sizeof(float));
    if (bias_host) std::memcpy(&wb[75 * 64], bias_host, 64 * sizeof(float));
    float* d = st.upload(wb, (size_t)B * N * CP);
    // conv0 reads the frame stack in the packed space_to_depth layout the non-local block leaves it in
    st.run([&] { return pfnl::launch_nl_pack(x, d + wb.size(), B, T, H, W, st.s); });
    st.run([&] { return pfnl::launch_conv0(d + wb.size(), d, d + 75 * 64, out, B, T, H, W, st.s, nullptr, f32 != 0); });
    return st.finish("conv0 op: ");
}

int pfnl_op_conv0_bf16(const float* x, const float* kernel_host, const float* bias_host, uint16_t* out, int B, int T, int H, int W,
                       void* stream) {
    if (!x || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if ((T != 3 && T != 5 && T != 7) || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "unsupported conv0 geometry");
    OpStage st(stream);
    const int CP = pfnl::nl_padded_ch(12 * T), N = (H / 2) * (W / 2);
    std::vector<float> wb(75 * 64 + 64, 0.f);
    std::memcpy(wb.data(), kernel_host, 75 * 64 * sizeof(float));
    if (bias_host) std::memcpy(&wb[75 * 64], bias_host, 64 * sizeof(float));
    float* d = st.upload(wb, (size_t)B * N * CP);
    st.run([&] { return pfnl::launch_nl_pack(x, d + wb.size(), B, T, H, W, st.s); });
    st.run([&] { return pfnl::launch_conv0_bf16(d + wb.size(), d, d + 75 * 64, out, B, T, H, W, st.s); });
    return st.finish("conv0 bf16 op: ");
}

int pfnl_op_conv0(const float* x, const float* kernel_host, const float* bias_host, float* out, int B, int T, int H, int W,
                  void* stream) {
    return pfnl_op_conv0_ex(x, kernel_host, bias_host, out, B, T, H, W, 0, stream);
}

int pfnl_op_tail(const float* merge, const float* x, const float* kernel_host, const float* bias_host, float* out, int B,
                 int T, int H, int W, int scale, void* stream) {
    if (!merge || !x || !kernel_host || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (B < 1 || T < 1 || H < 1 || W < 1 || (scale != 2 && scale != 4)) return fail(PFNL_ERR_INVALID, "unsupported tail geometry");
    OpStage st(stream);
    const int CO = scale == 4 ? 12 : 3;
    std::vector<float> wb(9 * 12 * CO + 64, 0.f);
    std::memcpy(wb.data(), kernel_host, (size_t)9 * 12 * CO * sizeof(float));
    if (bias_host) std::memcpy(&wb[9 * 12 * CO], bias_host, CO * sizeof(float));
    float* d = st.upload(wb);
    st.run([&] { return pfnl::launch_tail(merge, x, d, d + 9 * 12 * CO, out, B, T, H, W, scale, 48, st.s); });
    return st.finish("tail op: ");
}

int pfnl_op_gather_windows(const float* frames, float* win, int F, int first, int count, int T, int H, int W, void* stream) {
    if (!frames || !win) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (F < 1 || first < 0 || count < 1 || first + count > F || T < 1 || !(T & 1) || H < 1 || W < 1 || ((size_t)H * W * 3) % 4)
        return fail(PFNL_ERR_INVALID, "bad window geometry (H*W*3 must be a multiple of 4, T odd, first + count <= F)");
    HIPCHK(pfnl::launch_gather_windows(frames, win, F, first, count, T, (size_t)H * W * 3, (hipStream_t)stream));
    return 0;
}

int pfnl_op_gather_windows_u8(const uint8_t* ring, float* win, int cap, long long last, long long first, int count, int T, int H, int W,
                              void* stream) {
    if (!ring || !win) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (cap < 1 || last < 0 || first < 0 || count < 1 || T < 1 || !(T & 1) || H < 1 || W < 1 || ((size_t)H * W * 3) % 4)
        return fail(PFNL_ERR_INVALID, "bad window geometry (H*W*3 must be a multiple of 4, T odd, cap >= 1, first, last >= 0)");
    if (first + count - 1 > last) return fail(PFNL_ERR_INVALID, "a window's centre frame lies beyond `last`");
    if (reinterpret_cast<uintptr_t>(ring) % 4 || reinterpret_cast<uintptr_t>(win) % 16)
        return fail(PFNL_ERR_INVALID, "ring must be 4-byte aligned and win 16-byte aligned");
    // the frames the windows name, after the clamps, must all be in the ring at once
    const long long lo = first - T / 2 < 0 ? 0 : first - T / 2, hi = first + count - 1 + T / 2 > last ? last : first + count - 1 + T / 2;
    if (hi - lo + 1 > cap) return fail(PFNL_ERR_INVALID, "the windows span more frames than the ring holds");
    HIPCHK(pfnl::launch_gather_windows_u8(ring, win, cap, last, first, count, T, (size_t)H * W * 3, (hipStream_t)stream));
    return 0;
}

int pfnl_op_scene_sad_u8(const uint8_t* a, const uint8_t* b, int H, int W, unsigned long long* out_dev, void* stream) {
    if (!a || !b || !out_dev) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "H and W must be positive");
    if (reinterpret_cast<uintptr_t>(out_dev) % 8) return fail(PFNL_ERR_INVALID, "out_dev must be 8-byte aligned");
    OpStage st(stream);
    unsigned long long* scratch = st.alloc<unsigned long long>(2);
    st.run([&] { return hipMemsetAsync(scratch, 0, 2 * sizeof(unsigned long long), st.s); });
    st.run([&] { return pfnl::launch_scene_sad_u8(a, b, (size_t)H * W, scratch, pfnl::SceneDecision{out_dev, nullptr, 0, 0, 0, 0, 0, 0}, st.s); });
    return st.finish("scene sad op: ");
}

int pfnl_op_gather_windows_u8_scenes(const uint8_t* ring, const long long* scene_first_dev, float* win, int cap, long long last, long long first,
                                     int count, int T, int H, int W, void* stream) {
    if (!ring || !scene_first_dev || !win) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (cap < 1 || last < 0 || first < 0 || count < 1 || T < 1 || !(T & 1) || H < 1 || W < 1 || ((size_t)H * W * 3) % 4)
        return fail(PFNL_ERR_INVALID, "bad window geometry (H*W*3 must be a multiple of 4, T odd, cap >= 1, first, last >= 0)");
    if (first + count - 1 > last) return fail(PFNL_ERR_INVALID, "a window's centre frame lies beyond `last`");
    if (reinterpret_cast<uintptr_t>(ring) % 4 || reinterpret_cast<uintptr_t>(win) % 16 || reinterpret_cast<uintptr_t>(scene_first_dev) % 8)
        return fail(PFNL_ERR_INVALID, "ring must be 4-byte aligned, scene_first 8-byte and win 16-byte aligned");
    // every frame the windows can name lies between the plain clamps, whatever the scenes: those must all be in the ring at once
    const long long lo = first - T / 2 < 0 ? 0 : first - T / 2, hi = first + count - 1 + T / 2 > last ? last : first + count - 1 + T / 2;
    if (hi - lo + 1 > cap) return fail(PFNL_ERR_INVALID, "the windows span more frames than the ring holds");
    HIPCHK(pfnl::launch_gather_windows_u8_scenes(ring, scene_first_dev, win, cap, last, first, count, T, (size_t)H * W * 3, (hipStream_t)stream));
    return 0;
}

int pfnl_op_quantise_u8(const float* sr, uint8_t* out, size_t n, void* stream) {
    if (!sr || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!n || n % 4) return fail(PFNL_ERR_INVALID, "element count must be a positive multiple of 4");
    HIPCHK(pfnl::launch_quantise(sr, out, n, (hipStream_t)stream));
    return 0;
}

int pfnl_yuv_coefficients(int matrix, int full_range, int32_t out[15]) {
    if (!out) return fail(PFNL_ERR_INVALID, "NULL argument");
    pfnl::YuvCoef c;
    if (!pfnl::yuv_coefficients(8, matrix, full_range, &c)) return fail(PFNL_ERR_INVALID, "yuv: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    const int v[15] = {c.y0, c.yr, c.yg, c.yb, c.cbr, c.cbg, c.cbb, c.crr, c.crg, c.crb, c.dy, c.drv, c.dgu, c.dgv, c.dbu};
    for (int k = 0; k < 15; ++k) out[k] = v[k];
    return 0;
}

// as below: refused before any HIP call; *c = the table of (matrix, full_range)
static int yuv_op_refused(const void* a, const void* b, int fmt, int matrix, int full_range, int n, int H, int W, pfnl::YuvCoef* c) {
    if (!a || !b) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (fmt != PFNL_PIX_NV12 && fmt != PFNL_PIX_I420) return fail(PFNL_ERR_INVALID, "yuv: fmt must be PFNL_PIX_NV12 or PFNL_PIX_I420");
    if (!pfnl::yuv_coefficients(8, matrix, full_range, c)) return fail(PFNL_ERR_INVALID, "yuv: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    if (n < 1 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "yuv: n >= 1, H and W positive and even (4:2:0)");
    return 0;
}

static int siting_refused(int siting) {
    if (siting < PFNL_SITING_LEFT || siting > PFNL_SITING_TOPLEFT)
        return fail(PFNL_ERR_INVALID, "yuv: siting must be PFNL_SITING_LEFT, PFNL_SITING_CENTER or PFNL_SITING_TOPLEFT");
    return 0;
}

int pfnl_op_yuv420_to_rgb_u8_sited(const uint8_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* rgb, int siting,
                                   void* stream) {
    pfnl::YuvCoef c;
    if (int r = yuv_op_refused(yuv, rgb, fmt, matrix, full_range, n, H, W, &c)) return r;
    if (int r = siting_refused(siting)) return r;
    HIPCHK(pfnl::launch_yuv420_to_rgb_u8(yuv, rgb, fmt == PFNL_PIX_NV12, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_yuv420_to_rgb_u8(const uint8_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* rgb, void* stream) {
    return pfnl_op_yuv420_to_rgb_u8_sited(yuv, fmt, matrix, full_range, n, H, W, rgb, PFNL_SITING_LEFT, stream);
}

int pfnl_op_yuv420_to_rgb_u8_surface_sited(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint8_t* rgb, int siting,
                                           void* stream) {
    pfnl::YuvCoef c;
    if (int r = yuv_op_refused(yuv, rgb, fmt, matrix, full_range, 1, H, W, &c)) return r;
    if (int r = siting_refused(siting)) return r;
    if (const char* why = pfnl::surface_refused(yuv, fmt, H, W)) return fail(PFNL_ERR_INVALID, why);
    HIPCHK(pfnl::launch_yuv420_planes_to_rgb_u8(pfnl_internal_yuv_planes(*yuv, fmt == PFNL_PIX_NV12), rgb, fmt == PFNL_PIX_NV12, c, 1, H, W,
                                                siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_yuv420_to_rgb_u8_surface(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint8_t* rgb, void* stream) {
    return pfnl_op_yuv420_to_rgb_u8_surface_sited(yuv, fmt, matrix, full_range, H, W, rgb, PFNL_SITING_LEFT, stream);
}

int pfnl_op_rgb_to_yuv420_u8_sited(const uint8_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* yuv, int siting,
                                   void* stream) {
    pfnl::YuvCoef c;
    if (int r = yuv_op_refused(rgb, yuv, fmt, matrix, full_range, n, H, W, &c)) return r;
    if (int r = siting_refused(siting)) return r;
    HIPCHK(pfnl::launch_rgb_to_yuv420(rgb, yuv, fmt == PFNL_PIX_NV12, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_rgb_to_yuv420_u8(const uint8_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* yuv, void* stream) {
    return pfnl_op_rgb_to_yuv420_u8_sited(rgb, fmt, matrix, full_range, n, H, W, yuv, PFNL_SITING_LEFT, stream);
}

int pfnl_yuv10_coefficients(int matrix, int full_range, int32_t out[10]) {
    if (!out) return fail(PFNL_ERR_INVALID, "NULL argument");
    pfnl::YuvCoef c;
    if (!pfnl::yuv_coefficients(10, matrix, full_range, &c)) return fail(PFNL_ERR_INVALID, "yuv10: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    const int v[10] = {c.y0, c.yr, c.yg, c.yb, c.cbr, c.cbg, c.cbb, c.crr, c.crg, c.crb};
    for (int k = 0; k < 10; ++k) out[k] = v[k];
    return 0;
}

int pfnl_op_quantise_u10(const float* sr, uint16_t* out, size_t n, void* stream) {
    if (!sr || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!n || n % 4) return fail(PFNL_ERR_INVALID, "element count must be a positive multiple of 4");
    if (reinterpret_cast<uintptr_t>(sr) % 16 || reinterpret_cast<uintptr_t>(out) % 8)
        return fail(PFNL_ERR_INVALID, "quantise_u10: sr must be 16-byte aligned and out 8-byte aligned");
    HIPCHK(pfnl::launch_quantise(sr, out, n, (hipStream_t)stream));
    return 0;
}

int pfnl_colour_matrix(int src, int dst, int32_t out[9]) {
    if (!out) return fail(PFNL_ERR_INVALID, "NULL argument");
    pfnl::ColourMatrix m;
    if (!pfnl::colour_matrix(src, dst, &m)) return fail(PFNL_ERR_INVALID, "colour: primaries PFNL_PRIM_BT709, PFNL_PRIM_BT601_525 or PFNL_PRIM_BT601_625");
    for (int k = 0; k < 9; ++k) out[k] = m.m[k];
    return 0;
}

int pfnl_colour_tables(int bits, uint16_t* decode, uint16_t* encode) {
    if (!decode || !encode) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!pfnl::colour_tables(bits, decode, encode)) return fail(PFNL_ERR_INVALID, "colour: bits 8 or 10");
    return 0;
}

// both depths: refused before any HIP call; then the one launch, on the device's tables
extern "C++" template <typename T>
static int quantise_colour_op(const float* sr, T* out, size_t pixels, int src, int dst, void* stream) {
    if (!sr || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!pixels || pixels % 4) return fail(PFNL_ERR_INVALID, "quantise_colour: the pixel count must be a positive multiple of 4");
    if (reinterpret_cast<uintptr_t>(sr) % 16 || reinterpret_cast<uintptr_t>(out) % 8)
        return fail(PFNL_ERR_INVALID, "quantise_colour: sr must be 16-byte aligned and out 8-byte aligned");
    pfnl::ColourMatrix m;
    if (!pfnl::colour_matrix(src, dst, &m)) return fail(PFNL_ERR_INVALID, "quantise_colour: primaries PFNL_PRIM_BT709, PFNL_PRIM_BT601_525 or PFNL_PRIM_BT601_625");
    if (src == dst) {                                 // no conversion: the plain stage 0
        HIPCHK(pfnl::launch_quantise(sr, out, 3 * pixels, (hipStream_t)stream));
        return 0;
    }
    const uint16_t *tab8 = nullptr, *tab10 = nullptr;
    HIPCHK(pfnl::colour_device_tables(&tab8, &tab10));
    HIPCHK(pfnl::launch_quantise_colour(sr, out, pixels, sizeof(T) == 2 ? tab10 : tab8, m, (hipStream_t)stream));
    return 0;
}

int pfnl_op_quantise_colour_u8(const float* sr, uint8_t* out, size_t pixels, int src, int dst, void* stream) {
    return quantise_colour_op(sr, out, pixels, src, dst, stream);
}

int pfnl_op_quantise_colour_u10(const float* sr, uint16_t* out, size_t pixels, int src, int dst, void* stream) {
    return quantise_colour_op(sr, out, pixels, src, dst, stream);
}

int pfnl_op_rgb_to_yuv420_u10(const uint16_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* yuv, void* stream) {
    return pfnl_op_rgb_to_yuv420_u10_sited(rgb, fmt, matrix, full_range, n, H, W, yuv, PFNL_SITING_LEFT, stream);
}

int pfnl_op_rgb_to_yuv420_u10_sited(const uint16_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* yuv, int siting,
                                    void* stream) {
    if (!rgb || !yuv) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (fmt != PFNL_PIX_P010 && fmt != PFNL_PIX_I010) return fail(PFNL_ERR_INVALID, "yuv10: fmt must be PFNL_PIX_P010 or PFNL_PIX_I010");
    pfnl::YuvCoef c;
    if (!pfnl::yuv_coefficients(10, matrix, full_range, &c)) return fail(PFNL_ERR_INVALID, "yuv10: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    if (n < 1 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "yuv10: n >= 1, H and W positive and even (4:2:0)");
    if ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(yuv)) % 2) return fail(PFNL_ERR_INVALID, "yuv10: uint16 samples are 2-byte aligned");
    if (int r = siting_refused(siting)) return r;
    HIPCHK(pfnl::launch_rgb_to_yuv420(rgb, yuv, fmt == PFNL_PIX_P010, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

// ---- 10 bits in: the op hooks of the 16-bit input edge -----------------------------------------------------------------------------------

int pfnl_yuv10_decode_coefficients(int matrix, int full_range, int32_t out[6]) {
    if (!out) return fail(PFNL_ERR_INVALID, "NULL argument");
    pfnl::YuvCoef c;
    if (!pfnl::yuv_coefficients(10, matrix, full_range, &c)) return fail(PFNL_ERR_INVALID, "yuv10: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    const int v[6] = {c.y0, c.dy, c.drv, c.dgu, c.dgv, c.dbu};
    for (int k = 0; k < 6; ++k) out[k] = v[k];
    return 0;
}

// as yuv_op_refused, for the two 16-bit 4:2:0 layouts
static int yuv10_op_refused(const void* a, const void* b, int fmt, int matrix, int full_range, int n, int H, int W, int siting, pfnl::YuvCoef* c) {
    if (!a || !b) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (fmt != PFNL_PIX_P010 && fmt != PFNL_PIX_I010) return fail(PFNL_ERR_INVALID, "yuv10: fmt must be PFNL_PIX_P010 or PFNL_PIX_I010");
    if (!pfnl::yuv_coefficients(10, matrix, full_range, c)) return fail(PFNL_ERR_INVALID, "yuv10: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    if (n < 1 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return fail(PFNL_ERR_INVALID, "yuv10: n >= 1, H and W positive and even (4:2:0)");
    return siting_refused(siting);
}

int pfnl_op_yuv420_to_rgb_u10_sited(const uint16_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* rgb, int siting,
                                    void* stream) {
    pfnl::YuvCoef c;
    if (int r = yuv10_op_refused(yuv, rgb, fmt, matrix, full_range, n, H, W, siting, &c)) return r;
    if ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(yuv)) % 2) return fail(PFNL_ERR_INVALID, "yuv10: uint16 samples are 2-byte aligned");
    HIPCHK(pfnl::launch_yuv420_to_rgb(yuv, rgb, fmt == PFNL_PIX_P010, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_yuv420_to_rgb_u10_surface_sited(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint16_t* rgb, int siting,
                                            void* stream) {
    pfnl::YuvCoef c;
    if (int r = yuv10_op_refused(yuv, rgb, fmt, matrix, full_range, 1, H, W, siting, &c)) return r;
    if (reinterpret_cast<uintptr_t>(rgb) % 2) return fail(PFNL_ERR_INVALID, "yuv10: uint16 samples are 2-byte aligned");
    if (const char* why = pfnl::surface_refused(yuv, fmt, H, W)) return fail(PFNL_ERR_INVALID, why);
    HIPCHK(pfnl::launch_yuv420_planes_to_rgb_u10(pfnl_internal_yuv_planes(*yuv, fmt == PFNL_PIX_P010), rgb, fmt == PFNL_PIX_P010, c, 1, H, W,
                                                 siting, (hipStream_t)stream));
    return 0;
}

// ---- 4:2:2 and 4:4:4: the _sited hooks with the subsampling named (include/pfnl_hip.h CHROMA FORMAT) ------------------------------------

// what the six hooks refuse before any HIP call at PFNL_CHROMA_422 / _444 (at _420 each is its _sited twin); *c = the table of `bits`
static int chroma_op_refused(const void* a, const void* b, int bits, int fmt, int matrix, int full_range, int n, int H, int W, int chroma,
                             int siting, pfnl::YuvCoef* c) {
    if (!a || !b) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (bits == 8 && fmt != PFNL_PIX_NV12 && fmt != PFNL_PIX_I420) return fail(PFNL_ERR_INVALID, "yuv: fmt must be PFNL_PIX_NV12 or PFNL_PIX_I420");
    if (bits == 10 && fmt != PFNL_PIX_P010 && fmt != PFNL_PIX_I010)
        return fail(PFNL_ERR_INVALID, "yuv10: fmt must be PFNL_PIX_P010 or PFNL_PIX_I010");
    if (!pfnl::yuv_coefficients(bits, matrix, full_range, c)) return fail(PFNL_ERR_INVALID, "yuv: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    if (n < 1 || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "yuv: n >= 1, H and W positive");
    if (chroma == PFNL_CHROMA_422 && (W & 1)) return fail(PFNL_ERR_INVALID, "yuv: W must be even (4:2:2)");
    return siting_refused(siting);
}

static int chroma_refused(int chroma) {
    if (chroma < PFNL_CHROMA_420 || chroma > PFNL_CHROMA_444)
        return fail(PFNL_ERR_INVALID, "yuv: chroma must be PFNL_CHROMA_420, PFNL_CHROMA_422 or PFNL_CHROMA_444");
    return 0;
}

static int aligned16_refused(const void* a, const void* b) {
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 2) return fail(PFNL_ERR_INVALID, "yuv10: uint16 samples are 2-byte aligned");
    return 0;
}

int pfnl_op_yuv_to_rgb_u8_chroma(const uint8_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* rgb, int chroma, int siting,
                                 void* stream) {
    if (int r = chroma_refused(chroma)) return r;
    if (chroma == PFNL_CHROMA_420) return pfnl_op_yuv420_to_rgb_u8_sited(yuv, fmt, matrix, full_range, n, H, W, rgb, siting, stream);
    pfnl::YuvCoef c;
    if (int r = chroma_op_refused(yuv, rgb, 8, fmt, matrix, full_range, n, H, W, chroma, siting, &c)) return r;
    HIPCHK(pfnl::launch_yuv_to_rgb_chroma(yuv, rgb, fmt == PFNL_PIX_NV12, c, n, H, W, chroma, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_yuv_to_rgb_u10_chroma(const uint16_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* rgb, int chroma,
                                  int siting, void* stream) {
    if (int r = chroma_refused(chroma)) return r;
    if (chroma == PFNL_CHROMA_420) return pfnl_op_yuv420_to_rgb_u10_sited(yuv, fmt, matrix, full_range, n, H, W, rgb, siting, stream);
    pfnl::YuvCoef c;
    if (int r = chroma_op_refused(yuv, rgb, 10, fmt, matrix, full_range, n, H, W, chroma, siting, &c)) return r;
    if (int r = aligned16_refused(yuv, rgb)) return r;
    HIPCHK(pfnl::launch_yuv_to_rgb_chroma(yuv, rgb, fmt == PFNL_PIX_P010, c, n, H, W, chroma, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_yuv_to_rgb_u8_surface_chroma(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint8_t* rgb, int chroma,
                                         int siting, void* stream) {
    if (int r = chroma_refused(chroma)) return r;
    if (chroma == PFNL_CHROMA_420) return pfnl_op_yuv420_to_rgb_u8_surface_sited(yuv, fmt, matrix, full_range, H, W, rgb, siting, stream);
    pfnl::YuvCoef c;
    if (int r = chroma_op_refused(yuv, rgb, 8, fmt, matrix, full_range, 1, H, W, chroma, siting, &c)) return r;
    if (const char* why = pfnl::surface_refused(yuv, fmt, H, W, chroma)) return fail(PFNL_ERR_INVALID, why);
    HIPCHK(pfnl::launch_yuv_planes_to_rgb_chroma(pfnl_internal_yuv_planes(*yuv, fmt == PFNL_PIX_NV12), rgb, fmt == PFNL_PIX_NV12, c, 1, H, W, chroma,
                                                 siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_yuv_to_rgb_u10_surface_chroma(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint16_t* rgb, int chroma,
                                          int siting, void* stream) {
    if (int r = chroma_refused(chroma)) return r;
    if (chroma == PFNL_CHROMA_420) return pfnl_op_yuv420_to_rgb_u10_surface_sited(yuv, fmt, matrix, full_range, H, W, rgb, siting, stream);
    pfnl::YuvCoef c;
    if (int r = chroma_op_refused(yuv, rgb, 10, fmt, matrix, full_range, 1, H, W, chroma, siting, &c)) return r;
    if (int r = aligned16_refused(rgb, nullptr)) return r;
    if (const char* why = pfnl::surface_refused(yuv, fmt, H, W, chroma)) return fail(PFNL_ERR_INVALID, why);
    HIPCHK(pfnl::launch_yuv_planes_to_rgb_chroma(pfnl_internal_yuv_planes(*yuv, fmt == PFNL_PIX_P010), rgb, fmt == PFNL_PIX_P010, c, 1, H, W, chroma,
                                                 siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_rgb_to_yuv_u8_chroma(const uint8_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* yuv, int chroma, int siting,
                                 void* stream) {
    if (int r = chroma_refused(chroma)) return r;
    if (chroma == PFNL_CHROMA_420) return pfnl_op_rgb_to_yuv420_u8_sited(rgb, fmt, matrix, full_range, n, H, W, yuv, siting, stream);
    pfnl::YuvCoef c;
    if (int r = chroma_op_refused(rgb, yuv, 8, fmt, matrix, full_range, n, H, W, chroma, siting, &c)) return r;
    HIPCHK(pfnl::launch_rgb_to_yuv_chroma(rgb, yuv, fmt == PFNL_PIX_NV12, c, n, H, W, chroma, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_rgb_to_yuv_u10_chroma(const uint16_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* yuv, int chroma,
                                  int siting, void* stream) {
    if (int r = chroma_refused(chroma)) return r;
    if (chroma == PFNL_CHROMA_420) return pfnl_op_rgb_to_yuv420_u10_sited(rgb, fmt, matrix, full_range, n, H, W, yuv, siting, stream);
    pfnl::YuvCoef c;
    if (int r = chroma_op_refused(rgb, yuv, 10, fmt, matrix, full_range, n, H, W, chroma, siting, &c)) return r;
    if (int r = aligned16_refused(rgb, yuv)) return r;
    HIPCHK(pfnl::launch_rgb_to_yuv_chroma(rgb, yuv, fmt == PFNL_PIX_P010, c, n, H, W, chroma, siting, (hipStream_t)stream));
    return 0;
}

// ---- packed formats: the two kernels on one plane with a pitch (include/pfnl_hip.h PACKED FORMATS; pack_geom.h states the table) -------

// what the four hooks refuse before any HIP call; *c = the table of `bits`
static int packed_op_refused(const void* plane, size_t pitch, int pack, int bits, int matrix, int full_range, int siting, int n, size_t frame_stride,
                             int H, int W, const void* rgb, pfnl::YuvCoef* c) {
    if (!plane || !rgb) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (!pfnl::is_packing(pack)) return fail(PFNL_ERR_INVALID, "packed: pack must be PFNL_PACK_BGR24 .. PFNL_PACK_V210");
    if (n < 1 || H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "packed: n >= 1, H and W positive");
    const pfnl::PackInfo& p = pfnl::PACK_TABLE[pack];
    if (const char* why = pfnl::pack_refused(pack, p.yuv, bits, PFNL_CHROMA_422, W)) return fail(PFNL_ERR_INVALID, why);
    if (!pfnl::yuv_coefficients(bits, matrix, full_range, c)) return fail(PFNL_ERR_INVALID, "packed: matrix 0 (BT.601) or 1 (BT.709), full_range 0 or 1");
    if (int r = siting_refused(siting)) return r;
    const size_t row = pfnl::pack_row_bytes(pack, W);
    if (pitch < row) return fail(PFNL_ERR_INVALID, "packed: the pitch is smaller than the bytes of a row");
    if (n > 1 && frame_stride < (size_t)(H - 1) * pitch + row) return fail(PFNL_ERR_INVALID, "packed: the frame stride is smaller than the rows of a frame");
    if ((reinterpret_cast<uintptr_t>(plane) | pitch | (n > 1 ? frame_stride : 0)) % p.align)
        return fail(PFNL_ERR_INVALID, "packed: plane pointer, pitch and frame stride must be multiples of 2 (y210) or 4 (x2rgb10, x2bgr10, v210)");
    if (bits == 10 && reinterpret_cast<uintptr_t>(rgb) % 2) return fail(PFNL_ERR_INVALID, "packed: uint16 samples are 2-byte aligned");
    return 0;
}

int pfnl_op_packed_to_rgb_u8(const void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H,
                             int W, uint8_t* rgb, void* stream) {
    pfnl::YuvCoef c;
    if (int r = packed_op_refused(plane, pitch, pack, 8, matrix, full_range, siting, n, frame_stride, H, W, rgb, &c)) return r;
    HIPCHK(pfnl::launch_packed_to_rgb(plane, pitch, frame_stride, pack, rgb, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_packed_to_rgb_u10(const void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H,
                              int W, uint16_t* rgb, void* stream) {
    pfnl::YuvCoef c;
    if (int r = packed_op_refused(plane, pitch, pack, 10, matrix, full_range, siting, n, frame_stride, H, W, rgb, &c)) return r;
    HIPCHK(pfnl::launch_packed_to_rgb(plane, pitch, frame_stride, pack, rgb, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_rgb_to_packed_u8(void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H, int W,
                             const uint8_t* rgb, void* stream) {
    pfnl::YuvCoef c;
    if (int r = packed_op_refused(plane, pitch, pack, 8, matrix, full_range, siting, n, frame_stride, H, W, rgb, &c)) return r;
    HIPCHK(pfnl::launch_rgb_to_packed(rgb, plane, pitch, frame_stride, pack, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

int pfnl_op_rgb_to_packed_u10(void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H, int W,
                              const uint16_t* rgb, void* stream) {
    pfnl::YuvCoef c;
    if (int r = packed_op_refused(plane, pitch, pack, 10, matrix, full_range, siting, n, frame_stride, H, W, rgb, &c)) return r;
    HIPCHK(pfnl::launch_rgb_to_packed(rgb, plane, pitch, frame_stride, pack, c, n, H, W, siting, (hipStream_t)stream));
    return 0;
}

// ---- interlaced input: the deinterlacer on five decoded fields (include/pfnl_hip.h INTERLACED; deinterlace.hip) -------
static int deinterlace_op_refused(const void* p2, const void* p1, const void* cur, const void* n1, const void* n2, int H, int W, int parity,
                                  const void* out, int sample_bytes) {
    const void* const ptr[6] = {p2, p1, cur, n1, n2, out};
    const char* const name[6] = {"p2", "p1", "cur", "n1", "n2", "out"};
    for (int k = 0; k < 6; ++k) {
        if (!ptr[k]) return fail(PFNL_ERR_INVALID, std::string("deinterlace: ") + name[k] + " is NULL");
        if (reinterpret_cast<uintptr_t>(ptr[k]) % sample_bytes) return fail(PFNL_ERR_INVALID, std::string("deinterlace: ") + name[k] + ": uint16 samples are 2-byte aligned");
    }
    if (H < 2 || (H & 1)) return fail(PFNL_ERR_INVALID, "deinterlace: H must be even and at least 2");
    if (W < 1) return fail(PFNL_ERR_INVALID, "deinterlace: W must be at least 1");
    if (parity != 0 && parity != 1) return fail(PFNL_ERR_INVALID, "deinterlace: parity is 0 (cur is the top field) or 1");
    return 0;
}

int pfnl_op_deinterlace_u8(const uint8_t* p2, const uint8_t* p1, const uint8_t* cur, const uint8_t* n1, const uint8_t* n2, int H, int W, int parity,
                           uint8_t* out, void* stream) {
    if (int r = deinterlace_op_refused(p2, p1, cur, n1, n2, H, W, parity, out, 1)) return r;
    HIPCHK(pfnl::launch_deinterlace(p2, p1, cur, n1, n2, H, W, parity, out, (hipStream_t)stream));
    return 0;
}

int pfnl_op_deinterlace_u10(const uint16_t* p2, const uint16_t* p1, const uint16_t* cur, const uint16_t* n1, const uint16_t* n2, int H, int W,
                            int parity, uint16_t* out, void* stream) {
    if (int r = deinterlace_op_refused(p2, p1, cur, n1, n2, H, W, parity, out, 2)) return r;
    HIPCHK(pfnl::launch_deinterlace(p2, p1, cur, n1, n2, H, W, parity, out, (hipStream_t)stream));
    return 0;
}

extern "C++" template <typename T>
static int op_deinterlace_pair(const T* const fields[6], int H, int W, int parity, T* out, void* stream) {
    if (!fields) return fail(PFNL_ERR_INVALID, "deinterlace: fields is NULL");
    for (int k = 0; k < 6; ++k) {
        if (!fields[k]) return fail(PFNL_ERR_INVALID, "deinterlace: fields[" + std::to_string(k) + "] is NULL");
        if (reinterpret_cast<uintptr_t>(fields[k]) % sizeof(T)) return fail(PFNL_ERR_INVALID, "deinterlace: fields[" + std::to_string(k) + "]: uint16 samples are 2-byte aligned");
    }
    if (int r = deinterlace_op_refused(fields[0], fields[1], fields[2], fields[3], fields[4], H, W, parity, out, (int)sizeof(T))) return r;
    const pfnl::DeinterlaceJob<T> jobs[2] = {{fields[0], fields[1], fields[2], fields[3], fields[4], out, parity},
                                             {fields[1], fields[2], fields[3], fields[4], fields[5], out + (size_t)H * W * 3, 1 - parity}};
    HIPCHK(pfnl::launch_deinterlace(jobs, 2, H, W, (hipStream_t)stream));
    return 0;
}

int pfnl_op_deinterlace_pair_u8(const uint8_t* const fields[6], int H, int W, int parity, uint8_t* out, void* stream) {
    return op_deinterlace_pair(fields, H, W, parity, out, stream);
}

int pfnl_op_deinterlace_pair_u10(const uint16_t* const fields[6], int H, int W, int parity, uint16_t* out, void* stream) {
    return op_deinterlace_pair(fields, H, W, parity, out, stream);
}

// ---- inverse telecine: the match and the weave on three decoded fields (include/pfnl_hip.h TELECINE; telecine.hip) -------
// what both hooks refuse before any HIP call; *q: the parameters with the defaults filled in
static int telecine_op_refused(const void* A, const void* Xc, const void* Xp, int h, int W, int parity, const pfnl_telecine_params* params,
                               const void* out, const void* words_dev, int sample_bytes, pfnl_telecine_params* q) {
    const void* const ptr[5] = {A, Xc, Xp, out, words_dev};
    const char* const name[5] = {"A", "Xc", "Xp", "out", "the device words"};
    for (int k = 0; k < 5; ++k) {
        if (!ptr[k]) return fail(PFNL_ERR_INVALID, std::string("telecine: ") + name[k] + " is NULL");
        if (k < 4 && reinterpret_cast<uintptr_t>(ptr[k]) % sample_bytes) return fail(PFNL_ERR_INVALID, std::string("telecine: ") + name[k] + ": uint16 samples are 2-byte aligned");
    }
    if (reinterpret_cast<uintptr_t>(words_dev) % 8) return fail(PFNL_ERR_INVALID, "telecine: the device words must be 8-byte aligned");
    if (h < 1) return fail(PFNL_ERR_INVALID, "telecine: h must be at least 1");
    if (W < 1) return fail(PFNL_ERR_INVALID, "telecine: W must be at least 1");
    if ((unsigned long long)h * 3ull * (unsigned long long)W >= (1ull << 32)) return fail(PFNL_ERR_INVALID, "telecine: h 3 W must be below 2^32");
    if (parity != 0 && parity != 1) return fail(PFNL_ERR_INVALID, "telecine: parity is 0 (A is the top field) or 1");
    if (const char* why = pfnl::telecine_params_refused(params, h, W, q)) return fail(PFNL_ERR_INVALID, why);
    return 0;
}

extern "C++" template <typename T>
static int op_fieldmatch(const T* A, const T* Xc, const T* Xp, int h, int W, int parity, int threshold, unsigned long long* counts_dev, void* stream) {
    const pfnl_telecine_params given{threshold, 0, 0};
    pfnl_telecine_params q;
    if (int r = telecine_op_refused(A, Xc, Xp, h, W, parity, &given, A, counts_dev, (int)sizeof(T), &q)) return r;
    OpStage st(stream);
    unsigned long long* words = st.alloc<unsigned long long>(6);      // scratch [2] | decision [4]
    st.run([&] { return hipMemsetAsync(words, 0, 6 * sizeof(unsigned long long), st.s); });
    st.run([&] { return pfnl::launch_telecine_match(A, Xc, Xp, h, W, parity, threshold, words, pfnl::TelecineDecide{words + 2, nullptr, 0, 0}, st.s); });
    st.run([&] { return hipMemcpyAsync(counts_dev, words + 2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st.s); });
    return st.finish("fieldmatch op: ");
}

extern "C++" template <typename T>
static int op_telecine_frame(const T* A, const T* Xc, const T* Xp, int h, int W, int parity, const pfnl_telecine_params* params, T* out,
                             unsigned long long* decision_dev, void* stream) {
    pfnl_telecine_params q;
    if (int r = telecine_op_refused(A, Xc, Xp, h, W, parity, params, out, decision_dev, (int)sizeof(T), &q)) return r;
    const uintptr_t field = (uintptr_t)h * W * 3 * sizeof(T), o = reinterpret_cast<uintptr_t>(out);
    for (const T* f : {A, Xc, Xp})
        if (reinterpret_cast<uintptr_t>(f) < o + 2 * field && o < reinterpret_cast<uintptr_t>(f) + field)
            return fail(PFNL_ERR_INVALID, "telecine: out overlaps one of the fields");
    // the two launches a session issues per matched frame, and nothing else: the scratch is the caller's (words 4, 5; zero between launches)
    HIPCHK(pfnl::launch_telecine_match(A, Xc, Xp, h, W, parity, q.threshold, decision_dev + 4,
                                       pfnl::TelecineDecide{decision_dev, nullptr, q.post, (unsigned long long)q.comb_limit}, (hipStream_t)stream));
    HIPCHK(pfnl::launch_telecine_weave(A, Xc, Xp, h, W, parity, decision_dev, out, nullptr, nullptr, nullptr, (hipStream_t)stream));
    return 0;
}

int pfnl_op_fieldmatch_u8(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, int threshold,
                          unsigned long long* counts_dev, void* stream) {
    return op_fieldmatch(A, Xc, Xp, h, W, parity, threshold, counts_dev, stream);
}

int pfnl_op_fieldmatch_u10(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity, int threshold,
                           unsigned long long* counts_dev, void* stream) {
    return op_fieldmatch(A, Xc, Xp, h, W, parity, threshold, counts_dev, stream);
}

int pfnl_op_telecine_frame_u8(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, const pfnl_telecine_params* params,
                              uint8_t* out, unsigned long long* decision_dev, void* stream) {
    return op_telecine_frame(A, Xc, Xp, h, W, parity, params, out, decision_dev, stream);
}

int pfnl_op_telecine_frame_u10(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity,
                               const pfnl_telecine_params* params, uint16_t* out, unsigned long long* decision_dev, void* stream) {
    return op_telecine_frame(A, Xc, Xp, h, W, parity, params, out, decision_dev, stream);
}

// as pfnl_op_gather_windows_u8: what both gathers refuse before any HIP call (scene_first: null for the plain one)
static int gather_u10_refused(const uint16_t* ring, const long long* scene_first, const float* win, int cap, long long last, long long first,
                              int count, int T, int H, int W) {
    if (cap < 1 || last < 0 || first < 0 || count < 1 || T < 1 || !(T & 1) || H < 1 || W < 1 || ((size_t)H * W * 3) % 2)
        return fail(PFNL_ERR_INVALID, "bad window geometry (H*W*3 must be even, T odd, cap >= 1, first, last >= 0)");
    if (first + count - 1 > last) return fail(PFNL_ERR_INVALID, "a window's centre frame lies beyond `last`");
    if (reinterpret_cast<uintptr_t>(ring) % 4 || reinterpret_cast<uintptr_t>(win) % 16 || reinterpret_cast<uintptr_t>(scene_first) % 8)
        return fail(PFNL_ERR_INVALID, "ring must be 4-byte aligned, scene_first 8-byte and win 16-byte aligned");
    const long long lo = first - T / 2 < 0 ? 0 : first - T / 2, hi = first + count - 1 + T / 2 > last ? last : first + count - 1 + T / 2;
    if (hi - lo + 1 > cap) return fail(PFNL_ERR_INVALID, "the windows span more frames than the ring holds");
    return 0;
}

int pfnl_op_gather_windows_u10(const uint16_t* ring, float* win, int cap, long long last, long long first, int count, int T, int H, int W,
                               void* stream) {
    if (!ring || !win) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (int r = gather_u10_refused(ring, nullptr, win, cap, last, first, count, T, H, W)) return r;
    HIPCHK(pfnl::launch_gather_windows_u10(ring, win, cap, last, first, count, T, (size_t)H * W * 6, (hipStream_t)stream));
    return 0;
}

int pfnl_op_gather_windows_u10_scenes(const uint16_t* ring, const long long* scene_first_dev, float* win, int cap, long long last, long long first,
                                      int count, int T, int H, int W, void* stream) {
    if (!ring || !scene_first_dev || !win) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (int r = gather_u10_refused(ring, scene_first_dev, win, cap, last, first, count, T, H, W)) return r;
    HIPCHK(pfnl::launch_gather_windows_u10_scenes(ring, scene_first_dev, win, cap, last, first, count, T, (size_t)H * W * 6, (hipStream_t)stream));
    return 0;
}

int pfnl_op_scene_sad_u10(const uint16_t* a, const uint16_t* b, int H, int W, unsigned long long* out_dev, void* stream) {
    if (!a || !b || !out_dev) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (H < 1 || W < 1) return fail(PFNL_ERR_INVALID, "H and W must be positive");
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 2) return fail(PFNL_ERR_INVALID, "scene sad: uint16 samples are 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(out_dev) % 8) return fail(PFNL_ERR_INVALID, "out_dev must be 8-byte aligned");
    OpStage st(stream);
    unsigned long long* scratch = st.alloc<unsigned long long>(2);
    st.run([&] { return hipMemsetAsync(scratch, 0, 2 * sizeof(unsigned long long), st.s); });
    st.run([&] { return pfnl::launch_scene_sad_u10(a, b, (size_t)H * W, scratch, pfnl::SceneDecision{out_dev, nullptr, 0, 0, 0, 0, 0, 0}, st.s); });
    return st.finish("scene sad op: ");
}

int pfnl_op_content_box_u8(const uint8_t* frames, int n, int H, int W, int limit, int32_t* box_dev, uint32_t* rows_dev, uint32_t* cols_dev,
                           void* stream) {
    return op_content_box<uint8_t>(frames, n, H, W, limit, box_dev, rows_dev, cols_dev, stream);
}

int pfnl_op_content_box_u10(const uint16_t* frames, int n, int H, int W, int limit, int32_t* box_dev, uint32_t* rows_dev, uint32_t* cols_dev,
                            void* stream) {
    return op_content_box<uint16_t>(frames, n, H, W, limit, box_dev, rows_dev, cols_dev, stream);
}

int pfnl_op_resize_u10(const uint16_t* in, int n, int H, int W, int oH, int oW, uint16_t* out, void* stream) {
    if (!in || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (n < 1) return fail(PFNL_ERR_INVALID, "resize: n >= 1");
    pfnl::PlacePlan plan;                             // the whole raster on the whole canvas
    std::string why;
    if (!pfnl::place_plan(H, W, oH, oW, nullptr, nullptr, &plan, &why)) return fail(PFNL_ERR_INVALID, why);
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 2) return fail(PFNL_ERR_INVALID, "resize: uint16 samples are 2-byte aligned");
    const uint16_t black[3] = {0, 0, 0};
    OpStage st(stream);
    const int32_t* blob = st.upload(plan.r.blob);
    st.run([&] { return pfnl::launch_resize_place(in, out, plan, blob, black, n, st.s); });
    return st.finish("resize10 op: ");
}

int pfnl_resize_max_taps(int n_in, int n_out, int* ntaps) {
    if (!ntaps) return fail(PFNL_ERR_INVALID, "NULL argument");
    pfnl::ResizeAxis t;
    std::string why;
    if (!pfnl::resize_axis(n_in, n_out, &t, &why)) return fail(PFNL_ERR_INVALID, why);
    *ntaps = t.ntaps;
    return 0;
}

int pfnl_resize_taps(int n_in, int n_out, int32_t* first, int32_t* count, int16_t* coef) {
    if (!first || !count || !coef) return fail(PFNL_ERR_INVALID, "NULL argument");
    pfnl::ResizeAxis t;
    std::string why;
    if (!pfnl::resize_axis(n_in, n_out, &t, &why)) return fail(PFNL_ERR_INVALID, why);
    std::memcpy(first, t.first.data(), t.first.size() * sizeof(int32_t));
    std::memcpy(count, t.count.data(), t.count.size() * sizeof(int32_t));
    std::memcpy(coef, t.coef.data(), t.coef.size() * sizeof(int16_t));
    return 0;
}

int pfnl_op_resize_u8(const uint8_t* in, int n, int H, int W, int oH, int oW, uint8_t* out, void* stream) {
    if (!in || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (n < 1) return fail(PFNL_ERR_INVALID, "resize: n >= 1");
    pfnl::PlacePlan plan;                             // the whole raster on the whole canvas
    std::string why;
    if (!pfnl::place_plan(H, W, oH, oW, nullptr, nullptr, &plan, &why)) return fail(PFNL_ERR_INVALID, why);
    OpStage st(stream);
    const int32_t* blob = st.upload(plan.r.blob);
    st.run([&] { return pfnl::launch_resize_place(in, out, plan, blob, plan.fill, n, st.s); });
    return st.finish("resize op: ");
}

// both placement hooks: everything that needs no device (place_plan asks place_refused of stream_route.h, as the session does)
static int place_op_refused(const void* in, int n, int H, int W, int oH, int oW, const pfnl_rect* src, const pfnl_rect* dst, const void* out,
                            pfnl::PlacePlan* plan) {
    if (!in || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (n < 1) return fail(PFNL_ERR_INVALID, "place: n >= 1");
    std::string why;
    if (!pfnl::place_plan(H, W, oH, oW, src, dst, plan, &why)) return fail(PFNL_ERR_INVALID, why);
    return 0;
}

int pfnl_op_resize_place_u8(const uint8_t* in, int n, int H, int W, int oH, int oW, const pfnl_rect* src, const pfnl_rect* dst,
                            const uint8_t fill[3], uint8_t* out, void* stream) {
    pfnl::PlacePlan plan;
    if (int r = place_op_refused(in, n, H, W, oH, oW, src, dst, out, &plan)) return r;
    const uint8_t black[3] = {0, 0, 0};
    OpStage st(stream);
    const int32_t* blob = st.upload(plan.r.blob);
    st.run([&] { return pfnl::launch_resize_place(in, out, plan, blob, fill ? fill : black, n, st.s); });
    return st.finish("place op: ");
}

int pfnl_op_resize_place_u10(const uint16_t* in, int n, int H, int W, int oH, int oW, const pfnl_rect* src, const pfnl_rect* dst,
                             const uint16_t fill[3], uint16_t* out, void* stream) {
    pfnl::PlacePlan plan;
    if (int r = place_op_refused(in, n, H, W, oH, oW, src, dst, out, &plan)) return r;
    if (fill && (fill[0] > 1023 || fill[1] > 1023 || fill[2] > 1023)) return fail(PFNL_ERR_INVALID, "place: fill holds 10-bit sample values, 0 .. 1023");
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 2) return fail(PFNL_ERR_INVALID, "place: uint16 samples are 2-byte aligned");
    const uint16_t black[3] = {0, 0, 0};
    OpStage st(stream);
    const int32_t* blob = st.upload(plan.r.blob);
    st.run([&] { return pfnl::launch_resize_place(in, out, plan, blob, fill ? fill : black, n, st.s); });
    return st.finish("place10 op: ");
}

// every refusal comes before any HIP call: the argument checks work without a device
static int score_geometry_refused(int F, int H, int W) {
    if (F < 1 || F > 65535) return fail(PFNL_ERR_INVALID, "score: F must be in 1 .. 65535");
    if (H < 11 || W < 11) return fail(PFNL_ERR_INVALID, "score: H and W must be at least 11 (the 11x11 SSIM window)");
    if (H > 65536 || W > 65536) return fail(PFNL_ERR_INVALID, "score: H and W must be at most 65536");
    return 0;
}

int pfnl_op_score_scratch_bytes(int F, int H, int W, size_t* bytes) {
    if (!bytes) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (int r = score_geometry_refused(F, H, W)) return r;
    *bytes = pfnl::score_scratch_bytes(F, H, W);
    return 0;
}

int pfnl_op_score_y(const uint8_t* pred, const uint8_t* truth, int F, int H, int W, int sp_border, double* out, void* scratch,
                    void* stream) {
    if (!pred || !truth || !out || !scratch) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (int r = score_geometry_refused(F, H, W)) return r;
    if (sp_border < 0 || 2 * (long long)sp_border >= H || 2 * (long long)sp_border >= W)
        return fail(PFNL_ERR_INVALID, "score: sp_border must leave a crop (0 <= 2 * sp_border < H, W)");
    HIPCHK(pfnl::launch_score_y(pred, truth, F, H, W, sp_border, out, static_cast<double*>(scratch), (hipStream_t)stream));
    return 0;
}

// as below: refused before any HIP call
static int dihedral_op_refused(const void* a, const void* b, int n_img, int H, int W, int k) {
    if (!a || !b) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (k < 0 || k > 7) return fail(PFNL_ERR_INVALID, "dihedral: member k must lie in 0 .. 7");
    if (n_img < 1 || H <= 0 || W <= 0) return fail(PFNL_ERR_INVALID, "dihedral: n_img, H and W must be positive");
    return 0;
}

int pfnl_op_dihedral(const float* in, float* out, int n_img, int H, int W, int k, float scale, void* stream) {
    if (int r = dihedral_op_refused(in, out, n_img, H, W, k)) return r;
    HIPCHK(pfnl::launch_dihedral(in, out, n_img, H, W, k, scale, (hipStream_t)stream));
    return 0;
}

int pfnl_op_dihedral_accum(float* acc, const float* y, int n_img, int H, int W, int k, float scale, void* stream) {
    if (int r = dihedral_op_refused(acc, y, n_img, H, W, k)) return r;
    HIPCHK(pfnl::launch_dihedral_accum(acc, y, n_img, H, W, k, scale, (hipStream_t)stream));
    return 0;
}

// as above: refused before any HIP call; the grid of a call that passed
static int tile_op_refused(const void* a, const void* b, int B, int H, int W, const pfnl_tiling* t, int first, int count, pfnl::TileGrid* g) {
    if (!a || !b || !t) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (B < 1) return fail(PFNL_ERR_INVALID, "tile: B must be positive");
    if (const char* why = pfnl::tiling_refused(H, W, *t)) return fail(PFNL_ERR_INVALID, why);
    *g = pfnl::tile_grid(H, W, *t);
    const int total = pfnl::tile_total(*g, B);
    if (!total) return fail(PFNL_ERR_INVALID, "tile: the tile count overflows a 32-bit integer");
    if (first < 0 || count < 1 || count > total - first) return fail(PFNL_ERR_INVALID, "tile: first .. first + count - 1 must be tiles of the call");
    return 0;
}

int pfnl_op_tile_gather(const float* in, float* tiles, int B, int T, int H, int W, const pfnl_tiling* t, int first, int count, void* stream) {
    pfnl::TileGrid g;
    if (int r = tile_op_refused(in, tiles, B, H, W, t, first, count, &g)) return r;
    if (T < 1) return fail(PFNL_ERR_INVALID, "tile: T must be positive");
    HIPCHK(pfnl::launch_tile_gather(in, tiles, g, T, first, count, (hipStream_t)stream));
    return 0;
}

int pfnl_op_tile_scatter(const float* y, float* out, int B, int H, int W, int scale, const pfnl_tiling* t, int first, int count, void* stream) {
    pfnl::TileGrid g;
    if (int r = tile_op_refused(y, out, B, H, W, t, first, count, &g)) return r;
    if (scale < 1 || scale > 8) return fail(PFNL_ERR_INVALID, "tile: scale must lie in 1 .. 8");
    HIPCHK(pfnl::launch_tile_scatter(y, out, g, scale, first, count, (hipStream_t)stream));
    return 0;
}

int pfnl_op_bicubic(const float* x, float* out, int B, int H, int W, int scale, void* stream) {
    if (!x || !out) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (B < 1 || H < 1 || W < 1 || (scale != 2 && scale != 4)) return fail(PFNL_ERR_INVALID, "bad bicubic geometry");
    HIPCHK(pfnl::launch_bicubic(x, out, B, H, W, scale, (hipStream_t)stream));
    return 0;
}

int pfnl_op_blur_decimate(const float* hr, float* lr, int F, int H, int W, int scale, void* stream) {
    if (!hr || !lr) return fail(PFNL_ERR_INVALID, "NULL argument");
    if (F < 1 || H < 7 || W < 7 || (scale != 2 && scale != 4))
        return fail(PFNL_ERR_INVALID, "blur_decimate needs H, W >= 7 (reflect pad 6) and scale 2 or 4");
    HIPCHK(pfnl::launch_blur_decimate(hr, lr, F, H, W, scale, (hipStream_t)stream));
    return 0;
}

int pfnl_selftest_mfma(int device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PFNL_ERR_NODEVICE, "no HIP device visible");
    HIPCHK(hipSetDevice(device_id));
    int bad = -1;
    HIPCHK(pfnl::run_mfma_selftest(&bad));
    if (bad != 0) return fail(PFNL_ERR_STATE, "MFMA fragment layout mismatch: " + std::to_string(bad) + " elements");
    return 0;
}

}  // extern "C"
