// Shared declarations of libpfnl_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/pfnl_hip.h"   // pfnl_rect
#include "chain_order.h"   // persistent_grid: the grid of the persistent launches

namespace pfnl {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_32x32x2_f32: D[32x32] += A[32x2] * B[2x32], exact f32 (fmaf chain), 64 cycles/SIMD.
// Fragment maps (cdna_hip_programming.md §3): lane l holds A[i=l&31][k=l>>5], B[k=l>>5][j=l&31];
// D register r of lane l is D[i=(r&3)+8*(r>>2)+4*(l>>5)][j=l&31].
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int drow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// 16-byte buffer store that is safe to follow with anything.  Measured on gfx950 (tools/GFX950_NOTES.md, "store data"): a
// buffer_store_dwordx4 whose soffset is an SGPR still reads its data registers for a cycle or two after issue, this compiler's
// hazard recognizer knows the hazard only for the immediate-offset forms, and a VALU write to one of the registers in the next
// issue slot reached it first - one corrupted dword in 16 lanes, once in ~10^5 stores.  The s_nop takes the stored registers as
// INPUTS: they stay live up to it, so nothing the scheduler puts in between can write them.  tools/lint_store_hazard.py checks
// the emitted assembly of every kernel for the pattern.
typedef unsigned pfnl_u32x4 __attribute__((ext_vector_type(4)));
template <int AUX = 0>                                              // AUX: the cache-policy bits of the instruction (gfx940+: 1 sc0, 2 nt, 16 sc1)
__device__ __forceinline__ void buffer_store_b128_guarded(pfnl_u32x4 v, __amdgpu_buffer_rsrc_t rs, int voffset, int soffset) {
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, voffset, soffset, AUX);
    asm volatile("s_nop 1" ::"v"(v));
}

// Launch-time facts that are per DEVICE.  One process may drive several devices from several host threads (pfnl_comm_init_all, one
// handle per device): the launchers' lazy caches are indexed by the device and their slots are std::atomic, so a first launch
// racing with another thread's is a repeated, identical initialisation - not a data race, and never another device's CU count.
inline int device_cu_count() {                                      // CUs of the CURRENT device (0: it cannot be queried)
    static std::atomic<int> ncu[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int n = ncu[dev].load(std::memory_order_relaxed);
    if (!n) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 0;
        ncu[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// Graph capture against blocking copies, process-wide (DESIGN.md "What handles share").  Measured on HIP 7.2: while ANY host thread
// holds a stream capture open - hipStreamCaptureModeThreadLocal, on a blocking or on a non-blocking stream alike - another thread's
// hipMemcpy / hipMemcpyToSymbol returns hipErrorStreamCaptureImplicit AND invalidates that capture (hipStreamEndCapture:
// hipErrorStreamCaptureInvalidated).  Launches, asynchronous copies on a stream, hipMalloc / hipFree, hipHostMalloc and
// hipStreamSynchronize(NULL) are accepted.  So pfnl_forward captures under CaptureGuard (exclusive) and every blocking copy of the
// library is made under BlockingCopyGuard (shared): the two never overlap, whatever handles and threads they belong to.  Nothing on a
// forward's path takes either lock unless it captures (graph=on / auto).  Not recursive: no blocking copy inside a capture.
inline std::shared_mutex& capture_mutex() {
    static std::shared_mutex m;
    return m;
}
struct CaptureGuard {
    std::unique_lock<std::shared_mutex> lk{capture_mutex()};
};
struct BlockingCopyGuard {
    std::shared_lock<std::shared_mutex> lk{capture_mutex()};
};

__device__ __forceinline__ float lrelu(float v) { return fmaxf(v, 0.2f * v); }  // tf.nn.leaky_relu

// ---- MFMA implicit-GEMM convolution (conv_mfma.hip) ------------------------------------------
// Output tile of one workgroup: 8 rows x 32 columns x 64 output channels of one item.
constexpr int CONV_TW = 32;
constexpr int CONV_TH = 8;        // rows per workgroup at MT = 2 (conv_mfma.hip)
constexpr int CONV_CK = 16;       // input channels per K-chunk of the 3x3 kernel (conv_ck(): 32 for 1x1)
constexpr int CONV_NPAD = 64;     // output channels are padded to 64 in the packed weights

struct ConvParams {
    const float* in;       // [items*frames_per_item][H][W][in_cstride]
    const float* wpack;    // [nchunks][ks*ks][CONV_CK][64]
    const float* bias;     // [64] (zero padded); never null (use a zero vector)
    const float* addend;   // [items/add_div][H][W][64]  (added before the activation) \ both or
    const float* resid;    // [items][H][W][out_cstride] (added after the activation)  / neither
    float* out;            // [items][H][W][out_cstride]
    int H, W;
    int in_cstride;        // floats per input pixel (64)
    int out_cstride;       // floats per output pixel (= cout)
    int cout;              // valid output channels (<= 64)
    int chunks_per_frame;  // in_cstride / CONV_CK
    int frames_per_item;   // 1: per-frame conv; T: conv over the concat of T frames
    int nchunks;           // frames_per_item * chunks_per_frame
    int add_div;           // addend item = item / add_div
    int act;               // 1 = leaky_relu(0.2)
};

hipError_t launch_conv_mfma(const ConvParams& p, int ksize, int items, hipStream_t s);
int conv_ck(int ksize);
size_t conv_pack_floats(int ksize, int cin);                 // floats in the packed weight blob
// HWIO [k,k,cin_total,cout] rows [cin_begin, cin_begin+cin) -> [chunk][tap][CK][64]
void conv_pack_weights(const float* hwio, int ksize, int cin_total, int cin_begin, int cin,
                       int cout, float* dst);

// ---- fused Winograd F(2x2,3x3) 64->64 convolution (conv_wino.hip) -------------------------------
// conv10_i: streaming 1x1 over the concat of T frames, T*64 -> 64 (conv1x1.hip)
hipError_t launch_conv1x1_stream(const float* in, const float* wpack, const float* bias, float* out, int items, int T,
                                 int HW, int act, hipStream_t s);
hipError_t launch_conv1x1_split16(const float* in, const uint16_t* wpack, const float* bias, float* out, int items, int T,
                                  int HW, int act, hipStream_t s,    // same contract on the f16 pipe, exactly split operands
                                  bool in_sf = false, bool out_sf = false);   // in / out in the split format (conv_split16.h)
size_t conv1x1_split16_pack_halfs(int T);
void conv1x1_split16_pack_weights(const float* hwio, int T, uint16_t* dst);   // HWIO [1,1,T*64,64]
size_t conv1x1_pack_floats(int T);
void conv1x1_pack_weights(const float* hwio, int T, float* dst);   // HWIO [1,1,T*64,64]

struct WinoParams {
    const float* in;       // [items][H][W][64]
    const float* upack;    // U = G g G^T, packed [chunk][xi][kk][lane][nu*2+nt] (wino_pack_weights)
    const float* bias;     // [64]; never null
    const float* addend;   // [items/add_div][H][W][64] \ both or
    const float* resid;    // [items][H][W][64]         / neither
    float* out;            // [items][H][W][64]
    int H, W;              // both even
    int add_div;
    int act;
    int items;
    long long in_item_stride;   // floats between consecutive input items; 0 = H*W*64 (conv_wino_ws only)
    const float* in2;      // conv_wino_ws MODE 2 (whole conv2_i): base [items/add_div][H][W][64]; else null
    const float* upack2;   // ... and the packed U of the kernel rows that multiply it
    int accum;             // conv_wino_ws MODE 3 (convmerge1): sum over the add_div frames of a clip, one output per clip
    long long upack_stride;   // ... floats between the packed U of consecutive frames
};
hipError_t launch_conv_wino(const WinoParams& p, hipStream_t s);
hipError_t launch_conv_wino_ws(const WinoParams& p, hipStream_t s);  // persistent wave-specialised variant (conv_wino_ws.hip), same packed U
size_t wino_pack_floats();
void wino_pack_weights(const float* hwio, int cin_total, int cin_begin, float* dst, int cout = 64);

// ---- non-local block (nonlocal.hip) ----------------------------------------------------------
int nl_padded_ch(int C);                                      // 32*ceil(C/32)
hipError_t launch_nl_pack(const float* x, float* X, int B, int T, int H, int W, hipStream_t s);
size_t nl_partial_floats(int B, int N, int C);               // scratch for the key-split partials (0 if unsplit)
hipError_t launch_nl_attn(const float* X, float* Xo, const float* Wp, const float* bp, float* partial, int B,
                          int N, int C, hipStream_t s, const float* Q = nullptr,    // Q: projected queries (nltype 0) or null = X
                          int q0 = 0, int q1 = -1);                                 // queries [q0, q1) only (-1: N): a strip of the frame
hipError_t launch_nl_qproj(const float* X, const float* M, const float* c, float* Q, int B, int N, int C, hipStream_t s,
                           bool dot_column = false);                                // + column C = theta . b_phi (nltype 2)
// the general form of the block (reference utils.py:18-71, nltype 0 / 1 / 2, sub_sample >= 1): keys = values = Kx [B][Nk][CP]
hipError_t launch_nl_attn_general(const float* X, const float* Kx, int Nk, float* Xo, const float* Wp, const float* bp,
                                  float* partial, int B, int N, int C, hipStream_t s, const float* Q, int q0, int q1, bool dot);
hipError_t launch_nl_pool(const float* X, float* Xs, int B, int h2, int w2, int sub, int C, hipStream_t s);
int nl_key_splits(int B, int N);
hipError_t launch_nl_merge(const float* X, const float* Zp, const float* ML, const float* bp, float* Xo, int B, int N, int C, int ks,
                           hipStream_t s, int q0 = 0, int q1 = -1);
hipError_t launch_nl_unpack(const float* Xo, float* out, int B, int T, int H, int W, hipStream_t s);

// ---- head / tail (misc_kernels.hip) ----------------------------------------------------------
// A strip of the frame (single-clip multi-GPU sharding): the trunk buffers hold LR rows [yoff, yoff + Hs)
// of the H-row frame; only rows [core0, core1) (strip-local) of the result are written, at their place in the full output.  The non-local
// block runs the queries [q0, q1) of the packed frame (-1: all of them) against all keys.
struct StripGeom {
    int yoff, Hs, core0, core1;
    int q0 = 0, q1 = -1;
};
hipError_t launch_conv0(const float* Xo, const float* w75x64, const float* bias, float* out, int B,
                        int T, int H, int W, hipStream_t s, const StripGeom* strip = nullptr, bool force_f32 = false);   // force_f32: the VALU fp32 kernel
hipError_t launch_tail(const float* merge, const float* x, const float* w2, const float* b2,
                       float* out, int B, int T, int H, int W, int scale, int merge_cstride, hipStream_t s,
                       const StripGeom* strip = nullptr, unsigned* nonfinite = nullptr);   // nonfinite: set to 1 if a written value is inf / NaN (device or device-mapped host memory)
hipError_t launch_blur_decimate(const float* hr, float* lr, int F, int H, int W, int scale, hipStream_t s);
hipError_t launch_bicubic(const float* x, float* out, int B, int H, int W, int scale, hipStream_t s);
hipError_t run_mfma_selftest(int* mismatches);
hipError_t launch_gather_windows(const float* frames, float* win, int F, int first, int count, int T, size_t frame_floats,
                                 hipStream_t s);
// the output edge's stage 0, one kernel over the sample type (sample_depth.h): fp32 -> uint8 0 .. 255 | uint16 0 .. 1023; n % 4 == 0
hipError_t launch_quantise(const float* sr, uint8_t* out, size_t n, hipStream_t s);
hipError_t launch_quantise(const float* sr, uint16_t* out, size_t n, hipStream_t s);   // sr 16-byte, out 8-byte aligned
// ring [cap][frame_bytes] uint8 (frame f in slot f % cap) -> win [count][T][frame_bytes] fp32 = u8 / 255. as the harness computes it,
// window w slot t = frame clamp(first + w + t - T/2, 0, last); frame_bytes % 4 == 0 (stream.hip)
hipError_t launch_gather_windows_u8(const uint8_t* ring, float* win, int cap, long long last, long long first, int count, int T,
                                    size_t frame_bytes, hipStream_t s);
// stage 0 with a change of primaries in it (colour.hip; the rule: pfnl_amd/colour.py): the same levels, then D -> m -> E per pixel; tab: the
// device copy of colour_geom.h colour_blob of the depth (colour_device_tables); pixels % 4 == 0, sr 16-byte, out 8-byte aligned
struct ColourMatrix;
hipError_t colour_device_tables(const uint16_t** tab8, const uint16_t** tab10);   // of the current device: uploaded once per process, never freed
hipError_t launch_quantise_colour(const float* sr, uint8_t* out, size_t pixels, const uint16_t* tab, const ColourMatrix& m, hipStream_t s);
hipError_t launch_quantise_colour(const float* sr, uint16_t* out, size_t pixels, const uint16_t* tab, const ColourMatrix& m, hipStream_t s);
// ---- scenes of the streaming session (stream.hip; the rule: pfnl_amd/scene.py) ----
// What the block that completes a frame's sum of absolute luma differences does with it: sad[slot] = the sum and, where scene_first is
// given, scene_first[slot] = (force || (detect && min(sum, |sum - sad[prev]|) >= thr_sum)) ? frame : scene_first[prev].
struct SceneDecision {
    unsigned long long* sad;       // [cap]
    long long* scene_first;        // [cap], or null: the sum alone
    int slot, prev;                // frame % cap, (frame - 1) % cap
    long long frame;
    int force, detect;
    unsigned long long thr_sum;
};
hipError_t launch_scene_sad_u8(const uint8_t* a, const uint8_t* b, size_t npix, unsigned long long* scratch, const SceneDecision& d,
                               hipStream_t s);
hipError_t launch_scene_first_frame(unsigned long long* sad, long long* scene_first, int slot, hipStream_t s);
hipError_t launch_gather_windows_u8_scenes(const uint8_t* ring, const long long* scene_first, float* win, int cap, long long last,
                                           long long first, int count, int T, size_t frame_bytes, hipStream_t s);
// the same three kernel bodies on a ring of uint16 samples at 10 bits (a sample above 1023 counts as 1023): win = u10 / 1023. (depth10.py
// dequantise10), the luma of the sums on the 8-bit scale (scene.py luma_u10); frame_bytes = 2 bytes per sample
hipError_t launch_gather_windows_u10(const uint16_t* ring, float* win, int cap, long long last, long long first, int count, int T,
                                     size_t frame_bytes, hipStream_t s);
hipError_t launch_gather_windows_u10_scenes(const uint16_t* ring, const long long* scene_first, float* win, int cap, long long last,
                                            long long first, int count, int T, size_t frame_bytes, hipStream_t s);
hipError_t launch_scene_sad_u10(const uint16_t* a, const uint16_t* b, size_t npix, unsigned long long* scratch, const SceneDecision& d,
                                hipStream_t s);

// ---- the content box of RGB frames (bars.hip; the rule: pfnl_amd/bars.py, its integer steps: bars_geom.h) ----
// frames [n][H][W][3] uint8, or uint16 at 10 bits (a sample above 1023 counts as 1023) -> what BarsOut names, one launch (per 32768
// frames), any alignment a sample can have: 16-byte reads where the rows allow, else 4-byte ones or single samples.  H, W 1 .. 16384,
// limit 0 .. 219, else hipErrorInvalidValue.  scratch: bars_scratch_words(n, H, W) 32-bit words, zero before the first launch; every
// launch leaves the words it needs zero again (launches that share them must not overlap).
struct BarsOut {
    int32_t* box;                  // [n][4] y0, x0, h, w
    uint32_t* rows;                // [n][H] the sums of luma along the rows, or null
    uint32_t* cols;                // [n][W] ... along the columns, or null
};
size_t bars_scratch_words(int n, int H, int W);
hipError_t launch_content_box(const uint8_t* frames, int n, int H, int W, int limit, uint32_t* scratch, const BarsOut& out, hipStream_t s);
hipError_t launch_content_box(const uint16_t* frames, int n, int H, int W, int limit, uint32_t* scratch, const BarsOut& out, hipStream_t s);

// ---- YUV 4:2:0 <-> RGB (yuv.hip; the rule: pfnl_amd/yuv.py, 10 bits: pfnl_amd/depth10.py) ----
// The fifteen integers of yuv.py coefficients(), 14 fractional bits: the one table, computed on the host and passed to the kernels by value.
struct YuvCoef {
    int y0;
    int yr, yg, yb, cbr, cbg, cbb, crr, crg, crb;   // RGB -> YUV
    int dy, drv, dgu, dgv, dbu;                     // YUV -> RGB
};
// bits 8: samples 0 .. 255, limited range 16 .. 235 / 16 .. 240; bits 10: samples 0 .. 1023, 64 .. 940 / 64 .. 960; matrix 0 BT.601 |
// 1 BT.709; false: unknown depth, matrix or range (no device needed)
bool yuv_coefficients(int bits, int matrix, int full_range, YuvCoef* c);
// yuv [n][H*W*3/2] (NV12 or I420, tightly packed) <-> rgb [n][H][W][3]; H, W even; any alignment (words where W and the pointers allow);
// siting: PFNL_SITING_* (0 left | 1 centre | 2 top left; anything else is hipErrorInvalidValue), in all four launchers
hipError_t launch_yuv420_to_rgb_u8(const uint8_t* yuv, uint8_t* rgb, bool nv12, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s);
// The decode's source as planes: H rows of W samples at y; NV12 / P010: H/2 rows of W samples (Cb, Cr interleaved) at cb, cr unused; I420 /
// I010: H/2 rows of W/2 samples at cb and at cr.  pitch_*: BYTES from one row to the next (>= the row); frame: bytes from one frame's planes
// to the next's.  16-bit samples: every pointer and pitch even.
struct YuvPlanes {
    const uint8_t *y, *cb, *cr;
    size_t pitch_y, pitch_cb, pitch_cr, frame;
};
// the same kernel on planes (the packed launcher calls this with pitch W, W/2): words where W, every plane, every pitch and rgb allow
hipError_t launch_yuv420_planes_to_rgb_u8(const YuvPlanes& src, uint8_t* rgb, bool nv12, const YuvCoef& c, int n, int H, int W, int siting,
                                          hipStream_t s);
// the decode at 10 bits, the same kernel body on uint16 samples with the 10-bit table: P010 (semiplanar, the value in the upper ten bits,
// the low six ignored) or I010 (a sample above 1023 is 1023) -> rgb uint16 0 .. 1023; 16-byte words where W % 8 == 0 and the pointers allow
hipError_t launch_yuv420_to_rgb(const uint16_t* yuv, uint16_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s);
hipError_t launch_yuv420_planes_to_rgb_u10(const YuvPlanes& src, uint16_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int siting,
                                           hipStream_t s);
// the encode, one kernel over the sample type: uint8 -> NV12 (semiplanar) or I420 with the 8-bit table; uint16 with values 0 .. 1023 ->
// P010 (semiplanar, samples << 6) or I010 with the 10-bit table; H, W even; any alignment a sample can have
hipError_t launch_rgb_to_yuv420(const uint8_t* rgb, uint8_t* yuv, bool semiplanar, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s);
hipError_t launch_rgb_to_yuv420(const uint16_t* rgb, uint16_t* yuv, bool semiplanar, const YuvCoef& c, int n, int H, int W, int siting, hipStream_t s);

// ---- YUV 4:2:2 / 4:4:4 <-> RGB (yuv_chroma.hip; the same rule with chroma = "422" | "444", the same tables) ----
// chroma: PFNL_CHROMA_422 | PFNL_CHROMA_444 (4:2:0 is the launchers above; anything else is hipErrorInvalidValue); semiplanar: NV16 / NV24
// (16-bit samples: P210 / P410, the value in the upper ten bits), else I422 / I444.  The chroma planes of YuvPlanes then have H rows of
// W / 2 | W samples (interleaved: W | 2 W), a packed frame 2 H W | 3 H W samples.  4:2:2: W even; 4:4:4: any H, W >= 1.  Of the siting only
// the horizontal axis is read, and at 4:2:2 alone.  Words where W and every pointer, pitch and frame stride allow, as above.
hipError_t launch_yuv_planes_to_rgb_chroma(const YuvPlanes& src, uint8_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma,
                                           int siting, hipStream_t s);
hipError_t launch_yuv_planes_to_rgb_chroma(const YuvPlanes& src, uint16_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma,
                                           int siting, hipStream_t s);
hipError_t launch_yuv_to_rgb_chroma(const uint8_t* yuv, uint8_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s);
hipError_t launch_yuv_to_rgb_chroma(const uint16_t* yuv, uint16_t* rgb, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s);
hipError_t launch_rgb_to_yuv_chroma(const uint8_t* rgb, uint8_t* yuv, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s);
hipError_t launch_rgb_to_yuv_chroma(const uint16_t* rgb, uint16_t* yuv, bool semiplanar, const YuvCoef& c, int n, int H, int W, int chroma, int siting,
                                    hipStream_t s);

// ---- packed formats <-> RGB (packed.hip; the rule: pfnl_amd/packed.py; the table: pack_geom.h) ----
// pack: PFNL_PACK_BGR24 .. PFNL_PACK_V210.  n frames in one plane: frame f at plane + f * frame_stride, rows `pitch` bytes apart (a tight
// frame and a caller's surface are one kernel); rgb [n][H][W][3] of uint8 samples for the 8-bit packings and of uint16 values 0 .. 1023
// for the 10-bit ones.  The table is the one of the packing's depth; an RGB packing does not read it.  hipErrorInvalidValue for what
// pack_geom.h refuses, a short pitch or frame stride and a pointer, pitch or stride that is no multiple of the packing's alignment.
// Bytes between a row's end and the pitch are neither read nor written.
hipError_t launch_packed_to_rgb(const void* plane, size_t pitch, size_t frame_stride, int pack, void* rgb, const YuvCoef& c, int n, int H, int W,
                                int siting, hipStream_t s);
hipError_t launch_rgb_to_packed(const void* rgb, void* plane, size_t pitch, size_t frame_stride, int pack, const YuvCoef& c, int n, int H, int W,
                                int siting, hipStream_t s);

// ---- interlaced input: five decoded fields -> one progressive frame (deinterlace.hip; the rule: pfnl_amd/deinterlace.py) ----
// The fields are tight [H/2][W][3] samples of T (uint8_t, or uint16_t whose values are taken as min(v, 1023)), read-only, and may be one
// another; cur has parity `parity` (0: it holds the frame's even rows); out is the tight frame [H][W][3] and overlaps none of them.  H even
// and >= 2, W >= 1, any alignment a sample can have (16-byte words where 3 W samples and every pointer are multiples of 16 bytes, 4-byte
// words for multiples of 4, else single samples).  n = 2 makes both frames of a pushed frame in ONE launch.  hipErrorInvalidValue otherwise.
template <typename T>
struct DeinterlaceJob {
    const T *p2, *p1, *cur, *n1, *n2;
    T* out;
    int parity;
};
hipError_t launch_deinterlace(const DeinterlaceJob<uint8_t>* jobs, int n, int H, int W, hipStream_t s);
hipError_t launch_deinterlace(const DeinterlaceJob<uint16_t>* jobs, int n, int H, int W, hipStream_t s);
hipError_t launch_deinterlace(const uint8_t* p2, const uint8_t* p1, const uint8_t* cur, const uint8_t* n1, const uint8_t* n2, int H, int W, int parity,
                              uint8_t* out, hipStream_t s);
hipError_t launch_deinterlace(const uint16_t* p2, const uint16_t* p1, const uint16_t* cur, const uint16_t* n1, const uint16_t* n2, int H, int W,
                              int parity, uint16_t* out, hipStream_t s);

// ---- inverse telecine: field matching, the weave and the frame distance (telecine.hip; the rule: pfnl_amd/telecine.py) ----
// A, Xc, Xp: the kept field of parity `parity` and its two candidate partners, tight [h][W][3] samples of T (uint16_t: min(v, 1023)),
// read-only; they may be one another.  Any alignment a sample can have (16-byte words, 4-byte words or single samples, as deinterlace.hip).
// The match leaves decision[4] = count of c, count of p, match (0: c, 1: p), post (0 | 1) in device memory and adds one to stats[0 | 1 | 2]
// (matched c, matched p, post-processed; NULL: no statistics).  scratch: two zeroed 64-bit words that every launch leaves zeroed (launches
// that share them must not overlap).  h 3 W < 2^32.
struct TelecineDecide {
    unsigned long long* decision;
    unsigned long long* stats;
    int post;                                // 1: a frame whose smaller count exceeds comb_limit is flagged
    unsigned long long comb_limit;
};
hipError_t launch_telecine_match(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, int threshold,
                                 unsigned long long* scratch, const TelecineDecide& d, hipStream_t s);
hipError_t launch_telecine_match(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity, int threshold,
                                 unsigned long long* scratch, const TelecineDecide& d, hipStream_t s);
// The matched frame out [2 h][W][3] from the decision on the device: the weave of A and the chosen partner, or, post-flagged, what `out`
// already holds (the deinterlaced frame) untouched.  dist != NULL: *dist = sum |out - prev| over all samples, TC_D_FIRST where prev is NULL
// (scratch as above; NULL with dist NULL).  out overlaps none of the inputs.
hipError_t launch_telecine_weave(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, const unsigned long long* decision,
                                 uint8_t* out, const uint8_t* prev, unsigned long long* scratch, unsigned long long* dist, hipStream_t s);
hipError_t launch_telecine_weave(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity, const unsigned long long* decision,
                                 uint16_t* out, const uint16_t* prev, unsigned long long* scratch, unsigned long long* dist, hipStream_t s);

// ---- RGB frames at a chosen raster: the tap tables (resize.hip; the rule: pfnl_amd/resize.py) ----
constexpr int RESIZE_MAX_SIZE = 16384;   // per axis, in and out; ceil(n_in / 4) <= n_out <= 2 n_in
constexpr int RESIZE_TW = 64;            // output pixels of one workgroup: across,
constexpr int RESIZE_TH = 16;            // and down
// One axis: output o = sum_k coef[o * ntaps + k] * in[first[o] + k] / 2^14 over k < count[o] (zero behind count); ntaps = max count.
struct ResizeAxis {
    std::vector<int32_t> first, count;
    std::vector<int16_t> coef;
    int ntaps = 0;
};
bool resize_axis(int n_in, int n_out, ResizeAxis* t, std::string* why);   // false + *why: outside the limits (no device needed)
// Both axes of H x W -> oH x oW as the one block of device memory the kernel reads, and the rows of its largest tile.
struct ResizePlan {
    int H = 0, W = 0, oH = 0, oW = 0, ht = 0, vt = 0, max_rows = 0;
    std::vector<int32_t> blob;
};
bool resize_plan(int H, int W, int oH, int oW, ResizePlan* p, std::string* why);

// ---- a rectangle of the frame on a canvas (place.hip; the rule: pfnl_amd/fit.py place, pfnl_amd/depth10.py place10) ----
// What a session's stage 1 runs (pfnl_stream_resize, pfnl_stream_place): the rectangle src of the raster sH x sW resampled into the rectangle
// dst of the canvas cH x cW, the fill colour elsewhere.  `r` is resize_plan(src.h, src.w, dst.h, dst.w) as it always was - tables, blob and
// the rows of the largest tile, the kernel's tiling being anchored at dst -; cH = 0: off; `whole`: src is the raster and dst the canvas, a
// plain resize, and the launch is the kernel's instantiation without rectangles.
struct PlacePlan {
    ResizePlan r;
    int sH = 0, sW = 0, cH = 0, cW = 0;
    pfnl_rect src{}, dst{};
    bool whole = true;
    uint8_t fill[3] = {0, 0, 0};   // the session's, as given: 8 bits (a 10-bit route replicates, (v << 2) | (v >> 6)); the launchers take their own
};
constexpr uint16_t fill_u10(uint8_t v) { return (uint16_t)((v << 2) | (v >> 6)); }   // 0 -> 0, 255 -> 1023
// src NULL: the whole raster; dst NULL: the whole canvas.  false + *why: place_refused (stream_route.h) or resize_plan says no (no device needed)
bool place_plan(int sH, int sW, int cH, int cW, const pfnl_rect* src, const pfnl_rect* dst, PlacePlan* p, std::string* why);
// in [n][sH][sW][3] -> out [n][cH][cW][3], both passes in one launch, every sample of out stored once; blob_dev: p.r.blob on the device; any
// alignment a sample can have (16-byte stores where cW is a multiple of 16 - of 8 for uint16 samples - and out is aligned, single samples
// otherwise); fill: sample values (uint16: 0 .. 1023), unused by a whole plan.  One kernel over the sample type (sample_depth.h).
hipError_t launch_resize_place(const uint8_t* in, uint8_t* out, const PlacePlan& p, const int32_t* blob_dev, const uint8_t fill[3], int n,
                               hipStream_t s);
hipError_t launch_resize_place(const uint16_t* in, uint16_t* out, const PlacePlan& p, const int32_t* blob_dev, const uint16_t fill[3], int n,
                               hipStream_t s);

// ---- the flips and transposes of the self-ensemble (dihedral.hip; the rule: pfnl_amd/ensemble.py) ----
// member k: bit 0 mirrors W, bit 1 mirrors H, bit 2 transposes H and W (applied last).  scale == 1 leaves the bits as they are.
// out = g_k(in) * scale: in [n][H][W][3] -> out [n][H][W][3], or [n][W][H][3] for k >= 4
hipError_t launch_dihedral(const float* in, float* out, int n, int H, int W, int k, float scale, hipStream_t s);
// acc = (acc + g_k^-1(y)) * scale: acc [n][H][W][3]; y [n][H][W][3], or [n][W][H][3] for k >= 4; one thread per element of acc, no atomics
hipError_t launch_dihedral_accum(float* acc, const float* y, int n, int H, int W, int k, float scale, hipStream_t s);

// ---- the two launches of a tiled forward's run (tiles.hip; the geometry: tile_geom.h; the rule: pfnl_amd/tiles.py) ----
// tiles first .. first + count - 1 of the call's grid `g` (inside its total: the callers check).  Both copy bits, in 16-, 8- or 4-byte words
// as the addresses allow.
struct TileGrid;
// in [B][T][H][W][3] -> tiles [count][T][th][tw][3]
hipError_t launch_tile_gather(const float* in, float* tiles, const TileGrid& g, int T, int first, int count, hipStream_t s);
// y [count][scale th][scale tw][3] -> the owned rectangles of those tiles inside out [B][scale H][scale W][3], each element stored once
hipError_t launch_tile_scatter(const float* y, float* out, const TileGrid& g, int scale, int first, int count, hipStream_t s);

// ---- Y-channel PSNR / SSIM sums of uint8 RGB frame pairs (score.hip) ---------------------------
// pred, truth [F][H][W][3]; out [F][4] = sum_d2_full, sum_d2_crop (border sp_border), ssim_sum_full, ssim_sum_valid;
// partial: score_scratch_bytes(F, H, W) of device memory (one slot per workgroup: the sums are repeatable bit for bit)
size_t score_scratch_bytes(int F, int H, int W);
hipError_t launch_score_y(const uint8_t* pred, const uint8_t* truth, int F, int H, int W, int sp_border, double* out, double* partial,
                          hipStream_t s);

}  // namespace pfnl
