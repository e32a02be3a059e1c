/*
 * pfnl_hip.h — C-ABI of libpfnl_hip.so: the MI355X (gfx950) implementation of PFNL's
 * forward/inference hot path.
 *
 * The reference (psychopa4/PFNL) is pure Python on TensorFlow 1.12 and has no FFI/operator
 * interface of its own; the seam this library replaces is the TF runtime underneath
 *   - PFNL.forward                 (reference model/pfnl.py:39-80)   -> pfnl_forward
 *   - utils.NonLocalBlock          (reference utils.py:18-71)        -> pfnl_op_nonlocal
 *   - tf.layers.Conv2D instances   (reference model/pfnl.py:48-53)   -> pfnl_op_conv2d
 *   - tf.image.resize_images(..,2) (reference model/pfnl.py:63)      -> pfnl_op_bicubic
 *   - tf.train.Saver.restore       (reference model/base_model.py:231-243): variables arrive
 *     through pfnl_set_weight under their TF names (nlvsr/conv0/kernel ...), HWIO float32.
 *   - sess.run(SR_test, feed_dict) (reference model/pfnl.py:252,309) -> pfnl_forward with host
 *     pointers (H2D/D2H inside, like the reference's timing includes).
 *
 * Conventions: every entry point is extern "C", takes plain pointers and sizes, returns 0 on
 * success or a negative pfnl_status; the message of the last failure on the calling thread is
 * available from pfnl_last_error().  A handle is bound to one device and is not re-entrant;
 * distinct handles are independent, from distinct host threads too (tests/test_gpu_threads.py), with one
 * exception that is the HIP runtime's: while a handle captures a graph (option graph = on / auto, inside
 * pfnl_forward), a BLOCKING copy made by the caller on another thread (hipMemcpy, hipMemcpyToSymbol) fails
 * with hipErrorStreamCaptureImplicit and invalidates the capture: that pfnl_forward returns PFNL_ERR_HIP.
 * The library's own blocking copies wait for a capture to end (one process-wide lock).  "device pointer" = memory accessible from that device
 * (e.g. a torch-ROCm tensor's data_ptr()); "stream" = a hipStream_t passed as void* (NULL: see
 * STREAMS below).  All tensors are float32 (the *_bf16 single-op hooks alone take bfloat16 bit patterns as
 * uint16_t), contiguous, NHWC-style as in the reference:
 *   input  [B, T, H, W, 3]      values nominally in [0,1]
 *   output [B, 1, s*H, s*W, 3]  not clipped (the harness clips, reference model/pfnl.py:255-257)
 *
 * STREAMS (tested on hipStreamNonBlocking streams: tests/test_gpu_streams.py).  An entry that takes `stream` and
 * device pointers enqueues ALL its work on that stream and returns: nothing of it runs on, or waits for, another stream.  stream == NULL
 * with device pointers is the legacy null stream itself (pfnl_forward, pfnl_forward_strip, the op hooks); host-pointer forwards and
 * graph replays of a NULL-stream call run on the handle's own blocking stream, which the null stream orders implicitly, and a
 * host-pointer call returns with its output filled.  A captured graph (option "graph") is captured and replayed on the caller's stream,
 * between staging copies on that stream.  A session has two streams: the one given to pfnl_stream_open (gather, forward, quantisation,
 * the edge kernels, device-pointer pushes and pops) and a non-blocking copy stream of its own (host-pointer pushes and pops, which
 * return with the copy complete); pfnl_stream_scenes / _format / _resize / _place are setup calls that allocate and may block.  The calls on one
 * handle share its workspace: a caller that changes the stream between calls orders them itself (an event, or a synchronise), and plain
 * forwards between the pushes of a session go on the session's stream.  pfnl_sync waits for the handle's own stream and the null
 * stream, NOT for a stream of the caller's: synchronise that one first, then pfnl_sync or pfnl_range_flag reads the range flag of the
 * device-pointer calls behind it.  Op hooks that synchronise `stream` before they return (they upload a weight pack or a table with a
 * blocking copy, which goes through the null stream): every pfnl_op_* that takes host weights (the conv, non-local, conv0 and tail
 * hooks), pfnl_op_resize_u8 / _u10, pfnl_op_resize_place_u8 / _u10 and pfnl_op_scene_sad_u8.  Asynchronous: pfnl_op_gather_windows / _u8 / _u8_scenes,
 * pfnl_op_quantise_u8 / _u10, pfnl_op_yuv420_to_rgb_u8 / _u8_surface, pfnl_op_rgb_to_yuv420_u8 / _u10, pfnl_op_bicubic, pfnl_op_blur_decimate (its
 * first call per device uploads a constant table), pfnl_op_score_y.
 */
#ifndef PFNL_HIP_H
#define PFNL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pfnl_handle pfnl_handle;

typedef enum pfnl_status {
    PFNL_OK = 0,
    PFNL_ERR_INVALID = -1,     /* bad argument / shape (odd H or W, unknown tensor name ...) */
    PFNL_ERR_STATE = -2,       /* e.g. forward before finalize_weights, missing weights        */
    PFNL_ERR_HIP = -3,         /* a HIP runtime call failed                                    */
    PFNL_ERR_NOMEM = -4,
    PFNL_ERR_NODEVICE = -5,    /* no gfx950-capable device visible                             */
    PFNL_ERR_COMM = -6,        /* an RCCL call failed / RCCL could not be loaded               */
    PFNL_ERR_RANGE = -7        /* a forward left the range of its binary16-operand kernels (see "strict_fp32"): pfnl_sync after a
                                  device-pointer forward; pfnl_forward itself with host pointers under precision=bf16 (no f32 re-run there) */
} pfnl_status;

/* Mirrors the constants hard-coded in the reference (model/pfnl.py:21-23, 40-43). */
typedef struct pfnl_config {
    int32_t num_frames;   /* T: 7 (reference); 3 and 5 also supported                    */
    int32_t scale;        /* 4 (reference) or 2 (build-defined tail)      */
    int32_t mf;           /* trunk width, must be 64                                     */
    int32_t num_block;    /* progressive-fusion blocks, 20 in the reference (>=0)        */
    int32_t device_id;    /* HIP device ordinal                                          */
    int32_t reserved[3];  /* must be 0                                                   */
} pfnl_config;

const char* pfnl_last_error(void);
int pfnl_version(void);                        /* ABI version, currently 4 (+ the _ex op hooks: MFMA shape and split chains chosen by the caller) */
int pfnl_device_count(int* count);

/* ---- model lifetime ---------------------------------------------------------------------- */
int pfnl_create(const pfnl_config* cfg, pfnl_handle** out);
int pfnl_destroy(pfnl_handle* h);

/* Replaces tf.train.Saver.restore (reference model/base_model.py:231-243).  `tf_name` is the TF
 * variable name ("nlvsr/conv1_3/kernel", "nlvsr/nlblock_0/g/g/bias" ...; reference
 * model/pfnl.py:47-53, utils.py:23-26,66-67).  `host` is float32 HWIO (kernels) / [Cout] (biases)
 * and stays owned by the caller; the library keeps its own repacked device copies. */
int pfnl_set_weight(pfnl_handle* h, const char* tf_name, const float* host,
                    const int64_t* shape, int rank);
/* Optional: "nlvsr/nlblock_0/theta/theta/{kernel,bias}" and ".../phi/phi/{kernel,bias}" ([1,1,C,C] / [C], C = 12T) switch
 * the non-local block to the embedded-Gaussian form (reference utils.py:31-42 with nltype 0: theta = conv(x), phi = conv(x));
 * all four or none.  PFNL itself calls the block with nltype 1 (model/pfnl.py:58), where these scopes hold no variables.
 * Number of variables still missing (0 = complete; the optional ones never count). */
int pfnl_missing_weights(pfnl_handle* h, int* count);
/* Repack + upload: splits conv2_i into its shared-`base` half and per-frame half, folds
 * Wg*Ww of the non-local block, chunks the implicit-GEMM weights. */
int pfnl_finalize_weights(pfnl_handle* h);

/* Tuning knobs (all parity-tested):  key "conv3x3" =
 *   "auto"          (default) "split16" when a launch has at least 200 tiles of 8x32 pixels, "winograd" below that;
 *   "winograd"      fused Winograd F(2x2,3x3) on f32 MFMA (2.25x fewer multiplies), persistent
 *                   wave-specialised kernel: matrix waves + helper waves (conv_wino_ws.hip);
 *   "winograd_tile" same maths, one 4-wave workgroup per tile (conv_wino.hip);
 *   "direct"        implicit-GEMM f32 MFMA (conv_mfma.hip);
 *   "split16"       direct 3x3 on the f16 matrix pipe with exactly split fp32 operands (3 f16 MFMAs per product block,
 *                   fp32 accumulation, >= 22 mantissa bits per product: conv_split16.hip);
 * key "strict_fp32" = "off" (default) | "on".  The default fp32 path computes on the f16 matrix pipe with exactly split operands
 *   (fp32 tensors, fp32 accumulation, >= 22 mantissa bits per product) and therefore has a DOMAIN the reference's fp32 kernels do
 *   not have: |activation|, |weight| < 65504, and inputs of the non-local block on a [0,1] scale (|x| < ~350).  Leaving it makes
 *   an operand inf and the result non-finite; the tail kernel flags that.  Host-pointer calls then redo the call on the f32-MFMA
 *   kernels before returning (pfnl_range_reruns counts them), so they cover the whole fp32 range; device-pointer calls are
 *   asynchronous: pfnl_sync returns PFNL_ERR_RANGE.  "on" (or env PFNL_STRICT_FP32=1) uses the f32-MFMA kernels throughout; weights
 *   beyond binary16's range select them by themselves at pfnl_finalize_weights.
 * key "small" = "auto" (default: the small-shape trunk kernels of conv_small.hip when a 3x3 launch has fewer than 200 tiles (256 until round 5) of 8x32
 *   pixels - conv2_i as one 128 -> 64 convolution) | "on" | "off".
 * key "small_c10" = "on" (default since round 4: TWO launches per progressive-fusion block at small shapes - the conv1_i launch also
 *   runs its finished tile through this frame's 64 x 64 slice of conv10_i and writes the partial sum; the conv2_i launch adds the T
 *   partials (+ bias, leaky-relu) on the way into LDS: its `base` source.  No 1x1 launch, no inter-workgroup exchange inside a
 *   launch, fixed summation order) | "off" (three launches, conv10_i on conv_small_1x1_kernel).
 * key "split16_sf" = "on" (default) | "off": with conv3x3 and conv1x1 on "split16", conv1_i and conv10_i write the split format
 *   (hi, lo' binary16 pairs: the MFMA operands themselves) and both halves of conv2_i read it by LDS-DMA (conv_sf.hip).
 * key "split16_chain" = "on" (default) | "off": with split16_sf, conv2_i is one launch - per (clip, tile) the shared half stays in
 *   registers as the initial C of the T per-frame tiles (no pb tensor, no addend reads, 20 launches fewer per forward).
 * key "split16_c10" = "on" (default) | "off": with split16_sf, conv1_i and conv10_i are one launch (conv3x3_c1c10_kernel): per (clip,
 *   tile) the T frame tiles of conv1_i leave as split-format lines through LDS, where conv10_i takes them as MFMA operands - inp1 is
 *   written once and never read back by a 1x1 launch (2 launches per progressive-fusion block with split16_chain).
 * key "split16_mid" = "auto" (default since round 5) | "off": the two-launch block deals out CHAINS - a workgroup takes the T frames of
 *   a (clip, 8x32-pixel tile) - so a launch with fewer chains than CUs leaves most of the chip idle (one clip of 128x128: 64 chains).
 *   Below 136 chains (and above the small-shape rule's 200 tiles; both scale with the device's CU count / 256) the block runs as four launches that deal out single tiles:
 *   conv1_i, conv10_i, the shared half of conv2_i, the per-frame half in flat order (same arithmetic as split16_c10=off +
 *   split16_chain=off; tools/precision_ladder.py has the crossover).  Only with conv3x3=auto and both of those options on.
 * key "split16_splitchains" = "auto" (default since round 6) | "off": the two-launch block deals out whole (clip, tile) chains, so a batch whose
 *   chains are not a whole number of rounds of the grid (256 workgroups) pays a whole extra chain for its last, partial round (5 clips of
 *   128x128 = 1.25 rounds took 1.57x the time of 4).  When that round has at most grid / 2 chains, they are cut by FRAMES into parts (one per
 *   workgroup): conv3x3_c1c10_kernel leaves a part's share of conv10_i's sum as raw fp32 and c10_finalize_kernel adds the parts up in fixed
 *   order (+ leaky-relu, split format); the chain kernel recomputes the shared half per part.  Deterministic; batches that are whole rounds
 *   (configs[1]) run exactly as before (bit-identical); the clips of the whole rounds keep their bits, the cut chains differ from the uncut
 *   launch in summation order (oracle tolerance).  pfnl_plan: "chain2_split", whole_chains / split_parts / part_frames.  The bf16 trunk's two chained
 *   launches and convmerge1's accumulating launch are cut the same way ("bf16_3_split").
 * key "split16_sf0" = "off" (default) | "on" (round 6): in the two-launch block ("chain2") the chain kernel writes the block's output - the
 *   next block's inp0 - a second time in the split format, and conv3x3_c1c10_kernel takes its halo from that copy by LDS-DMA in operand form
 *   (no fp32 -> binary16 split on the VALU, no register-staged commit).  Same operands in the same order: BIT-IDENTICAL results (tested).
 *   Measured slower on the same box (configs[1]: 4.86 against 4.45 ms per step - the copy costs the chain kernel 22 us per launch, the
 *   DMA halo saves conv1_i + conv10_i 0.6 us: DESIGN.md R6.1), so it is not the default; kept as the switch that reproduces the measurement.
 * key "conv1x1" = "split16" (default: streaming kernel on the f16 pipe, exactly split fp32 operands) | "stream" (streaming f32-MFMA
 *                 kernel) | "tiled" (conv_mfma.hip).
 * key "nonlocal" (fp32 precision only) = "auto" (default: "split16" from 1024 keys, "f32" below) | "f32" (f32 MFMA, nonlocal.hip) |
 *                 "split16" (f16 MFMA with exactly split operands: fp32-level accuracy at a third of the time, nonlocal_f16.hip).
 * key "graph"   = "off" (default) | "on" (every shape is captured into a hipGraph on its second call and replayed
 *                 between the staging buffers) | "auto" (only shapes with frames*H*W <= 65536 pixels).  Measured: no
 *                 gain - the small shapes are bound by per-kernel latency, not by launch gaps.
 * key "conv2"   = "grouped" (default with conv3x3=winograd: one launch per block, shared half in LDS; taken when there
 *                 are at least 224 (clip, 4x32-pixel tile) groups, like the accumulating convmerge1) | "split".
 * key "precision" = "fp32" (default: the reference's arithmetic, |dPSNR| <= 0.01 dB) | "bf16" (BASELINE.json configs[3]:
 *                 the 20 progressive-fusion blocks keep their activations and weights in bf16 and accumulate in fp32 on
 *                 bf16 MFMA (conv_bf16.hip); the non-local block, its logits, conv0's arithmetic, convmerge1, the tail and
 *                 the bicubic skip stay fp32; the interface tensors stay float32.  Tolerance: DESIGN.md section 4).
 * key "nl_type" = "auto" (default: 0 when the theta / phi variables are loaded, else 1 = PFNL's own call, model/pfnl.py:58) | "0" |
 *                 "1" | "2": utils.NonLocalBlock's nltype (embedded Gaussian / Gaussian / dot product; 0 and 2 need theta / phi).
 * key "nl_sub_sample" = "1" (default, PFNL's call) | n: average-pool g and phi n x n on the space_to_depth grid (utils.py:27-28,35-36).
 *                 nl_type != 1 or nl_sub_sample > 1 run on the f32-MFMA kernel (nonlocal.hip) in both precisions.
 *                 ONE DIVERGENCE FROM THE REFERENCE AS WRITTEN, by design: utils.py:57-58 takes exp(S) and then divides by its row sum
 *                 without subtracting the row maximum, so a row whose sum exceeds fp32's range (N exp(s) > 3.4e38: at N = 4096 every
 *                 logit > 80.4, i.e. a 128x128 input that is >= 0.98-white throughout) comes out as P = 0 / inf = 0 and the block returns
 *                 its bias there.  Every kernel here runs the softmax as a streaming, max-subtracted recurrence: on those inputs it
 *                 returns the mathematically defined softmax (tested against the stabilised fp64 oracle), everywhere else the same
 *                 values as the reference's formula.  There is no "as written" switch: reproducing an overflow is not a feature.
 * key "bf16_conv10" = "fused" (default: conv10_i runs inside the conv1_i launch of the bf16 trunk) | "separate".
 * key "bf16_mfma" = "16" (default since round 6: the two chained 3x3 launches of the bf16 trunk issue v_mfma_f32_16x16x32_bf16 - the K = 32 shape costs 14 %
 *   less energy per FLOP on a package that sits on its power cap; 1080p 3.77 -> 3.58 ms) | "32" (the 32x32x16 form: same rounding points, another summation order).
 * key "split16_mfma" = "16" (default since round 6: the chain launch of conv2_i - fp32 path, whole rounds of at least one (clip, tile) chain per CU - issues
 *   v_mfma_f32_16x16x32_f16, conv3x3_sf_chain16_kernel; split chains, split16_sf0 and launches with fewer chains stay on the 32x32x16 kernel) | "32".
 *   Under the same rule conv1_i's 3x3 stage of the block's other launch runs on that shape too (conv3x3_c1c10_kernel's M16 form; conv10_i's stage stays on
 *   32x32x16); "32" restores the 32x32x16 kernels for both launches.  pfnl_plan's mfma field says which ran (c1_mfma: the conv1_i + conv10_i launch).  Same operands, another summation order: results agree within rounding (observed 2e-7), not bit for bit.
 * key "bf16_nonlocal" = "f16" (the only value since round 4: the non-local block of precision=bf16 on the f16 matrix pipe with
 *                 binary16 operands, fp32 accumulation and softmax state - nonlocal_f16.hip, hi parts only; within 1e-3 of the
 *                 fp64 block on [0,1]-scale outputs, measured 1e-4 ... 5e-4.  Round 1's split-operand bf16 kernel - 2.5x the
 *                 MFMAs at the same error - is kept out of the library under tools/experiments/nonlocal_bf16.hip).
 * The default can also be set with the environment variable PFNL_CONV3X3 read by pfnl_create.
 * Kernel generations that are NOT options (round 5): the library ships one kernel per job.  What remains switchable by environment, read
 * once per process, is the assignment of the two bf16 3x3 generations to the three modes - PFNL_BF16_V3 = 0 (second generation,
 * conv_bf16_v2.hip, for all three), 1 (third generation for all three), 2 (third for conv1_i + conv10_i only); default: third for conv1_i +
 * conv10_i and the per-frame half of conv2_i, second for the shared half.  Same arithmetic in every assignment (bit-equal results): it
 * exists as the same-box A/B switch and as the reference of the schedule soak test (tools/soak_r04.py), not as a fallback for a failure.
 * Gone since round 5: PFNL_BF16_V2 (first-generation bf16 kernel for modes 0 - 2), PFNL_NL_SW (first-generation non-local kernel; batches
 * beyond 2 GB of packed operands run through the one kernel in clip chunks). */
int pfnl_set_option(pfnl_handle* h, const char* key, const char* value);
/* The current value of option `key` in the spelling pfnl_set_option takes back - whatever set it (a call, an environment variable read by
 * pfnl_create, the default).  For callers that change an option temporarily (the harness's range-flag recovery, model.py) and must put back
 * what was there, not what they remember having set.  NUL-terminated into buf[buflen]. */
int pfnl_get_option(pfnl_handle* h, const char* key, char* buf, size_t buflen);

/* ---- the hot path ------------------------------------------------------------------------ */
/* Replaces sess.run(SR_test, feed_dict={L_test: ...}) (reference model/pfnl.py:252,309) /
 * PFNL.forward (model/pfnl.py:39-80).  `in`  = [B,T,H,W,3] float32, `out` = [B,1,sH,sW,3]
 * float32.  H and W must be even (tf.space_to_depth, model/pfnl.py:57).  With device pointers
 * the call is asynchronous on `stream`; with host pointers it returns when `out` is filled. */
int pfnl_forward(pfnl_handle* h, const void* in, int in_is_device, void* out, int out_is_device,
                 int B, int H, int W, void* stream);
/* Single-clip multi-GPU sharding (the reference is single-GPU, main.py:10): the rows
 * [scale*row0, scale*(row0+nrows)) of every SR frame, written at their place in the FULL-size `out`.  `in` is the full clip
 * (device pointers, asynchronous on `stream`).  The non-local block runs this strip's queries against ALL keys of the frame
 * (they need the whole input, which every rank holds: 7 LR frames), the trunk runs on the strip plus a halo of
 * 4 + 2*num_block LR rows per side that is recomputed instead of exchanged - ranks share nothing on the data path and the
 * union of the strips equals pfnl_forward's output up to summation order (tile alignment differs). */
int pfnl_forward_strip(pfnl_handle* h, const void* in, void* out, int B, int H, int W, int row0, int nrows, void* stream);
/* SELF-ENSEMBLE (additions to version 4; with n = 1, the default everywhere, every path issues the calls it always issued).  The "+" row
 * of a super-resolution table: the network runs on the flips and transposes of its input, each result is transformed back, and the
 * results are averaged.  The reference has no such switch; the loop sits around its sess.run(SR_test, ...) (model/pfnl.py:252, 309), i.e.
 * around pfnl_forward.  The rule is stated once on the host, pfnl_amd/ensemble.py.  Members k = 0 .. 7 act on the axes H, W of
 * [..., H, W, 3]: bit 0 mirrors W, bit 1 mirrors H, bit 2 transposes H and W and is applied last; g_k^-1 undoes the steps in reverse
 * order.  An ensemble of n in {1, 2, 4, 8} uses members 0 .. n-1 (2: the horizontal mirror; 4: both mirrors; 8: adds the transposes, which
 * run the network at W x H) and is
 *     acc = f(x);  for k = 1 .. n-1: acc = fl32(acc + g_k^-1(f(g_k(x))));  out = acc * (1 / n)
 * with f the plain forward of this handle at the same B, fp32 accumulation in increasing k by the one thread that owns each output element,
 * and an exact scale (a power of two).  n = 1 IS pfnl_forward; n > 1 equals the composition of pfnl_forward calls byte for byte.
 *   pfnl_forward_ensemble: arguments, checks, stream rule and host-pointer staging of pfnl_forward; n outside {1, 2, 4, 8} is
 *     PFNL_ERR_INVALID before any device call.  Member 0 writes `out` directly; every other member goes g_k(in) -> a handle buffer, the
 *     forward -> a second handle buffer, and is added into `out` at g_k^-1's positions (pfnl_amd/csrc/dihedral.hip: two bandwidth-bound
 *     kernels, the transposing members through an LDS tile).  Both buffers and the workspace of BOTH geometries (the plan-dependent
 *     buffers differ between H x W and W x H) are sized before the first member is enqueued: nothing moves while members are in flight.
 *   Range: every member's tail kernel writes the call's flag.  A host-pointer call reads it once, behind the last member, and redoes the
 *     WHOLE ensemble on the f32-MFMA kernels (one count in pfnl_range_reruns; PFNL_ERR_RANGE under precision=bf16, as pfnl_forward);
 *     device-pointer calls stay asynchronous and leave the flag to pfnl_sync / pfnl_range_flag.
 *   The option "graph" does not apply for n > 1: members always run eagerly.  The kernels of dihedral.hip run under no profile class.
 *   pfnl_stream_ensemble (below): a session's batches go through this call.
 * Out of scope: pfnl_forward_strip and the multi-GPU paths stay without an ensemble; other groups (rotations by other angles, temporal
 * reversal); weighting the members. */
int pfnl_forward_ensemble(pfnl_handle* h, const void* in, int in_is_device, void* out, int out_is_device,
                          int B, int H, int W, int n, void* stream);
/* TILES (additions to version 4; with no tiling, the default everywhere, every path issues the calls it always issued).  The tile-size
 * switch of a super-resolution tool: a large frame runs as a batch of overlapping tiles of one shape.  The trunk is linear in the frame
 * and the non-local block quadratic (4 N^2 84 FLOPs per clip, N = (H/2)(W/2)); on tiles the block runs at patch scale, nearer its
 * training scale (in_size 32) than a 4K frame is.  The reference has no such switch; like the self-ensemble the loop sits around
 * pfnl_forward.  The rule is stated once on the host, pfnl_amd/tiles.py, and once in C++, pfnl_amd/csrc/tile_geom.h.  Per axis of
 * length n (even), tile extent t and margin p = pad:
 *     t == 0 or t >= n: one tile [0, n) that owns all of it.  Otherwise t is even, p >= 0, 2p < t, and
 *     step = t - 2p;  count = ceil((n - 2p) / step);  origin o_i = min(i step, n - t)   (the last tile moves inward)
 *     tile i owns [a_i, b_i):  a_0 = 0,  a_i = o_i + p,  b_i = a_(i+1),  b_last = n
 * so every tile has extent t and an even origin, the owned ranges partition [0, n), and every owned sample lies at least p from each
 * tile edge that is not a frame edge.  One pad serves both axes.  The tiles of a call are numbered (b ny + iy) nx + ix and run in runs
 * of `batch` consecutive tiles (the last run may be shorter; 0: all in one run), each run one forward at [run,T,th,tw,3]; the output is
 * the owned rectangle of each tile's result, scaled by `scale`, at its place - every output element is written exactly once, nothing is
 * blended.  With pad >= 4 + 2 num_block (the halo pfnl_forward_strip recomputes) the result differs from the full-frame forward only
 * through the non-local block seeing its own tile.
 *   pfnl_tile_axis: the axis rule; needs no device.  *count receives the number of tiles; the arrays, each NULL or of *count entries
 *     (call once with NULL arrays for the count), the origins and the owned ranges.  A bad n, tile or pad is PFNL_ERR_INVALID.
 *   pfnl_forward_tiled: arguments, checks, stream rule and host-pointer staging of pfnl_forward_ensemble, plus the tiling's own check
 *     (odd or negative extents, 2 pad >= tile where the axis is split, negative pad or batch, a tile count beyond int), all before any
 *     device call.  t == NULL, or one tile per clip in one run, IS pfnl_forward_ensemble(..., ensemble_n, ...): the same launches.  Else
 *     each run is gather -> the forward (the ensemble for ensemble_n > 1) -> scatter on the caller's stream (pfnl_amd/csrc/tiles.hip: two
 *     bandwidth-bound kernels).  Two grow-only handle buffers - the run's tile stack and the run's result - and the workspace of both run
 *     sizes (the full run and the short last one; for ensemble_n == 8 of the transposed tile as well) are sized before the first run is
 *     enqueued: nothing moves while runs are in flight.
 *   Range: every run's tail kernel writes the call's flag.  A host-pointer call reads it once, behind the last run, and redoes the WHOLE
 *     tiled call on the f32-MFMA kernels (one count in pfnl_range_reruns; PFNL_ERR_RANGE under precision=bf16); device-pointer calls stay
 *     asynchronous and leave the flag to pfnl_sync / pfnl_range_flag.
 *   The option "graph" does not apply: runs always execute eagerly.  The kernels of tiles.hip run under no profile class.
 *   pfnl_stream_tile (below): a session's batches go through this call.
 * Out of scope: blending in the overlap; per-axis pads; tiles for pfnl_forward_strip and the multi-GPU paths; gathering tiles straight
 * from the session's uint8 ring. */
typedef struct pfnl_tiling { int32_t tile_h, tile_w, pad, batch; } pfnl_tiling;
int pfnl_tile_axis(int n, int tile, int pad, int* count, int32_t* origin, int32_t* own_first, int32_t* own_count);
int pfnl_forward_tiled(pfnl_handle* h, const void* in, int in_is_device, void* out, int out_is_device, int B, int H, int W,
                       const pfnl_tiling* t, int ensemble_n, void* stream);
/* Every buffer a pfnl_forward with these arguments can touch.  pfnl_forward_ensemble with n > 1 adds two grow-only buffers that are not
 * counted here: the transformed input, B*T*H*W*3 floats, and one member's output, B*sH*sW*3 floats; with n = 8 also whatever the plan of
 * (B, W, H) needs beyond that of (B, H, W) (pfnl_workspace_bytes(h, B, W, H) states it).  pfnl_forward_tiled touches what a forward of
 * its full run touches, pfnl_workspace_bytes(h, run, th, tw), plus two grow-only buffers of its own: the run's tile stack,
 * run*T*th*tw*3 floats, and the run's result, run*s*th*s*tw*3 floats. */
int pfnl_workspace_bytes(pfnl_handle* h, int B, int H, int W, size_t* bytes);
/* THE LAUNCH PLAN of the progressive-fusion trunk (reference model/pfnl.py:65-71) for a [B,T,H,W,3] forward under the handle's current
 * options, as text: "<structure> launches_per_block=<n> c1x1=<launches of class conv1x1 among them> precision=<..> conv3x3=<..> conv1x1=<..>
 * c10_fused=<0|1> chain=<0|1> sf0=<0|1> strict=<0|1> tiles=<8x32-pixel tiles per per-frame launch> chains=<(clip, tile) chains>
 * whole_chains=<n> split_parts=<s> part_frames=<q> nl=<split16 | f16 | f32 | general_f32: the non-local block's kernel family> nl_pack_fused=<0|1> mfma=<16|32: the MFMA shape of the chained 3x3 launches - 16 = v_mfma_f32_16x16x32_*: the bf16 trunk's, and the fp32 chain launch of conv2_i when every CU has a chain> merge1=<small | bf16 | split16 | split16_cut | winograd | direct: convmerge1's launch; split16_cut adds c10_finalize_kernel>".  Structures: "small2" / "small3" (conv_small.hip,
 * below ~0.78 tiles per CU: 200 on a 256-CU device), "mid4" (four per-tile launches, below ~0.53 chains per CU: 136), "chain2" (conv1_i +
 * conv10_i, then the whole of conv2_i), "chain2_split" (the same with the chains of a last, partial round cut by frames: option
 * split16_splitchains) and "chain2_sf0" (the same with a split-format copy of every block's output so that the next block's
 * conv1_i takes its halo by LDS-DMA: option split16_sf0=on), "split16_3" / "split16_4", "winograd_ws3" / "winograd_ws4", "winograd_tile4",
 * "direct4"; bf16: "bf16_3", "bf16_3_split", "bf16_4", "bf16_mid4".  The ONE statement of the dispatch rule (pfnl_amd/csrc/launch_plan.h: trunk_plan, a pure
 * function of the options, the shape and the CU count, testable on the host): pfnl_forward runs it, pfnl_workspace_bytes sizes
 * from it, bench.py's byte model and the tests read it here.  The structure changes the summation order, hence the last bits: the same clip
 * gives bit-different (oracle-equal) results in a batch that takes "chain2" and alone ("mid4" / "small2"). */
int pfnl_plan(pfnl_handle* h, int B, int H, int W, char* buf, size_t buflen);
int pfnl_sync(pfnl_handle* h);
/* number of synchronous forwards that were redone on the f32-MFMA kernels because the f16-pipe range flag was set */
int pfnl_range_reruns(pfnl_handle* h, long long* count);
/* The range flag of ASYNCHRONOUS (device-pointer) forwards, read and cleared WITHOUT synchronising: *flagged = 1 when a
 * device-pointer forward that has completed since the last pfnl_sync / pfnl_range_flag wrote a non-finite value.  The caller
 * orders the read behind the forwards it asks about (an event / stream synchronise of its own) - what a pipelined harness uses
 * once per batch instead of pfnl_sync (pfnl_amd/model.py, the replacement of the loop around sess.run, reference
 * model/pfnl.py:249-258).  Synchronous (host-pointer) forwards keep a flag of their own and never consume this one.  The fence
 * is armed where a kernel with a binary16 domain runs and a non-finite value cannot be the reference's own result: not under
 * strict_fp32 (f32-MFMA kernels throughout) and not with nl_type 2 (0 / 0 for a query without a positive affinity).
 * The word is taken with one atomic exchange, so a flag raised by a forward that is STILL IN FLIGHT while this is called is not lost:
 * it is either returned now or by the next call - i.e. a returned 1 may also cover forwards that have not completed yet (a caller that
 * re-runs a batch on it should treat the batches already enqueued behind it as suspect too: pfnl_amd/model.py does). */
int pfnl_range_flag(pfnl_handle* h, int* flagged);

/* ---- streaming session: uint8 LR frames in, uint8 SR frames out ------------------------------ */
/* The loop the reference runs around sess.run (model/pfnl.py:236-262, 293-320: clamped T-frame windows, the forward, clip / round to uint8)
 * for frames that arrive one at a time and a sequence whose length is not known: push LR frames [H,W,3] uint8 RGB (values / 255. as the
 * harness feeds them), pop SR frames [sH,sW,3] uint8 in index order.  One open session per handle; `hip_stream` NULL = the handle's own.
 * BATCHES: frame i is super-resolved in the batch [k*batch, min((k+1)*batch, F)) that holds it, whatever the timing of the calls -
 *   pfnl_stream_next_batch is the rule, and the session runs it: first = launched; before pfnl_stream_end a batch launches when its last
 *   window's newest frame is there (pushed >= launched + batch + T/2), after it the remainder does (count = min(batch, pushed - launched)).
 *   The launch plan, and with it the last bits, depend on the batch size (pfnl_plan): these are the batches - and the bytes - of
 *   test_video_lr with num_once == batch.
 * push copies the frame into a device ring (host pointer: the buffer is free on return) and, when a batch is due, enqueues window gather,
 *   pfnl_forward and quantisation on the session's stream without waiting for them.  pop delivers the next frame (*got = 1, *index) or
 *   nothing (*got = 0: not an error); it waits only for the batch that holds that frame.  With device pointers both are asynchronous on
 *   the session's stream.  pfnl_stream_ready: the frames pop would deliver without another push.
 * BOUNDED: at most 2 * batch undelivered SR frames; a push that would launch a batch beyond that returns PFNL_ERR_STATE ("pop first") and
 *   changes nothing.  All device buffers are allocated by pfnl_stream_open (ring of 3 batch + T - 2 LR frames, one window stack, two
 *   batches of SR frames).
 * RANGE: before the first frame of a batch leaves, the session reads pfnl_range_flag; a flagged batch and every batch already enqueued
 *   behind it are computed again with strict_fp32=on (under precision=bf16: precision=fp32 as well), and so is the rest of the sequence.
 *   The flag belongs to the handle, not to a batch: with two batches in flight, one raised by the second may be read at the first's check,
 *   and then the batch IN FRONT of the one that left the range is recomputed too (its strict result is as valid; the harness does the same).
 *   The pop that delivers the last frame after pfnl_stream_end, pfnl_stream_reset and pfnl_stream_close put back what pfnl_get_option
 *   returned before (only the keys that were changed).  pfnl_stream_reset drops what was not popped and starts the next sequence.
 * Plain pfnl_forward calls on the handle remain possible between pushes: on the session's stream, or after synchronising it. */
typedef struct pfnl_stream pfnl_stream;
int pfnl_stream_open(pfnl_handle* h, int H, int W, int batch, void* hip_stream, pfnl_stream** out);
int pfnl_stream_push(pfnl_stream* s, const uint8_t* frame /*[H,W,3]*/, int is_device);
int pfnl_stream_end(pfnl_stream* s);
int pfnl_stream_ready(pfnl_stream* s, int* frames);
int pfnl_stream_pop(pfnl_stream* s, uint8_t* out /*[sH,sW,3]*/, int is_device, long long* index, int* got);
int pfnl_stream_reset(pfnl_stream* s);
int pfnl_stream_close(pfnl_stream* s);
int pfnl_stream_next_batch(int T, int batch, long long pushed, int ended, long long launched, long long* first, int* count);
/* SCENES (off by default; off, the session delivers what it always did).  A video has cuts, and a T-frame window across one mixes two
 * unrelated scenes in the non-local block and in conv10_i.  With scenes on, each scene is a sequence of its own: window c, slot t = frame
 * clamp(c + t - T/2, a, b), a = the first frame of c's scene, b = its last frame among those pushed - the rule of model/pfnl.py:238-242 with
 * the scene's ends in the place of 0 and `last` (stated once, on the host: pfnl_amd/scene.py).  Batches, the ring and the bound do not change.
 *   pfnl_stream_scenes: mode 0 off | 1 cuts marked by the caller | 2 marks and the detector: frame f >= 1 starts a scene when
 *     min(sad[f], |sad[f] - sad[f-1]|) >= ceil(threshold * H * W), sad[f] = the sum over the pixels of |Y(f) - Y(f-1)|,
 *     Y = (66 R + 129 G + 25 B + 128) >> 8, sad[0] = 0; threshold = a mean luma difference in (0, 255].  The second term keeps fast motion,
 *     flicker and the frame behind a cut from firing.  Accepted only while no frame of the current sequence has been pushed (else
 *     PFNL_ERR_STATE); the setting survives pfnl_stream_reset.  Modes 1 and 2 compute sad for every frame, on the device, in the ring,
 *     without a host round trip: on the session's stream for device-pointer pushes, on the copy's for host-pointer ones.
 *   pfnl_stream_mark_cut: the next pushed frame starts a scene.  PFNL_ERR_STATE in mode 0; before the first frame of a sequence it does
 *     nothing (frame 0 starts scene 0 anyway); pfnl_stream_reset clears it.
 *   pfnl_stream_pop_info: the first frame of the scene of the frame the last successful pop delivered, and that frame's sad (0, 0 in
 *     mode 0); PFNL_ERR_STATE before any pop of the sequence.  Both travel with the batch, so this call waits for nothing. */
int pfnl_stream_scenes(pfnl_stream* s, int mode, double threshold);
int pfnl_stream_mark_cut(pfnl_stream* s);
int pfnl_stream_pop_info(pfnl_stream* s, long long* scene_first, unsigned long long* sad);
/* YUV 4:2:0 (RGB24 by default; then the session is what it always was).  Decoders deliver NV12 or I420 and encoders take them back; with a
 * format set the session converts at its two edges, on the device, and everything between them - the ring, the scene sums, the windows, a
 * replay behind the range fence - goes on seeing RGB bytes.  The arithmetic is integer and stated once on the host, pfnl_amd/yuv.py:
 *   frames are tightly packed, H * W * 3 / 2 bytes: NV12 = Y [H][W], CbCr [H/2][W/2][2]; I420 = Y [H][W], Cb [H/2][W/2], Cr [H/2][W/2];
 *   coefficients of BT.601 or BT.709, limited (16..235 / 16..240) or full range, with 14 fractional bits, each rounded once
 *     (pfnl_yuv_coefficients: y0, then yr yg yb cbr cbg cbb crr crg crb, then dy drv dgu dgv dbu);
 *   chroma sited left (H.264 / HEVC type 0; SITING below names the others): in: 3 : 1 between the near and the far chroma row, 1 : 1 between two samples on odd columns,
 *     indices clamped; out: 1-2-1 over the two luma rows of the unrounded numerators, columns clamped, one rounding.
 *   pfnl_stream_format: in_fmt for push (H*W*3/2 bytes, converted into the frame's ring slot: a device pointer on the session's stream, a
 *     host pointer through a staging buffer on the copy's, before push returns), out_fmt for pop (sH*sW*3/2 bytes = the conversion of the
 *     RGB frame it would have delivered, made per batch behind the quantisation, recomputed batches included).  The two are independent;
 *     (RGB24, RGB24) is the default again.  Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE);
 *     the setting survives pfnl_stream_reset.  Allocates its staging on first use (PFNL_ERR_NOMEM); pfnl_stream_close frees it.
 * 10 BITS OUT (off by default; a session that sets none of these runs the launches it always ran).  The network's result is fp32 and a 4 x
 * upscale turns one-level steps of the LR frames into ramps that 8 bits do not resolve; HEVC Main10 and AV1 encoders take P010.  With
 * out_fmt = PFNL_PIX_RGB10, PFNL_PIX_P010 or PFNL_PIX_I010 the session quantises each batch to round(clip(sr * 1023, 0, 1023)) (the float32
 * product, half to even) and runs the resampler and the 4:2:0 conversion on those values: samples are little-endian uint16, pop copies
 * twice the bytes and takes the same uint8_t* (2-byte aligned).  The arithmetic is stated once on the host, pfnl_amd/depth10.py:
 *   RGB10 = [H][W][3], values 0 .. 1023; P010 = Y [H][W], CbCr [H/2][W/2][2], every sample value << 6; I010 (yuv420p10le) = Y, Cb, Cr,
 *     every sample the value itself; limited range is 64 .. 940 / 64 .. 960 (pfnl_yuv10_coefficients: y0, then the nine encode integers);
 *   the output size uses pfnl_resize_taps' tables with h = (sum c p + 2^9) >> 10 and clip((sum c h + 2^17) >> 18, 0, 1023);
 *   the input side (RGB24, NV12, I420), scenes, the push bound, reset and the replay behind the range fence are what they are at 8 bits.
 *   As in_fmt the three are PFNL_ERR_INVALID (10-bit input is a setting of its own, 10 BITS IN below: in_fmt names the layout), and so is
 *   RGB10 out of a YUV in_fmt.
 *   The 16-bit output slots are allocated by the call that sets the format (PFNL_ERR_NOMEM) and freed by pfnl_stream_close.
 * Out of scope: 12 and 16 bits, sitings beyond SITING's three, transfer functions, BT.2020 (4:2:2 and 4:4:4: CHROMA FORMAT below). */
enum { PFNL_PIX_RGB24 = 0, PFNL_PIX_NV12 = 1, PFNL_PIX_I420 = 2, PFNL_PIX_RGB10 = 3, PFNL_PIX_P010 = 4, PFNL_PIX_I010 = 5 };
enum { PFNL_MATRIX_BT601 = 0, PFNL_MATRIX_BT709 = 1 };
int pfnl_stream_format(pfnl_stream* s, int in_fmt, int out_fmt, int matrix, int full_range);
int pfnl_yuv_coefficients(int matrix, int full_range, int32_t out[15]);    /* y0, 9 encode, 5 decode; no device needed */
int pfnl_yuv10_coefficients(int matrix, int full_range, int32_t out[10]);  /* y0, 9 encode, for 10-bit samples; no device needed */
/* 10 BITS IN (additions to version 4; 8 by default, and a session that never calls pfnl_stream_input_depth, or sets 8, issues the launches
 * it always issued).  HEVC Main10, AV1 and UHD sources are 10-bit; cut to 8 bits ahead of the network, a 10-bit out_fmt only widens what
 * was already truncated.  The depth of the input is a setting of its own: in_fmt keeps naming the LAYOUT, and pfnl_stream_input_depth(s, 10)
 * says that its samples are little-endian uint16 in the conventions of the three 10-bit output formats:
 *   in_fmt RGB24 = the RGB10 layout, [H][W][3] values 0 .. 1023; NV12 = P010, the value in the upper ten bits; I420 = I010, the value itself.
 *   The session is lenient where a decoder's memory is not: P010's low six bits are ignored, an I010 / RGB10 sample above 1023 counts as
 *   1023 (pfnl_amd/depth10.py values10) - no kernel multiplies or indexes with an unclamped sample.
 *   push and push_surface take such frames (push keeps its const uint8_t*, 2-byte aligned, as pop does for 16-bit output; surfaces are
 *     checked with the 16-bit layout's geometry).  The ring becomes [cap][H][W][3] uint16 and the YUV staging frame doubles; they are
 *     allocated by whichever of pfnl_stream_input_depth and pfnl_stream_format comes second (PFNL_ERR_NOMEM: nothing half-made stays and
 *     the setting is unchanged); pfnl_stream_close frees everything.
 *   P010 / I010 are decoded straight into the ring slot by the one conversion kernel on uint16 samples (pfnl_amd/depth10.py to_rgb10:
 *     pfnl_yuv10_decode_coefficients' integers, chroma offset 512, clip at 1023; sitings as at 8 bits): a device pointer on the session's
 *     stream, a host pointer through the staging frame on the copy stream.  The windows are u10 / 1023. - the division in double,
 *     rounded once to fp32 (depth10.py dequantise10) - gathered from the 16-bit ring, recomputed batches included.  The scene sums use
 *     (66 R + 129 G + 25 B + 512) >> 10, luma on the 8-bit scale (pfnl_amd/scene.py luma_u10): thresholds and pfnl_stream_pop_info's sad
 *     keep their meaning and magnitude.  Everything behind the windows - forward, ensemble, tiles, quantisation, the output route - is
 *     untouched, and any out_fmt is allowed under pfnl_stream_format's rule (RGB10 out still goes with the RGB layout in).
 *   Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); any value but 8 or 10 is PFNL_ERR_INVALID
 *     before any HIP call; the setting survives pfnl_stream_reset and pfnl_stream_format.
 * Out of scope: 12 and 16 bits, 4:2:2 / 4:4:4, BT.2020 and transfer functions, the 10-bit names as in_fmt. */
int pfnl_stream_input_depth(pfnl_stream* s, int bits);   /* 8 (default) | 10 */
int pfnl_yuv10_decode_coefficients(int matrix, int full_range, int32_t out[6]);  /* y0, dy, drv, dgu, dgv, dbu; no device needed */
/* OUTPUT SIZE (off by default; then the session is what it always was).  The network's factor is fixed and display and encode rasters are
 * not (480p -> 1080p is 2.25 x, 720p -> 2160p is 3 x): with a size set the session resamples each batch's uint8 RGB frames on the device,
 * behind the quantisation and ahead of the YUV conversion, so a delivered frame is a pure function of the bytes the plain session
 * delivers.  The arithmetic is integer and stated once on the host, pfnl_amd/resize.py: a separable Keys cubic (a = -1/2) whose support
 * widens by in / out when the raster shrinks; per axis and output index a run of taps with 14 fractional bits that sums to 2^14 exactly,
 * indices clamped to the frame; horizontal pass first, h = (sum c p + 2^7) >> 8, unclipped; then clip((sum c h + 2^19) >> 20, 0, 255).
 *   pfnl_stream_resize: pop delivers out_H x out_W pixels (out_H*out_W*3 samples, or *3/2 in a 4:2:0 output format: then both must be even -
 *     whichever of pfnl_stream_resize and pfnl_stream_format comes second checks against the other's setting, PFNL_ERR_INVALID); 0, 0 is off.
 *     Per axis ceil(n_in / 4) <= n_out <= 2 n_in with n_in = scale * H or scale * W, and n_in, n_out <= 16384, else PFNL_ERR_INVALID.
 *     Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); the setting survives pfnl_stream_reset.
 *     Builds and uploads the tap tables and allocates the resized batches (PFNL_ERR_NOMEM: nothing half-made stays and the setting is
 *     unchanged); recomputed batches take the same route; pfnl_stream_close frees everything.
 *   pfnl_resize_max_taps / pfnl_resize_taps: one axis of the table, in exact integers, no device needed: output o =
 *     sum over k < count[o] of coef[o * ntaps + k] * in[first[o] + k] / 2^14; coef is [n_out][ntaps], zero behind count[o], with ntaps the
 *     longest run, as pfnl_resize_max_taps reports it.  Sizes outside the limits above and NULL: PFNL_ERR_INVALID.
 * Out of scope: other filters, resampling ahead of the quantisation, the input side (crop, letterbox and aspect fit: PLACEMENT below). */
int pfnl_stream_resize(pfnl_stream* s, int out_H, int out_W);
int pfnl_resize_max_taps(int n_in, int n_out, int* ntaps);
int pfnl_resize_taps(int n_in, int n_out, int32_t* first /*[n_out]*/, int32_t* count /*[n_out]*/, int16_t* coef /*[n_out][ntaps]*/);
/* PLACEMENT (additions to version 4; off by default, and a session that does not call pfnl_stream_place issues the launches it always
 * issued).  pfnl_stream_resize stretches the whole SR raster onto the whole output raster; where the two aspect ratios differ a frame
 * wants a crop, bars, or both.  With a placement the session resamples the rectangle `src` of the network's raster (scale*H x scale*W)
 * into the rectangle `dst` of a canvas of out_H x out_W and writes fill_rgb everywhere else, in the one launch that is stage 1 of the
 * output route, at 8 and at 10 bits: every sample of the canvas is written once - no memset, no cropped copy, no second launch.  The rule
 * is stated once on the host, pfnl_amd/fit.py place: the canvas = fill, with the resize of pfnl_stream_resize (pfnl_amd/resize.py; at 10
 * bits pfnl_amd/depth10.py) of the source rectangle ALONE written at dst - taps clamp at the edges of `src`, no pixel outside it reaches
 * the output.  The tables are pfnl_resize_taps(src.w, dst.w) and (src.h, dst.h).  A rectangle is y, x, h, w in pixels.
 *   pfnl_stream_place: src NULL = the whole raster, dst NULL = the whole canvas, fill_rgb NULL = black; at 10 bits a fill value v becomes
 *     (v << 2) | (v >> 6).  A 4:2:0 out_fmt converts the canvas as it converts any frame (an even canvas, as for pfnl_stream_resize; the
 *     rectangles need not be even; black bars leave as Y 16 / 64, chroma 128 / 512).  out_H = out_W = 0 with all pointers NULL is off; a size
 *     with src and dst NULL - or covering raster and canvas - is pfnl_stream_resize(s, out_H, out_W), the same launches; each of the two
 *     calls replaces what the other set.  Rectangles have h, w >= 1 and lie inside their rasters, per axis ceil(src / 4) <= dst <= 2 src,
 *     raster and canvas <= 16384: else PFNL_ERR_INVALID, the message naming src or dst (pfnl_amd/csrc/stream_route.h place_refused states
 *     the check once, before any HIP call and any change to the session).  State, reset, PFNL_ERR_NOMEM, recomputed batches, pop,
 *     pfnl_stream_pop_surface and pfnl_stream_format called later: as for pfnl_stream_resize, with the canvas as the output size.
 *   Aspect rules ("contain", "cover", a sample aspect ratio) are integer arithmetic on the host: pfnl_amd/fit.py rects; this interface
 *     takes rectangles only.
 * Out of scope: rotation and flips, cropping the input side, more than one picture on a canvas. */
typedef struct pfnl_rect {
    int32_t y, x, h, w;
} pfnl_rect;
int pfnl_stream_place(pfnl_stream* s, int out_H, int out_W, const pfnl_rect* src, const pfnl_rect* dst, const uint8_t fill_rgb[3]);
/* SURFACES (additions to version 4; a session that calls neither function issues the launches and copies it always issued).  A hardware
 * decoder or encoder hands out no packed frame: a surface is a pointer per plane and a row pitch per plane, rounded up to 64 or 256 bytes,
 * with a coded height above the displayed one, so that CbCr does not start at Y + H * W.  pfnl_stream_push_surface and
 * pfnl_stream_pop_surface are pfnl_stream_push and pfnl_stream_pop with the frame described that way, in the session's in_fmt and, for
 * pop, its out_fmt and output size; a sequence may mix them with the packed calls, and every state rule is theirs (ended, "pop first",
 * marks, the scene decision, the range check and the replay, pfnl_stream_pop_info, *got = 0).
 *   planes of a frame of H x W, b = 1 byte per sample, 2 for RGB10 / P010 / I010:
 *     RGB24 / RGB10: plane[0] = H rows of 3 W b bytes;  NV12 / P010: plane[0] = Y, H rows of W b, plane[1] = CbCr, H/2 rows of W b;
 *     I420 / I010: plane[0] = Y, H rows of W b, plane[1] = Cb and plane[2] = Cr, H/2 rows of W/2 b each.  Entries past those are ignored.
 *   the planes a format needs are non-NULL, all host pointers (is_device = 0) or all device pointers; pitch >= the bytes of a row; with
 *     16-bit samples pointers and pitches are even.  Anything else is PFNL_ERR_INVALID (the message names the plane or the pitch) before
 *     any HIP call and before any change to the session: pfnl_amd/csrc/surface_geom.h states the check once.
 *   push, device pointers: NV12 / I420 are read in place by the one conversion kernel, on the session's stream, straight into the ring slot
 *     (no staging pass; 16-byte words where W, every plane and every pitch are multiples of 16 - 8 for I420's chroma -, 4-byte words for
 *     multiples of 4 - 2 -, else single bytes); RGB24 is one hipMemcpy2DAsync.  Host pointers: one pitched copy per plane on the copy
 *     stream, YUV through the packed staging frame and the kernel; the caller's memory is free on return.
 *   pop: the batch has been converted into its packed slot as ever; delivery is one hipMemcpy2DAsync per plane out of it (device pointers:
 *     on the session's stream; host pointers: on the copy stream, complete on return).  Only the bytes of each row are written: what lies
 *     between a row's end and the pitch is never touched.
 *   a window of a larger surface needs no argument of its own: point plane[] at the first displayed sample (x and y even, so that the
 *     chroma pointers are whole samples) and keep the surface's pitch - the frame is then that window, and chroma clamps at its edges.
 * Out of scope: conversion kernels that write into the caller's surface (the conversion runs per batch, before a destination is known),
 * odd sizes (crop and letterbox: PLACEMENT above puts the frame on a canvas before it is delivered). */
typedef struct pfnl_surface {
    void*  plane[3];   /* RGB24 / RGB10: [0].  NV12 / P010: Y, CbCr.  I420 / I010: Y, Cb, Cr.  Unused entries are ignored. */
    size_t pitch[3];   /* bytes from one row of that plane to the next */
} pfnl_surface;
int pfnl_stream_push_surface(pfnl_stream* s, const pfnl_surface* frame, int is_device);
int pfnl_stream_pop_surface(pfnl_stream* s, const pfnl_surface* out, int is_device, long long* index, int* got);
/* SITING (additions to version 4; a session that does not call pfnl_stream_chroma_siting issues the launches it always issued and
 * delivers the same bytes).  4:2:0 streams differ in where a chroma sample sits among its four luma pixels, and converting with the
 * wrong assumption shifts the colour by half a luma pixel - two pixels after a 4 x upscale.  Chroma sample (j, i) sits at the luma
 * coordinates (row, column):
 *   PFNL_SITING_LEFT    (2j + 1/2, 2i)        H.264 / HEVC type 0, MPEG-2, Y4M C420mpeg2: the default, and the rule stated above;
 *   PFNL_SITING_CENTER  (2j + 1/2, 2i + 1/2)  JPEG, MPEG-1, Y4M C420jpeg;
 *   PFNL_SITING_TOPLEFT (2j, 2i)              HEVC type 2 (UHD), Y4M C420paldv.
 * Per axis a siting is midway (the vertical axis of LEFT, both of CENTER) or co-sited.  The rule is stated once on the host,
 * pfnl_amd/yuv.py upsample / encode_filter (10 bits: pfnl_amd/depth10.py):
 *   in: per axis two taps in quarters, chroma indices clamped - midway: near = j, far = j + 1 on odd and j - 1 on even luma indices,
 *     3 : 1; co-sited: near = j, far = j + 1, 4 : 0 on even and 2 : 2 on odd indices; the sample is (sum wy wx C + 8) >> 4;
 *   out: the unrounded numerators filtered per axis, indices clamped - midway: a box over 2j, 2j + 1 (k = 1); co-sited: 1-2-1 over
 *     2j - 1, 2j, 2j + 1 (k = 2) - and one rounding by 14 + k bits, k summed over both axes: 3 for LEFT, 2 for CENTER, 4 for TOPLEFT.
 *   pfnl_stream_chroma_siting: in_siting for what push takes, out_siting for what pop delivers, each used where that edge is 4:2:0 and
 *     ignored by an RGB edge; the surface calls follow them.  NULL and a value outside the enum: PFNL_ERR_INVALID, before any HIP call.
 *     Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); the setting survives pfnl_stream_reset
 *     and pfnl_stream_format.  It allocates nothing: the siting is an argument of the edge's one conversion launch.
 * Out of scope: HEVC types 1, 3, 4 and 5, sitings that differ between Cb and Cr. */
enum { PFNL_SITING_LEFT = 0, PFNL_SITING_CENTER = 1, PFNL_SITING_TOPLEFT = 2 };
int pfnl_stream_chroma_siting(pfnl_stream* s, int in_siting, int out_siting);
/* CHROMA FORMAT (additions to version 4).  The pixel formats name a LAYOUT - semi-planar (NV12 / P010) or planar (I420 / I010) - and a
 * sample depth; how the chroma planes are subsampled is a value of its own, and 4:2:0 is what every entry without that value means:
 *   PFNL_CHROMA_420  chroma planes of H/2 rows of W/2 samples: everything stated above;
 *   PFNL_CHROMA_422  H rows of W/2 samples.  NV12 -> NV16 = Y [H][W], CbCr [H][W/2][2]; I420 -> I422 = Y, Cb [H][W/2], Cr; P010 -> P210
 *                    (every value << 6); I010 -> yuv422p10le.  2 H W samples a frame; W even and >= 2, H >= 1;
 *   PFNL_CHROMA_444  H rows of W samples.  NV24 = Y [H][W], CbCr [H][W][2]; I444 = three planes [H][W]; P410; yuv444p10le.  3 H W samples;
 *                    any H, W >= 1.
 * The rule is SITING's, applied per axis, and an axis that is not subsampled takes no filter at all (pfnl_amd/yuv.py, pfnl_amd/depth10.py
 * with chroma = "422" | "444"): in, 4:2:2: (w_near C[near] + w_far C[far] + 2) >> 2 with the horizontal taps of the siting, 4:4:4: the
 * sample itself; out, 4:2:2: the box (k = 1) or 1-2-1 (k = 2) across and one rounding by 14 + k bits, 4:4:4: (N + 2^13) >> 14.  Of a siting
 * only the horizontal axis is read at 4:2:2 - LEFT and TOPLEFT are one rule there, CENTER the midway one - and nothing at 4:4:4.  Matrix
 * and range coefficients are untouched.  A lane converts one luma row by 16, 4 or single pixels (10 bits: 8 or single), in 16-byte words
 * where the width and every pointer, pitch and frame stride allow (pfnl_amd/csrc/yuv_chroma.hip).
 *   pfnl_stream_chroma_format: in_chroma for what push takes, out_chroma for what pop delivers, each used where that edge's format is a
 *     YUV layout and ignored by an RGB edge, as the siting is; push / pop and the surface calls follow it (frame sizes and planes as
 *     above), and so does every combination a session allows with a YUV edge - 10 bits in and out, scenes, resize, place, ensemble,
 *     tiling.  It follows pfnl_stream_input_depth's rules of order: whichever of it and pfnl_stream_format / pfnl_stream_resize /
 *     pfnl_stream_place comes later checks against the other's setting and allocates the staging whose size depends on both; accepted
 *     only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); it survives pfnl_stream_reset and
 *     pfnl_stream_format; a failed call leaves the session as it was; NULL and a value outside the enum: PFNL_ERR_INVALID before any
 *     HIP call.  A session that never calls it, or sets 420 / 420, issues exactly the launches it always issued.
 *     The output size (and a canvas) is even along the axes the output subsampling halves: both at 4:2:0, the width at 4:2:2, none at
 *     4:4:4.  Nothing behind the ring or ahead of the quantisation changes.
 * The op hooks pfnl_op_*_chroma below are the two kernels on their own.
 * Out of scope: monochrome, 4:1:1, alpha planes, 12 and 16 bits, BT.2020. */
enum { PFNL_CHROMA_420 = 0, PFNL_CHROMA_422 = 1, PFNL_CHROMA_444 = 2 };
int pfnl_stream_chroma_format(pfnl_stream* s, int in_chroma, int out_chroma);
/* PACKED FORMATS (additions to version 4).  What a capture card, an SDI card or a swap chain hands over is ONE plane whose samples are
 * interleaved within a pixel or a pixel group.  A packing is a setting per side of its own, beside layout, depth, chroma format and siting;
 * PFNL_PACK_NONE is the planes of the layout, and the PFNL_PIX_* enum does not grow.  Each other value names one complete single-plane
 * layout and is valid only on a side whose family, depth and chroma format agree with it:
 *   value               side must be            unit                                                         bytes of a row
 *   PFNL_PACK_BGR24     RGB, 8 bits             3 bytes B, G, R                                              3 W
 *   PFNL_PACK_RGBA      RGB, 8 bits             4 bytes R, G, B, A                                           4 W
 *   PFNL_PACK_BGRA      RGB, 8 bits             4 bytes B, G, R, A                                           4 W
 *   PFNL_PACK_YUYV      YUV, 8 bits, 4:2:2      4 bytes Y0 Cb Y1 Cr per pixel pair (YUY2)                    2 W
 *   PFNL_PACK_UYVY      YUV, 8 bits, 4:2:2      4 bytes Cb Y0 Cr Y1                                          2 W
 *   PFNL_PACK_X2RGB10   RGB, 10 bits            one little-endian uint32: bits 29..20 R, 19..10 G, 9..0 B    4 W
 *   PFNL_PACK_X2BGR10   RGB, 10 bits            uint32: bits 29..20 B, 19..10 G, 9..0 R (DXGI R10G10B10A2)   4 W
 *   PFNL_PACK_Y210      YUV, 10 bits, 4:2:2     four uint16 Y0 Cb Y1 Cr, the value in the upper ten bits     4 W
 *   PFNL_PACK_V210      YUV, 10 bits, 4:2:2,    16 bytes per 6 pixels: four little-endian uint32 of three    16 W / 6
 *                       W a multiple of 6       10-bit samples at bits 9..0, 19..10, 29..20 - word 0: Cb0 Y0 Cr0; 1: Y1 Cb1 Y2;
 *                                               2: Cr1 Y3 Cb2; 3: Y4 Cr2 Y5
 * A tightly packed frame is H rows of the row bytes, except v210, whose rows are ((W + 47) / 48) * 128 bytes (the format's own rule).
 * "Side must be" is read from what is set: the input side's in_fmt family and pfnl_stream_input_depth, the output side's out_fmt (which
 * carries its depth), and PFNL_CHROMA_*.  A YUV layout name on a packed side only says the side is YUV.
 * Alpha and the spare bits of an X2 word are ignored on input and written opaque (255; 3 in the two bits); bits 31..30 of a v210 word and
 * the padding of a tight v210 row are written 0 and ignored on input; bytes between a row's end and the pitch of a caller's surface are
 * never written.  Sample values pass as they come, 0 .. 1023 at 10 bits, with no clamp to a legal range.  A 4:2:2 packing reads the
 * horizontal half of the side's siting exactly as planar 4:2:2 does; matrix and range are the session's.  The arithmetic is CHROMA FORMAT's
 * at PFNL_CHROMA_422 and nothing else: a packed frame equals pack(planar result) byte for byte (pfnl_amd/packed.py).  A lane converts one
 * row by the pixels of one 16-byte word of the packed side, or by one unit where the addresses do not allow that (pfnl_amd/csrc/packed.hip).
 *   pfnl_stream_packing: in_pack for what push takes, out_pack for what pop delivers.  A value outside the enum, or a packing that
 *     disagrees with its side as it is set at the call (the words name family, depth, chroma format or the width): PFNL_ERR_INVALID
 *     before any HIP call.  Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); it survives
 *     pfnl_stream_reset.  With a packing in force pfnl_stream_format, pfnl_stream_input_depth, pfnl_stream_chroma_format and the size
 *     setters refuse a change that contradicts it (PFNL_ERR_INVALID: set PFNL_PACK_NONE first).  push / pop move tightly packed frames;
 *     the surface calls use plane[0] / pitch[0], pointer and pitch multiples of 2 (y210) or 4 (x2rgb10, x2bgr10, v210).  On input every
 *     packed side goes through the kernel, on output the packing is stage 2 of the route, for the RGB packings too.  A session that
 *     never calls it issues exactly the launches it always issued.
 * The op hooks pfnl_op_packed_to_rgb_* / pfnl_op_rgb_to_packed_* below are the two kernels on their own.
 * Out of scope: big-endian variants, 12 and 16 bits, packed 4:4:4, alpha carried through, BT.2020, v210 widths not a multiple of 6. */
enum {
    PFNL_PACK_NONE = 0, PFNL_PACK_BGR24 = 1, PFNL_PACK_RGBA = 2, PFNL_PACK_BGRA = 3, PFNL_PACK_YUYV = 4, PFNL_PACK_UYVY = 5,
    PFNL_PACK_X2RGB10 = 6, PFNL_PACK_X2BGR10 = 7, PFNL_PACK_Y210 = 8, PFNL_PACK_V210 = 9
};
int pfnl_stream_packing(pfnl_stream* s, int in_pack, int out_pack);
/* INTERLACED (additions to version 4; a session that does not call pfnl_stream_interlace, or sets PFNL_INTERLACE_OFF, issues the launches
 * it always issued).  What an SDI card, a DVD or a broadcast archive delivers is woven: a frame of H rows (H even) is two fields of H / 2
 * rows taken at two instants - the top field (parity 0) rows 0, 2, ..., the bottom field (parity 1) rows 1, 3, ...  With the setting on
 * pushed frames are woven frames in the pushed layout, and progressive frames reach the ring; from the ring on nothing knows the frames
 * were interlaced.  The rule is stated once on the host, pfnl_amd/deinterlace.py; its index rules once in pfnl_amd/csrc/field_geom.h:
 *   fields: N frames are the fields k = 0 .. 2 N - 1 in time order; PFNL_FIELD_TFF: field 2 n is frame n's top field, 2 n + 1 its bottom
 *     field; PFNL_FIELD_BFF the other way round.  An index q outside [0, 2 N - 1] is replaced by q + 2 (q < 0) or q - 2: same parity.
 *   the progressive frame at the time of field k (parity p, samples A; P1, N1 = fields k -+ 1, P2, N2 = k -+ 2): row 2 i + p is A[i]; row
 *     2 j + (1 - p), with u = j - p and field rows clamped to [0, H / 2 - 1], per sample (no horizontal term; MAX = 255 | 1023):
 *       c = A[u], e = A[u + 1], s = clip((9 (c + e) - (A[u - 1] + A[u + 2]) + 8) >> 4, 0, MAX),  x = P1[j], y = N1[j], d = (x + y + 1) >> 1,
 *       diff = max((|x - y| + 1) >> 1, (|P2[u] - c| + |P2[u + 1] - e| + 1) >> 1, (|N2[u] - c| + |N2[u + 1] - e| + 1) >> 1),
 *       out = min(max(s, d - diff), d + diff): an exact weave where nothing moves, the field's own cubic within diff of d where it does.
 *   decoding: a field is a picture of H / 2 rows - rows p, p + 2, ... of every plane of the pushed frame - decoded by the launch that
 *     decodes a progressive frame of this setting, as a surface of H / 2 rows with every pitch doubled and the plane pointers advanced by
 *     p rows: no conversion kernel is added.  Only 4:2:0 filters vertically; there a field's chroma rows belong to that field, H is a
 *     multiple of 4, and a field's chroma is sited like a progressive picture's (the quarter-row offset of interlaced 4:2:0 is not modelled).
 *   pfnl_stream_interlace: mode PFNL_INTERLACE_FRAME - one ring frame per pushed frame, at the time of its first field - or
 *     PFNL_INTERLACE_FIELD - one per field, two per pushed frame -, PFNL_INTERLACE_OFF the session as it always was; field_order
 *     PFNL_FIELD_TFF | PFNL_FIELD_BFF.  A setting beside layout, depth, chroma format, siting and packing: accepted only while no frame of
 *     the current sequence has been pushed (else PFNL_ERR_STATE), it survives pfnl_stream_reset.  Unknown values, and 4:2:0 planes with
 *     H % 4 != 0, are PFNL_ERR_INVALID; whichever of this call, pfnl_stream_format and pfnl_stream_chroma_format comes second makes that
 *     check against the other's setting.  The first call that turns it on allocates the field store - three frames' decoded fields,
 *     [3][2][H/2][W][3] samples of the input depth, ahead of the ring; PFNL_ERR_NOMEM leaves nothing half-made and the setting unchanged;
 *     pfnl_stream_close frees it.
 *   latency: frame n becomes deinterlaceable when frame n + 1 has been pushed, or at pfnl_stream_end - ONE FRAME of latency.  Then one
 *     launch (pfnl_amd/csrc/deinterlace.hip) writes one ring frame or two straight into their ring slots, and each is admitted exactly as
 *     a progressive push admits a frame: the scene sum and decision behind it, the batches it completes.  Pop indices count progressive
 *     frames: N in frame mode, 2 N in field mode; pfnl_stream_ready, the batches, the range replay, ensemble, tiles and the output route
 *     are what they are.  Every push path is taken: push and push_surface, host and device pointers (they may alternate), 8 and 10 bits,
 *     RGB, NV12 / I420 at the three chroma formats, every packing.  A device-pointer push decodes and deinterlaces on the session's stream;
 *     a host-pointer push does both on the copy stream before it returns.
 *   the bound: a push that cannot admit every ring frame it completes returns PFNL_ERR_STATE ("pop first") and changes nothing - the
 *     pushed frame is not stored, no counter moves; pfnl_stream_end first admits the held frame under the same bound, and a refusal
 *     leaves the session un-ended.
 *   cuts: pfnl_stream_mark_cut marks the next pushed frame; the mark travels with that frame and lands on the first ring frame made from
 *     it.  pfnl_stream_reset forgets the field store's contents and a pending mark.  The deinterlacer itself reads no marks: across a cut
 *     the rule's own clamp widens (t0 and t1 are large) and the made rows are the field's own cubic.
 * The op hooks pfnl_op_deinterlace_u8 / _u10 below are the kernel on its own.
 * Out of scope: edge-directed interpolation, interlaced output, the interlaced 4:2:0 siting offset, marks read by the deinterlacer, 12 and
 * 16 bits.  (Film carried in fields - 3:2 pulldown - and streams that mix it with video: TELECINE below.) */
enum { PFNL_INTERLACE_OFF = 0, PFNL_INTERLACE_FRAME = 1, PFNL_INTERLACE_FIELD = 2 };
enum { PFNL_FIELD_TFF = 0, PFNL_FIELD_BFF = 1 };
int pfnl_stream_interlace(pfnl_stream* s, int mode, int field_order);
/* TELECINE (additions to version 4; a session that does not call pfnl_stream_telecine, or sets PFNL_TELECINE_OFF, issues the launches it
 * always issued).  Film carried at 29.97 frames a second is not interlaced video: it is 24 progressive frames a second spread over fields
 * by 3:2 pulldown, so two of every five pushed frames are woven from two different film frames and one picture in five is a repeat.  The
 * deinterlacer would interpolate half the rows of those frames and keep the repeat; the film frames are all in the stream, intact as field
 * pairs.  With this setting on, pushed frames are re-paired field by field ahead of the ring and, in mode DECIMATE, one frame in five is
 * dropped.  The rule is stated once on the host, pfnl_amd/telecine.py, in INTERLACED's vocabulary (fields k = 0 .. 2 N - 1 in time order
 * under field_order, the replacement at the ends, samples min(v, MAX), no horizontal term); its index rules once in
 * pfnl_amd/csrc/telecine_geom.h:
 *   matching: for pushed frame n the kept field is A = field 2 n, of parity p; its partner is field 2 n + 1 (candidate c: the frame as
 *     pushed) or field 2 n - 1 (candidate p; replaced at n = 0, where it becomes field 1 and c = p).  A film frame covers two or three
 *     consecutive fields, so one of the two always belongs to A's film frame, in every phase and either field order.
 *   the comb count of a candidate X: over every missing row j = 0 .. h - 1 (h = H / 2), u = j - p, field rows clamped to [0, h - 1], and
 *     every sample of the row: a = X[j] - A[u], b = X[j] - A[u + 1]; the sample is combed iff a b > T^2 - it lies on one side of both
 *     vertical neighbours by more than T; T = threshold at 8 bits, 4 threshold at 10.  An exact integer, at most h 3 W.
 *   the choice: the smaller count, c on a tie; the matched frame m_n is the weave of A and the chosen partner.  With post on, a frame whose
 *     smaller count exceeds comb_limit is video: m_n is then INTERLACED's frame at the time of field 2 n, byte for byte.
 *   pfnl_telecine_params: threshold (1 .. 255; default 10), post (0 | 1; default 1), comb_limit (default, and any negative value:
 *     (h 3 W) >> 8).  Parameters of the rule - chosen, not measured.
 *   decimation (PFNL_TELECINE_DECIMATE): D_n = sum |m_n - m_(n-1)| over all samples, D_0 the largest uint64.  Frames 5 q .. 5 q + 4, counted
 *     from the start of the sequence or the last reset, are cycle q; of a complete cycle the frame with the smallest D is dropped (the
 *     lowest index on a tie) and four are delivered in order; pfnl_stream_end delivers an incomplete last cycle whole.
 *     PFNL_TELECINE_MATCH delivers every m_n.
 *   pfnl_stream_telecine: a setting beside pfnl_stream_interlace and exclusive with it - whichever of the two is turned on while the other
 *     is on returns PFNL_ERR_INVALID.  Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); it
 *     survives pfnl_stream_reset.  Unknown values, odd H, 4:2:0 planes with H % 4 != 0 (checked by whichever of this call,
 *     pfnl_stream_format and pfnl_stream_chroma_format comes second) and, in mode DECIMATE, a ring that can never hold the four frames a
 *     cycle completes are PFNL_ERR_INVALID.  The first call that turns it on allocates INTERLACED's field store and, beside it, the five
 *     matched frames of a cycle, the device words of the decision and a pinned host copy of a cycle's D; PFNL_ERR_NOMEM leaves nothing
 *     half-made and the setting unchanged.
 *   latency: m_n exists once frame n + 1 has been pushed, or at pfnl_stream_end - INTERLACED's one frame, which post needs.  Per matched
 *     frame: the match launch, INTERLACED's launch into the frame's place (post on: the weave leaves it alone where the decision flags the
 *     frame), the weave launch, which reads the decision from device memory and in mode DECIMATE sums D_n in the same pass
 *     (pfnl_amd/csrc/telecine.hip).  No host round trip sits between the counts and the weave.  Mode MATCH writes m_n straight into its
 *     ring slot.  Mode DECIMATE keeps a cycle's matched frames beside the ring and admits its four kept frames together when the
 *     cycle's last matched frame exists: THE HOST WAITS ONCE PER CYCLE, and never per frame, for a pinned copy of the cycle's five D - on
 *     the session's stream for a device-pointer push, on the copy stream for a host-pointer push -, as it must know the drop index to place
 *     marks and to count pops.  A device-pointer push decodes the caller's frame on the session's stream, behind whatever is queued there,
 *     and the D follow from that frame: this wait therefore also waits for the forwards in flight on that stream, once in five pushes,
 *     where a host-pointer push waits for its own copy stream as every host-pointer push does.  Every push path INTERLACED takes is taken.
 *   the bound: INTERLACED's, applied to everything a push completes - up to four ring frames at the end of a cycle.  A refused push or
 *     pfnl_stream_end ("pop first", PFNL_ERR_STATE) changes nothing.
 *   cuts: the mark of pfnl_stream_mark_cut travels with its pushed frame and lands on the first delivered frame made from it, or from a
 *     later frame where its own is dropped.  Cycles do not restart at marks: the rate stays 4 / 5 throughout.
 *   pfnl_stream_telecine_stats: out[5] = frames matched c, matched p, post-processed (counted there and under neither match), dropped,
 *     and admitted to the ring, of the current sequence; it waits for the session's two streams.
 *   pfnl_telecine_deliverable: the ring frames a session in `mode` has made of `pushed` pushed frames; needs no device.
 * The op hooks pfnl_op_fieldmatch_* / pfnl_op_telecine_frame_* below are the kernels on their own.
 * Out of scope: soft-telecine flags (RFF: a demuxer's matter), cadences other than 3:2 (they pass through MATCH; DECIMATE drops one frame
 * in five whatever the cadence), interlaced output, the interlaced 4:2:0 siting offset. */
enum { PFNL_TELECINE_OFF = 0, PFNL_TELECINE_MATCH = 1, PFNL_TELECINE_DECIMATE = 2 };
typedef struct pfnl_telecine_params {
    int threshold;
    int post;
    long long comb_limit;
} pfnl_telecine_params;
int pfnl_stream_telecine(pfnl_stream* s, int mode, int field_order, const pfnl_telecine_params* params /* NULL: the defaults */);
int pfnl_stream_telecine_stats(pfnl_stream* s, long long out[5]);
int pfnl_telecine_deliverable(int mode, long long pushed, int ended, long long* frames);
/* COLOUR (additions to version 4; a session that does not call pfnl_stream_colour issues the launches it always issued).  SD material is
 * BT.601 in matrix and SMPTE-C or EBU in primaries; an HD stream is read as BT.709 in both.  pfnl_stream_format gives the session one
 * matrix and one range for both edges; with this setting each edge has its own colour description and the conversion between the two
 * runs on the device.  The rule is stated once on the host, pfnl_amd/colour.py; its integers once in pfnl_amd/csrc/colour_geom.h:
 *   matrix and range per side: the coefficients of YUV <-> RGB (pfnl_amd/yuv.py) are arguments of the two conversion launches; the decode
 *     reads the input side's, the output route's last stage the output side's.  No kernel and no memory depend on them.  On an RGB side
 *     they are accepted and ignored: RGB is full range.
 *   primaries per side (PFNL_PRIM_*; white D65 for all three, no chromatic adaptation): where the two ids differ, stage 0 of the output
 *     route - the launch that reads every fp32 result and writes every sample - is the colour kernel (pfnl_amd/csrc/colour.hip) in place
 *     of the plain quantisation: the same levels, rintf(clip(x TOP, 0, TOP)) with NaN -> 0, then per pixel
 *       out = E[clip((M . D[level] + 2^13) >> 14, 0, 65535)]
 *     with D[v] = floor(65535 f^-1(v / TOP) + 0.5), E[l] = floor(TOP f(l / 65535) + 0.5), f the BT.709 OETF, which all three systems share,
 *     and M = pfnl_colour_matrix(in, out): RGB -> XYZ of the input's primaries, XYZ -> RGB of the output's, in exact rationals, times
 *     2^14, rounded half away from zero, the diagonal taking each row's residual.  Rows sum to 2^14 and E[D[v]] = v, so greys pass
 *     untouched.  Everything behind stage 0 - resize, placement and its fill colour, YUV at every chroma format, siting and depth,
 *     packing - is untouched and sees RGB in the output's colours; a batch recomputed behind the range fence takes the same launch.
 *     The kernel keeps D and E in LDS (E as the code at the start of each 64-wide bucket of l and the thresholds: 3 KB at 8 bits, 6 KB
 *     at 10); they are uploaded once per device and process, by the first setting whose ids differ (PFNL_ERR_NOMEM: the setting is
 *     unchanged) or the first call of an op hook below, and are nobody's to free.
 *   pfnl_stream_colour: in / out NULL: that side keeps what it has.  pfnl_stream_format keeps its meaning and its domain: it sets matrix
 *     and range of both sides and leaves the primaries alone; each of the two calls replaces the matrix and range the other set.
 *     Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); it survives pfnl_stream_reset; a
 *     matrix other than 0 | 1, a full_range other than 0 | 1 and primaries outside the enum are PFNL_ERR_INVALID with the setting
 *     unchanged.
 *   pfnl_colour_matrix / pfnl_colour_tables (bits 8 | 10; decode [2^bits], encode [65536]): the integers themselves; they need no device
 *     and refuse bad arguments with PFNL_ERR_INVALID before anything else.
 * The op hooks pfnl_op_quantise_colour_* below are the kernel on its own.
 * Out of scope: BT.2020, PQ / HLG and tone mapping, chromatic adaptation, per-frame colour changes. */
enum { PFNL_PRIM_BT709 = 0, PFNL_PRIM_BT601_525 = 1, PFNL_PRIM_BT601_625 = 2 };
typedef struct pfnl_colour {
    int matrix;
    int full_range;
    int primaries;
} pfnl_colour;
int pfnl_stream_colour(pfnl_stream* s, const pfnl_colour* in, const pfnl_colour* out /* NULL: that side keeps what it has */);
int pfnl_colour_matrix(int src, int dst, int32_t out[9]);
int pfnl_colour_tables(int bits, uint16_t* decode, uint16_t* encode /* [65536] */);
/* SELF-ENSEMBLE in a session (additions to version 4; a session that does not call this issues the launches it always issued).  With
 * n in {2, 4, 8} the one forward of every batch is pfnl_forward_ensemble(..., n, ...) (SELF-ENSEMBLE above); gather, quantisation, the
 * output route, scenes and the replay behind the range fence are untouched, and a recomputed batch goes through the same call.  n = 1 is
 * off; any other n is PFNL_ERR_INVALID.  Accepted only while no frame of the current sequence has been pushed (else PFNL_ERR_STATE); the
 * setting survives pfnl_stream_reset. */
int pfnl_stream_ensemble(pfnl_stream* s, int n);
/* TILES in a session (additions to version 4; a session that does not call this issues the launches it always issued).  With a tiling
 * set the one forward of every batch is pfnl_forward_tiled(..., t, the session's ensemble, ...) (TILES above); gather, quantisation, the
 * output route, scenes and the replay behind the range fence are untouched, and a recomputed batch goes through the same call.  t == NULL
 * is off; a tiling that does not fit the session's H x W is PFNL_ERR_INVALID.  Accepted only while no frame of the current sequence has
 * been pushed (else PFNL_ERR_STATE); the setting survives pfnl_stream_reset. */
int pfnl_stream_tile(pfnl_stream* s, const pfnl_tiling* t);
/* BARS (additions to version 4; a session that does not call pfnl_stream_bars, or sets mode 0, issues the launches it always issued).  A
 * letterboxed or pillarboxed frame carries its picture between black bars; this measures where the picture is, on the device, where the
 * frames already are.  The rule is stated once on the host, pfnl_amd/bars.py; its integer steps once in pfnl_amd/csrc/bars_geom.h:
 *   luma: the scene sums' - integer BT.601 on the 8-bit scale without its + 16 (black 0, white 219 | 220) at either depth.
 *   rows[y] = the sum of luma along row y, cols[x] along column x: exact integers, below 2^32 for H, W <= 16384.
 *   row y is picture iff rows[y] > limit W, column x iff cols[x] > limit H (limit 0 .. 219; 8 is ffmpeg cropdetect's 24 on a Y from 16).
 *   box = (y0, x0, h, w) from the first to the last picture row and column, whatever lies between; (0, 0, 0, 0) with no picture row or column.
 *   the kernel (pfnl_amd/csrc/bars.hip): one launch for all frames of a call; a workgroup sums a strip of whole rows, column sums leave it
 *     as one 32-bit add per column and strip, and the workgroup that finishes a frame last scans both arrays and writes the box.  It
 *     reads every sample once, in 16-byte words where the rows allow (W a multiple of 16, of 8 at 10 bits, and the pointer aligned), else
 *     in 4-byte words or single samples, and leaves its scratch words zero for the next launch.
 *   pfnl_stream_bars: mode 0 off (the default), mode 1: every ring frame is measured as it is admitted - behind the decode, the
 *     deinterlacer or inverse telecine, on the stream that made it - with `limit` (ignored in mode 0).  Accepted only while no frame of the
 *     current sequence has been pushed (else PFNL_ERR_STATE); it survives pfnl_stream_reset; a mode other than 0 | 1 or a limit outside
 *     0 .. 219 is PFNL_ERR_INVALID.  The first call that turns it on allocates the boxes of the ring's slots, the kernel's scratch and
 *     two pinned host copies; PFNL_ERR_NOMEM leaves nothing half-made and the setting unchanged.
 *   pfnl_stream_pop_box: the box of the frame the last successful pop delivered.  The boxes travel with the batch as
 *     pfnl_stream_pop_info's values do: the call waits for nothing.
 *   pfnl_stream_content_box: the union of the boxes of the frames popped so far in the sequence, and their number.
 *     Both: PFNL_ERR_STATE in mode 0 or before any frame of the sequence has been popped.
 * The op hooks pfnl_op_content_box_u8 / _u10 below are the kernel on its own.
 * Out of scope: acting on a box that changes inside a sequence, a crop decided inside the session (python -m pfnl_amd.upscale --crop
 * opens the session at the cropped size), windowboxed material whose rows the pillars dilute below the limit. */
int pfnl_stream_bars(pfnl_stream* s, int mode, int limit);
int pfnl_stream_pop_box(pfnl_stream* s, int32_t box[4]);
int pfnl_stream_content_box(pfnl_stream* s, int32_t box[4], long long* frames);

/* Page-locked host buffers (hipHostMalloc / hipHostFree) for the tensors a caller hands to a host-pointer pfnl_forward - the call that
 * replaces sess.run(SR_test, feed_dict={L_test: ...}) (reference model/pfnl.py:252,309): the copy engine then moves them directly, with
 * no staging copy through the handle's strips.  Process-wide, not tied to a handle; pfnl_amd/engine.py keeps a small, size-capped pool of
 * them for the arrays PFNLEngine.forward returns (no torch involved: ADVICE r4). */
int pfnl_host_alloc(size_t bytes, void** out);
int pfnl_host_free(void* p);

/* ---- multi-GPU (RCCL over xGMI) ------------------------------------ */
/* Clips are independent (reference model/pfnl.py:44,55: the batch is only the leading dimension), so ranks share NOTHING on
 * the data path; these entry points carry what the reference's single-GPU session (main.py:10) has no counterpart for:
 * the weight replica, the statistics, and an optional gather.  RCCL is loaded at run time (dlopen; PFNL_RCCL_LIB overrides
 * the search) - a single-GPU caller never needs it.  One communicator per process: rank 0 calls pfnl_comm_get_unique_id,
 * moves the PFNL_COMM_ID_BYTES bytes to the other ranks through any host channel, every rank calls pfnl_comm_init_rank
 * (collective).  One process driving several devices: pfnl_comm_init_all (comms[i] on devs[i], devs NULL = 0..ndev-1). */
typedef struct pfnl_comm pfnl_comm;
#define PFNL_COMM_ID_BYTES 128
enum { PFNL_COMM_SUM = 0, PFNL_COMM_MAX = 1 };
int pfnl_comm_get_unique_id(void* id /*[PFNL_COMM_ID_BYTES]*/);
int pfnl_comm_init_rank(int nranks, int rank, const void* id, int device_id, pfnl_comm** out);
int pfnl_comm_init_all(int ndev, const int* devs, pfnl_comm** comms /*[ndev]*/);
int pfnl_comm_destroy(pfnl_comm* c);
/* (rank, nranks) as RCCL itself reports them for this communicator (ncclCommUserRank / ncclCommCount when the library exports them; they
 * must equal what the communicator was created with, else PFNL_ERR_COMM): bench.py prints them as config.comm_nranks. */
int pfnl_comm_rank(pfnl_comm* c, int* rank, int* nranks);
/* ncclBroadcast of the packed DEVICE weight blobs of `h` (what pfnl_finalize_weights built on `root`) to every rank's
 * handle of the same geometry; a non-root handle needs no pfnl_set_weight calls at all.  Replaces nothing in the reference
 * (tf.train.Saver.restore per process, model/base_model.py:231-243): one read of the checkpoint instead of one per GPU. */
int pfnl_comm_bcast_weights(pfnl_comm* c, pfnl_handle* h, int root);
/* The same replica without a communicator: the packed device blobs of `src` copied into `dst` (same geometry; same device or a
 * peer-accessible one - hipMemcpyDefault).  `dst` needs no pfnl_set_weight calls.  For several handles per process (one per
 * stream or per device) fed from one checkpoint read; also what the receive side of the broadcast is tested with on one GPU. */
int pfnl_copy_weights(pfnl_handle* dst, pfnl_handle* src);
int pfnl_comm_bcast(pfnl_comm* c, void* dev_buf, size_t bytes, int root);                 /* in place, synchronous */
/* all-reduce of n <= 64 HOST doubles in place (squared error / frame counts: PFNL_COMM_SUM; elapsed time: PFNL_COMM_MAX) */
int pfnl_comm_allreduce_f64(pfnl_comm* c, double* vals, int n, int op);
int pfnl_comm_barrier(pfnl_comm* c);
/* gather of equal per-rank shards of SR frames (device pointers): recv_dev [nranks][count_per_rank]; stream NULL = synchronous */
int pfnl_comm_allgather(pfnl_comm* c, const float* send_dev, float* recv_dev, size_t count_per_rank, void* stream);

/* ---- measurement ------------------------------------------------------------------------- */
/* Per-kernel-class HIP-event timing on the launch stream.  enable = 1: every launch of the classes
 * below is bracketed by hipEvents until disabled; enable = 2: the same for the launches outside the
 * progressive-fusion blocks and for blocks 3, 13, ... (every 4th block of models with fewer than ten; blocks are identical, so average launch durations
 * are unbiased; ~30 instead of ~95 events per forward - each event costs the stream ~2 us, and more where it breaks up back-to-back
 * launches); enable = 3: the launches of ONE progressive-fusion block (block num_block / 2) and nothing else - 3 events per forward: the
 * dominant kernel classes timed live at next to no cost to the forward that is being timed; enable = 4 ("class runs", for the
 * launch-bound small shapes where an event per launch costs a fifth of the forward): ONE event wherever the class of consecutive
 * launches changes and at the end of the forward (~8 per forward), each interval credited with the launches it holds;
 * pfnl_profile_read synchronises and returns accumulated milliseconds and the number of TIMED launches
 * since the last reset. */
enum {
    PFNL_K_NL_PACK = 0, PFNL_K_NL_ATTN = 1, PFNL_K_CONV0 = 2, PFNL_K_CONV3X3 = 3,
    PFNL_K_CONV1X1 = 4, PFNL_K_MERGE1 = 5, PFNL_K_TAIL = 6, PFNL_K_COUNT = 7
};
int pfnl_profile_enable(pfnl_handle* h, int enable);
int pfnl_profile_reset(pfnl_handle* h);
int pfnl_profile_read(pfnl_handle* h, double* ms /*[PFNL_K_COUNT]*/, int64_t* launches /*[PFNL_K_COUNT]*/);
/* Tracing: with env PFNL_ROCTX=1 every kernel class of a forward is wrapped in a roctx range ("pfnl:conv3x3", ...; roctx is
 * resolved at run time, never linked): `rocprofv3 --marker-trace --kernel-trace` then shows the launches inside named ranges. */

/* ---- debugging / per-stage parity --------------------------------------------------------- */
/* Copy an internal buffer of the last forward to host (synchronises).  Names:
 *   "nl_out"  [B,H,W,3T]   frame stack after the non-local residual (model/pfnl.py:60)
 *   "trunk"   [B,T,H,W,64] inp0 after the last PF block          (model/pfnl.py:71)
 *   "merge1"  [B,H,W,48]   after convmerge1                       (model/pfnl.py:74)  */
int pfnl_debug_tap(pfnl_handle* h, const char* name, float* host_dst, size_t count);

/* ---- single ops (the TF kernels the reference calls), device pointers, async on stream ---- */
/* tf.layers.Conv2D(k=1|3, 'same') + bias + optional leaky_relu(0.2) on NHWC float32 with the MFMA
 * implicit-GEMM kernel.  in [items*frames_per_item, H, W, 64] viewed as [items,H,W,64*fpi];
 * kernel_host = HWIO [k,k,64*fpi,cout] (host), bias_host [cout] or NULL; cout <= 64;
 * addend (device, [items/add_div,H,W,64]) or NULL is added before the activation, resid (device,
 * [items,H,W,cout]) or NULL after it; out [items,H,W,cout].  (model/pfnl.py:49-52,66-74) */
int pfnl_op_conv2d(const float* in, const float* kernel_host, const float* bias_host,
                   const float* addend, int add_div, const float* resid, float* out,
                   int items, int frames_per_item, int H, int W, int ksize, int cout, int act,
                   void* stream);
/* The whole of conv2_i (reference model/pfnl.py:51, :69-71) in one launch of the persistent Winograd kernel:
 * out[c*T+t] = resid[c*T+t] + act(conv3x3(concat([base[c], in[c*T+t]]); kernel) + bias), the base half computed
 * once per clip and tile and kept in LDS.  in/resid/out [clips*T, H, W, 64], base [clips, H, W, 64],
 * kernel_host HWIO [3,3,128,64]; out may alias resid. */
int pfnl_op_conv2_grouped(const float* in, const float* base, const float* kernel_host, const float* bias_host,
                          const float* resid, float* out, int clips, int frames_per_clip, int H, int W, int act,
                          void* stream);
/* convmerge1 (reference model/pfnl.py:52, :73-74): 3x3 convolution over the concat of frames_per_clip frames,
 * (64*fpc) -> cout <= 64, as ONE launch of the persistent Winograd kernel in its accumulating mode.
 * in [clips*fpc, H, W, 64], kernel_host HWIO [3,3,64*fpc,cout], out [clips, H, W, 64] (channels >= cout: act(0)). */
int pfnl_op_conv3x3_accum(const float* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                          int frames_per_clip, int H, int W, int cout, int act, void* stream);
/* The same sum on the f16 matrix pipe with exactly split operands: the accumulating mode of conv3x3_split16_kernel (any H, W;
 * what the forward runs for convmerge1 when conv3x3 resolves to split16; option merge1 = auto | split16 | winograd). */
int pfnl_op_conv3x3_accum_split16(const float* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                                  int frames_per_clip, int H, int W, int cout, int act, void* stream);
/* conv10_i (reference model/pfnl.py:50, :67-68): the 1x1, (frames_per_item*64) -> 64 convolution through
 * the streaming kernel that reads its A operand straight from HBM (no LDS; conv1x1.hip).
 * in [items*frames_per_item, HW, 64], kernel_host HWIO [1,1,64*fpi,64], out [items, HW, 64]. */
int pfnl_op_conv1x1_stream(const float* in, const float* kernel_host, const float* bias_host, float* out,
                           int items, int frames_per_item, int HW, int act, void* stream);
/* ... and on the f16 matrix pipe with exactly split fp32 operands (option conv1x1=split16, the default): same contract. */
int pfnl_op_conv1x1_split16(const float* in, const float* kernel_host, const float* bias_host, float* out,
                            int items, int frames_per_item, int HW, int act, void* stream);
/* bf16 trunk (option precision=bf16; BASELINE.json configs[3]): the 3x3 64->64 convolution of a progressive-fusion
 * block (reference model/pfnl.py:49,51,66,69-71) on bf16 MFMA with fp32 accumulation.  Tensors are bf16 (uint16_t
 * bit patterns) [items, H, W, 64]; kernel_host fp32 HWIO [3,3,64,64] (rounded to bf16 inside), bias fp32.
 * out = act(conv + bias + addend[item / add_div]) + resid; addend and resid both NULL or both given; out may alias resid. */
int pfnl_op_conv3x3_bf16(const uint16_t* in, const float* kernel_host, const float* bias_host, const uint16_t* addend,
                         int add_div, const uint16_t* resid, uint16_t* out, int items, int H, int W, int act, void* stream);
/* The fp32 3x3 64->64 convolution on the f16 matrix pipe with split operands (option conv3x3=split16, conv_split16.hip): fp32
 * tensors in and out, fp32 accumulation, every operand taken as f16(x) + f16((x - f16(x)) 2^11) 2^-11 (>= 22 mantissa bits per
 * product).  Same contract as pfnl_op_conv3x3_winograd (any H, W); out may alias resid. */
int pfnl_op_conv3x3_split16(const float* in, const float* kernel_host, const float* bias_host, const float* addend, int add_div,
                            const float* resid, float* out, int items, int H, int W, int act, void* stream);
/* conv1_i + conv10_i of a progressive-fusion block as ONE launch of the fp32 path (reference model/pfnl.py:66-68;
 * conv3x3_c1c10_kernel, option split16_c10): in [clips*T,H,W,64] fp32 (device) -> out1 = lrelu(conv3x3(in; k1) + b1) per frame,
 * base = lrelu(conv1x1(concat_t out1; k10) + b10) [clips,H,W,64]; k1_host HWIO [3,3,64,64], k10_host HWIO [1,1,64T,64].  The kernel
 * writes both results in the split format; the hook returns them as fp32 (hi + lo' 2^-11). */
int pfnl_op_conv1_conv10_split16(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                 const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                 void* stream);
/* ... with its input taken in the split format by LDS-DMA (conv3x3_c1c10_kernel<true>: what blocks 1 .. nb-1 of the default "chain2_sf0"
 * plan run, reference model/pfnl.py:66-68).  The hook converts `in` with the producer's own split first; results are BIT-IDENTICAL to
 * pfnl_op_conv1_conv10_split16 (same binary16 operand pairs, same order). */
int pfnl_op_conv1_conv10_split16_sf0(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                     const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                     void* stream);
/* The whole of conv2_i in one launch (pfnl_op_conv3x3_split16_sf which = 2; reference model/pfnl.py:69-71) that ALSO writes its result in
 * the split format (conv3x3_sf_chain_kernel<true>): out [items,H,W,64] fp32 as before; out_sf [items,H,W,128] binary16 bit patterns
 * (device) = per pixel [channel half][hi 32 | lo' 32], hi = f16(out), lo' = f16((out - hi) 2^11). */
int pfnl_op_conv2_chain_sf0(const float* in, const float* kernel_host, const float* bias_host, const float* base, int add_div, const float* resid,
                            float* out, uint16_t* out_sf, int items, int H, int W, int act, void* stream);
/* C-ABI v4: the chained launches of the trunk with the MFMA shape and the split-chain geometry chosen by the caller instead of the
 * forward's plan, so that every form the plan can pick is compared with the spec op by op.  Arguments and results as the hooks named below.
 *   mfma = 16: the v_mfma_*_16x16x32 form on its own weight pack; mfma = 32: the 32x32x16 form.
 *   split chains (split_s > 0): the first n_full (clip, 8x32 tile) chains - a multiple of the launch grid (the CU count rounded down to whole
 *   XCDs, at least 8) below the chain count - run whole; each chain behind them is cut by frames into split_s <= 7 parts of <= split_q
 *   frames, every part non-empty, the parts together the chain's frames, at most one part per workgroup of the grid.  split_s = 0: no cut
 *   (n_full and split_q ignored).  A geometry outside that rule returns PFNL_ERR_INVALID before any allocation or launch; `out` is untouched.
 * pfnl_op_conv2_chain_ex: the whole of conv2_i as pfnl_op_conv3x3_split16_sf(which = 2) (conv3x3_sf_chain_kernel / conv3x3_sf_chain16_kernel);
 *   mfma = 16 with split_s > 0 is refused (split chains exist on the 32x32x16 kernel only). */
int pfnl_op_conv2_chain_ex(const float* in, const float* kernel_host, const float* bias_host, const float* base, int add_div, const float* resid,
                           float* out, int items, int H, int W, int act, int mfma, int n_full, int split_s, int split_q, void* stream);
/* pfnl_op_conv1_conv10_split16 with split chains: the cut chains' parts leave raw conv10_i sums that c10_finalize_kernel adds into base. */
int pfnl_op_conv1_conv10_split16_ex(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                    const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                    int n_full, int split_s, int split_q, void* stream);
/* ... with the MFMA shape of conv1_i's 3x3 stage given: mfma = 16 runs conv3x3_c1c10_kernel's 16x16x32 form (what trunk_plan picks where pfnl_plan
 * says c1_mfma=16; whole rounds only: split_s must be 0), 32 is pfnl_op_conv1_conv10_split16_ex.  conv10_i's stage is on 32x32x16 in both. */
int pfnl_op_conv1_conv10_split16_mfma(const float* in, const float* k1_host, const float* b1_host, const float* k10_host,
                                      const float* b10_host, float* out1, float* base, int clips, int frames_per_clip, int H, int W,
                                      int mfma, int n_full, int split_s, int split_q, void* stream);
/* pfnl_op_conv3x3_accum_split16 (convmerge1) with split chains: the parts' raw sums meet in c10_finalize_kernel (+ bias, act) into out. */
int pfnl_op_conv3x3_accum_split16_ex(const float* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                                     int frames_per_clip, int H, int W, int cout, int act, int n_full, int split_s, int split_q, void* stream);
/* pfnl_op_conv3x3_bf16 in its fused mode (addend and resid required) and pfnl_op_conv1_conv10_bf16, both on the third-generation bf16
 * kernel called directly (conv_bf16_v3.hip; PFNL_BF16_V3 does not apply); mfma = 16 runs its M16 form.  Split chains of the conv1_conv10
 * form: the parts' raw conv10_i sums meet in c10_finalize_bf16_kernel (+ b10, leaky-relu, bf16) into base. */
int pfnl_op_conv3x3_bf16_ex(const uint16_t* in, const float* kernel_host, const float* bias_host, const uint16_t* addend, int add_div,
                            const uint16_t* resid, uint16_t* out, int items, int H, int W, int act, int mfma, int n_full, int split_s,
                            int split_q, void* stream);
int pfnl_op_conv1_conv10_bf16_ex(const uint16_t* in, const float* k1_host, const float* b1_host, const float* k10_host, const float* b10_host,
                                 uint16_t* out1, uint16_t* base, int clips, int frames_per_clip, int H, int W, int mfma, int n_full, int split_s,
                                 int split_q, void* stream);
/* The split-format variants of the split-f16 kernels (pfnl_amd/csrc/conv_split16.h "SF": an activation tensor that only feeds MFMA
 * operands - conv1_i's and conv10_i's outputs, model/pfnl.py:66-68 - is kept as (hi, lo') binary16 pairs, built once by its
 * producer).  fp32 at the hook's interface: conversions bracket the kernel under test.
 * which = 0: the 3x3 kernel of conv2_i (input SF by LDS-DMA, epilogue from registers; plain, or fused with addend + resid);
 * which = 1: the 3x3 kernel of conv1_i writing SF;
 * which = 2: the WHOLE of conv2_i in one launch (conv3x3_sf_chain_kernel): kernel_host = HWIO [3,3,128,64], `addend` = base
 *   [items/add_div][H][W][64] fp32, out = lrelu(conv(concat([base, in])) + bias) + resid. */
int pfnl_op_conv3x3_split16_sf(int which, const float* in, const float* kernel_host, const float* bias_host, const float* addend,
                               int add_div, const float* resid, float* out, int items, int H, int W, int act, void* stream);
int pfnl_op_conv1x1_split16_sf(const float* in, const float* kernel_host, const float* bias_host, float* out, int items,
                               int frames_per_item, int HW, int act, int in_sf, int out_sf, void* stream);
/* The small-shape trunk kernel (pfnl_amd/csrc/conv_small.hip; BASELINE.json configs[0] / configs[4]): conv1_i, conv10_i, the whole of
 * conv2_i (3x3 over concat([base, f]), model/pfnl.py:69-71) and convmerge1 as one template.  Source s of output item i is
 * s < nA ? a[i / a_div] : b[i * b_mul + (s - nA)] ([.][H][W][64] fp32 each); kernel HWIO [ks, ks, 64 nsrc, cout <= 64];
 * out [items][H][W][64] (channels >= cout are written as act(0)); resid may alias out. */
int pfnl_op_conv_small(const float* a, const float* b, int nA, int a_div, int b_mul, int nsrc, const float* kernel_host,
                       const float* bias_host, const float* resid, float* out, int items, int H, int W, int ks, int cout, int act,
                       void* stream);
/* One progressive-fusion block (reference model/pfnl.py:66-71) on the small-shape kernels as the forward launches it (option
 * small_c10 = on: two launches): inp1 = lrelu(conv3x3(x; k1) + b1) [clips*T, H, W, 64] - the same launch writes each frame's
 * 64 x 64 slice of conv10_i as a partial sum - and out = x + lrelu(conv3x3(concat([base, inp1_t]); k2) + b2), base = lrelu(sum of
 * the T partials + b10) formed in the second launch's prologue.  k1 HWIO [3,3,64,64], k10 [1,1,64T,64], k2 [3,3,128,64]. */
int pfnl_op_conv_small_pf_block(const float* x, const float* k1_host, const float* b1_host, const float* k10_host, const float* b10_host,
                                const float* k2_host, const float* b2_host, float* inp1, float* out, int clips, int T, int H, int W,
                                void* stream);
/* conv1_i and conv10_i of a progressive-fusion block (reference model/pfnl.py:66-68) in ONE launch of the bf16 3x3 kernel:
 * out1 = lrelu(conv3x3(in) + b1) [clips*fpc, H, W, 64], base = lrelu(conv1x1(concat_t out1_t) + b10) [clips, H, W, 64];
 * the 1x1 contraction reads every finished tile from LDS.  fpc in {3,5,7}. */
int pfnl_op_conv1_conv10_bf16(const uint16_t* in, const float* k1_host, const float* b1_host, const float* k10_host,
                              const float* b10_host, uint16_t* out1, uint16_t* base, int clips, int frames_per_clip, int H, int W,
                              void* stream);
/* convmerge1 (reference model/pfnl.py:52, :73-74) from the bf16 trunk: 3x3 over the concat of frames_per_clip frames,
 * (64*fpc) -> cout <= 64, as ONE launch of the bf16 3x3 kernel in its accumulating mode (the weight pack in LDS is replaced
 * between the frames of a chain).  in bf16 [clips*fpc, H, W, 64]; kernel_host fp32 HWIO [3,3,64*fpc,cout]; out fp32
 * [clips, H, W, 64] (channels >= cout: act(0)). */
int pfnl_op_conv3x3_accum_bf16(const uint16_t* in, const float* kernel_host, const float* bias_host, float* out, int clips,
                               int frames_per_clip, int H, int W, int cout, int act, void* stream);
/* ... and conv10_i (reference model/pfnl.py:50, :67-68): in [items*fpi, HW, 64] bf16, kernel_host fp32 HWIO
 * [1,1,64*fpi,64], out [items, HW, 64] bf16; fpi in {3,5,7}. */
int pfnl_op_conv1x1_bf16(const uint16_t* in, const float* kernel_host, const float* bias_host, uint16_t* out, int items,
                         int frames_per_item, int HW, int act, void* stream);
/* The same 3x3 64->64 convolution (frames_per_item = 1, cout = 64) through the fused Winograd
 * F(2x2,3x3) kernel; H and W must be even. */
int pfnl_op_conv3x3_winograd(const float* in, const float* kernel_host, const float* bias_host,
                             const float* addend, int add_div, const float* resid, float* out,
                             int items, int H, int W, int act, void* stream);
/* Same contract, the persistent wave-specialised kernel (conv_wino_ws.hip). */
int pfnl_op_conv3x3_winograd_ws(const float* in, const float* kernel_host, const float* bias_host,
                                const float* addend, int add_div, const float* resid, float* out, int items, int H,
                                int W, int act, void* stream);
/* utils.NonLocalBlock(nltype=1) + the residual of model/pfnl.py:55-60:
 * x [B,T,H,W,3] -> out [B,H,W,3T] = stack(x) + depth_to_space(NL(space_to_depth(stack(x)))). */
int pfnl_op_nonlocal(const float* x, const float* wg_host, const float* bg_host,
                     const float* ww_host, const float* bw_host, float* out,
                     int B, int T, int H, int W, void* stream);
/* The same block (fp32 in and out) on the f16 matrix pipe with exactly split operands (option nonlocal=split16, nonlocal_f16.hip):
 * Q, K, V and the probabilities are taken as f16(x) + f16(x - f16(x)), scaled by powers of two into binary16's normal range. */
int pfnl_op_nonlocal_split16(const float* x, const float* wg_host, const float* bg_host,
                     const float* ww_host, const float* bw_host, float* out,
                     int B, int T, int H, int W, void* stream);
/* The same kernel on the hi parts only - 16-bit (binary16) operands, fp32 accumulation and softmax state: the non-local block of
 * precision=bf16 (24 instead of 72 MFMAs per 64 keys). */
int pfnl_op_nonlocal_f16(const float* x, const float* wg_host, const float* bg_host,
                     const float* ww_host, const float* bw_host, float* out,
                     int B, int T, int H, int W, void* stream);
/* The embedded-Gaussian form of the block (reference utils.py:18-71 with nltype 0): same contract as pfnl_op_nonlocal plus
 * theta / phi 1x1 projections wt, wp [C,C] (row = input channel), bt, bp [C]. */
int pfnl_op_nonlocal_embedded(const float* x, const float* wg_host, const float* bg_host, const float* ww_host,
                              const float* bw_host, const float* wt_host, const float* bt_host, const float* wp_host,
                              const float* bp_host, float* out, int B, int T, int H, int W, void* stream);
/* utils.NonLocalBlock(input_x, out_channels, sub_sample, nltype) in its general form (reference utils.py:18-71) with the same
 * stack / space_to_depth / residual wrapper as pfnl_op_nonlocal: nltype 0 embedded Gaussian (theta, phi projections, exp / rowsum),
 * 1 Gaussian (theta = phi = x; wt .. bp may be NULL), 2 dot product (relu / rowsum, utils.py:59-62 - a query whose affinities are
 * all <= 0 divides by zero there and yields NaN here as well); sub_sample > 1: g and phi average-pooled (pool = stride = sub_sample,
 * 'valid') on the space_to_depth grid (utils.py:27-28,35-36).  nltype 3 ('concat') builds no graph in the reference and is rejected. */
int pfnl_op_nonlocal_block(const float* x, const float* wg_host, const float* bg_host, const float* ww_host,
                           const float* bw_host, const float* wt_host, const float* bt_host, const float* wp_host,
                           const float* bp_host, int nltype, int sub_sample, float* out, int B, int T, int H, int W, void* stream);
/* conv0 (reference model/pfnl.py:48,61-62): lrelu(conv5x5 'same' 3 -> 64 + b) of every frame.
 * x [B,T,H,W,3] (device), kernel_host HWIO [5,5,3,64], bias_host [64] or NULL, out [B*T,H,W,64] (device). */
int pfnl_op_conv0(const float* x, const float* kernel_host, const float* bias_host, float* out, int B, int T, int H, int W,
                  void* stream);
/* The same with the kernel chosen by the caller: f32 = 0 the default (the split-f16 MFMA kernel, or the VALU kernel under PFNL_CONV0=valu),
 * f32 != 0 the fp32 VALU kernel that strict_fp32=on and the range re-run use (an addition to ABI v4: nothing existing changed). */
int pfnl_op_conv0_ex(const float* x, const float* kernel_host, const float* bias_host, float* out, int B, int T, int H, int W,
                     int f32, void* stream);
/* conv0 as precision=bf16 runs it: the default kernel of pfnl_op_conv0 (same arithmetic, same PFNL_CONV0 choice), its result rounded
 * once to bf16 at the store.  out [B*T,H,W,64] bf16 (device).  (An addition to ABI v4: nothing existing changed.) */
int pfnl_op_conv0_bf16(const float* x, const float* kernel_host, const float* bias_host, uint16_t* out, int B, int T, int H, int W,
                       void* stream);
/* The tail(reference model/pfnl.py:53,63,76-80): depth_to_space(2) -> convmerge2 3x3 (no activation) -> depth_to_space(2)
 * (scale 4 only) -> + ResizeBicubic(x[:, T/2]) -> [B,1,sH,sW,3].  merge [B,H,W,48] (device, the output of convmerge1),
 * x [B,T,H,W,3] (device), kernel_host HWIO [3,3,12,12] (scale 4) or [3,3,12,3] (scale 2), bias_host or NULL. */
int pfnl_op_tail(const float* merge, const float* x, const float* kernel_host, const float* bias_host, float* out, int B,
                 int T, int H, int W, int scale, void* stream);
/* Harness helpers (reference model/pfnl.py:238-242, 254-257), device pointers, async on stream:
 * windows: frames [F,H,W,3] -> win [count,T,H,W,3], window w slot t = frame clip(first + w + t - T/2, 0, F-1);
 * quantise: uint8(np.round(np.clip(sr * 255, 0, 255))) (round half to even), n % 4 == 0. */
int pfnl_op_gather_windows(const float* frames, float* win, int F, int first, int count, int T, int H, int W, void* stream);
int pfnl_op_quantise_u8(const float* sr, uint8_t* out, size_t n, void* stream);
/* The session's input side (stream_gather_u8_kernel): ring [cap,H,W,3] uint8 with frame f in slot f % cap -> win [count,T,H,W,3] float32,
 * window w slot t = frame clip(first + w + t - T/2, 0, last), every value the harness's (u8 / 255.).astype(np.float32) bit for bit
 * (reference model/pfnl.py:287; a 256-entry table).  The frames the windows name must fit the ring; first + count - 1 <= last; ring
 * 4-byte aligned (16-byte for the 16-byte reads), win 16-byte aligned - else PFNL_ERR_INVALID. */
int pfnl_op_gather_windows_u8(const uint8_t* ring, float* win, int cap, long long last, long long first, int count, int T, int H, int W,
                              void* stream);
/* The session's scene kernels (pfnl_stream_scenes).  sad: a, b [H,W,3] uint8 (device) -> *out_dev (device) = sum |Y(a) - Y(b)|, exact; any
 * H, W >= 1 and any alignment (16-byte reads where H*W*3 is a multiple of 16 and both pointers are aligned, else 4-byte or single-byte
 * ones).  Synchronises `stream` (it owns a scratch word).  gather: pfnl_op_gather_windows_u8 with scene_first_dev [cap] int64 (device),
 * slot f % cap = the first frame of frame f's scene; one scene gives pfnl_op_gather_windows_u8's windows. */
int pfnl_op_scene_sad_u8(const uint8_t* a, const uint8_t* b, int H, int W, unsigned long long* out_dev, void* stream);
int pfnl_op_gather_windows_u8_scenes(const uint8_t* ring, const long long* scene_first_dev, float* win, int cap, long long last, long long first,
                                     int count, int T, int H, int W, void* stream);
/* The session's format kernels (pfnl_stream_format; the rule: pfnl_amd/yuv.py).  yuv [n][H*W*3/2] uint8 in fmt PFNL_PIX_NV12 or
 * PFNL_PIX_I420 <-> rgb [n][H][W][3] uint8, device pointers, asynchronous on stream.  H and W even; any alignment (16-byte words where
 * W is a multiple of 16 and both pointers are aligned, 4-byte words for multiples of 4, else single bytes).  NULL, odd or non-positive
 * H / W, n < 1, an unknown fmt / matrix / full_range and fmt = PFNL_PIX_RGB24: PFNL_ERR_INVALID before any HIP call. */
int pfnl_op_yuv420_to_rgb_u8(const uint8_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* rgb, void* stream);
int pfnl_op_rgb_to_yuv420_u8(const uint8_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* yuv, void* stream);
/* The same decode of one frame given as a surface (SURFACES: device planes by pointer and pitch, NV12 or I420) -> rgb [H][W][3], tightly
 * packed: the kernel a device-pointer pfnl_stream_push_surface runs, and byte for byte pfnl_op_yuv420_to_rgb_u8 of the packed frame.  A
 * NULL or short surface is refused as there, before any HIP call. */
int pfnl_op_yuv420_to_rgb_u8_surface(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W,
                                     uint8_t* rgb /*[H][W][3] packed*/, void* stream);
/* The session's resampler (pfnl_stream_resize; the rule: pfnl_amd/resize.py).  in [n][H][W][3] uint8 -> out [n][oH][oW][3] uint8, device
 * pointers, asynchronous on stream up to the hook's own synchronisation (it uploads the tap tables and frees them on return).  One launch
 * does both passes through an int16 LDS tile; any alignment (16-byte stores where oW is a multiple of 16 and out is aligned, single bytes
 * otherwise).  NULL, n < 1 and sizes outside pfnl_resize_taps' limits: PFNL_ERR_INVALID before any HIP call. */
int pfnl_op_resize_u8(const uint8_t* in, int n, int H, int W, int oH, int oW, uint8_t* out, void* stream);
/* The session's 10-bit output kernels (pfnl_stream_format with a 10-bit out_fmt; the rule: pfnl_amd/depth10.py), uint16 samples, device
 * pointers, asynchronous on stream.  quantise: sr [n] float32 (16-byte aligned) -> uint16(round(clip(sr * 1023, 0, 1023))) (8-byte
 * aligned), n a positive multiple of 4; NaN gives 0.  rgb_to_yuv420: rgb [n][H][W][3] with values 0 .. 1023 -> [n][H*W*3/2] in fmt
 * PFNL_PIX_P010 or PFNL_PIX_I010; H and W even; any alignment (16-byte words where W is a multiple of 8 and both pointers are aligned, else
 * single samples).  resize: pfnl_op_resize_u8 on values 0 .. 1023 (16-byte stores where oW is a multiple of 8 and out is aligned); it
 * synchronises as that hook does.  NULL, odd or non-positive sizes, n < 1, an unknown fmt / matrix / full_range (fmt: the 8-bit formats
 * and PFNL_PIX_RGB10 among them) and sizes outside pfnl_resize_taps' limits: PFNL_ERR_INVALID before any HIP call. */
int pfnl_op_quantise_u10(const float* sr, uint16_t* out, size_t n, void* stream);
/* Stage 0 with a change of primaries (COLOUR above; pfnl_amd/csrc/colour.hip): sr [pixels][3] fp32 -> out [pixels][3] samples, sample for
 * sample pfnl_amd/colour.py convert(quantise(sr), src, dst); src == dst is pfnl_op_quantise_u8 / _u10 itself.  pixels a positive multiple
 * of 4, sr 16-byte and out 8-byte aligned, src and dst PFNL_PRIM_*: PFNL_ERR_INVALID before any HIP call otherwise.  Asynchronous on
 * `stream`, as pfnl_op_quantise_u10 is; the first call on a device uploads its tables (a blocking copy). */
int pfnl_op_quantise_colour_u8(const float* sr, uint8_t* out, size_t pixels, int src, int dst, void* stream);
int pfnl_op_quantise_colour_u10(const float* sr, uint16_t* out, size_t pixels, int src, int dst, void* stream);
int pfnl_op_rgb_to_yuv420_u10(const uint16_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* yuv, void* stream);
int pfnl_op_resize_u10(const uint16_t* in, int n, int H, int W, int oH, int oW, uint16_t* out, void* stream);
/* The four conversion hooks above with the chroma siting named (SITING: PFNL_SITING_*), ahead of stream; the plain hooks are these with
 * PFNL_SITING_LEFT.  A siting outside the enum is PFNL_ERR_INVALID before any HIP call, like every other argument. */
int pfnl_op_yuv420_to_rgb_u8_sited(const uint8_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* rgb, int siting,
                                   void* stream);
int pfnl_op_yuv420_to_rgb_u8_surface_sited(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W,
                                           uint8_t* rgb /*[H][W][3] packed*/, int siting, void* stream);
int pfnl_op_rgb_to_yuv420_u8_sited(const uint8_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* yuv, int siting,
                                   void* stream);
int pfnl_op_rgb_to_yuv420_u10_sited(const uint16_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* yuv, int siting,
                                    void* stream);
/* The session's placement kernels (PLACEMENT, pfnl_stream_place; the rule: pfnl_amd/fit.py place, pfnl_amd/depth10.py place10).  in
 * [n][H][W][3] -> out [n][oH][oW][3]: fill everywhere, the resize of in[src] at dst; src NULL = the whole frame, dst NULL = the whole canvas,
 * fill NULL = zeros; at 10 bits fill is in sample values, <= 1023.  Device pointers; they synchronise as pfnl_op_resize_u8 does.  One launch,
 * every output sample stored once; any alignment (16-byte stores where oW is a multiple of 16 - of 8 at 10 bits - and out is aligned, single
 * samples otherwise).  NULL in / out, n < 1, a rectangle outside its raster, a src -> dst ratio outside pfnl_resize_taps' limits and a fill
 * above 1023: PFNL_ERR_INVALID before any HIP call, the message naming src, dst or fill. */
int pfnl_op_resize_place_u8(const uint8_t* in, int n, int H, int W, int oH, int oW, const pfnl_rect* src, const pfnl_rect* dst,
                            const uint8_t fill[3], uint8_t* out, void* stream);
int pfnl_op_resize_place_u10(const uint16_t* in, int n, int H, int W, int oH, int oW, const pfnl_rect* src, const pfnl_rect* dst,
                             const uint16_t fill[3], uint16_t* out, void* stream);
/* 10 BITS IN, the op hooks (10 BITS IN above; the rules: pfnl_amd/depth10.py to_rgb10 / values10 / dequantise10, pfnl_amd/scene.py luma_u10).
 * Device pointers to uint16 samples, 2-byte aligned (the rings 4-byte); NULL, a bad fmt / matrix / range / siting and odd sizes are
 * PFNL_ERR_INVALID before any HIP call.  They are the 8-bit hooks' kernel bodies on uint16 samples and synchronise as those do.
 *   pfnl_op_yuv420_to_rgb_u10_sited: yuv [n][H*W*3/2] in P010 (low six bits ignored) or I010 (above 1023 = 1023) -> rgb [n][H][W][3], values
 *     0 .. 1023.  16-byte words (8 pixels a lane) where W % 8 == 0 and both pointers are 16-byte aligned; single samples otherwise.
 *   pfnl_op_yuv420_to_rgb_u10_surface_sited: one frame as planes with a pitch (SURFACES), read in place.
 *   pfnl_op_gather_windows_u10 / _scenes: pfnl_op_gather_windows_u8 / _scenes on a ring [cap][H][W][3] uint16: win = min(sample, 1023) / 1023.
 *     through a 1024-entry table; H*W*3 even.
 *   pfnl_op_scene_sad_u10: pfnl_op_scene_sad_u8 on two [H][W][3] uint16 frames with luma_u10. */
int pfnl_op_yuv420_to_rgb_u10_sited(const uint16_t* yuv, int fmt /*P010|I010*/, int matrix, int full_range, int n, int H, int W, uint16_t* rgb,
                                    int siting, void* stream);
int pfnl_op_yuv420_to_rgb_u10_surface_sited(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint16_t* rgb, int siting,
                                            void* stream);
int pfnl_op_gather_windows_u10(const uint16_t* ring, float* win, int cap, long long last, long long first, int count, int T, int H, int W,
                               void* stream);
int pfnl_op_gather_windows_u10_scenes(const uint16_t* ring, const long long* scene_first_dev, float* win, int cap, long long last, long long first,
                                      int count, int T, int H, int W, void* stream);
int pfnl_op_scene_sad_u10(const uint16_t* a, const uint16_t* b, int H, int W, unsigned long long* out_dev, void* stream);
/* The kernel of BARS on its own.  frames [n][H][W][3] uint8 | uint16 at 10 bits (device; any alignment a sample can have) -> box_dev
 * [n][4] int32 (y0, x0, h, w) and, where given, rows_dev [n][H] and cols_dev [n][W] uint32 (device, 4-byte aligned), exact against
 * pfnl_amd/bars.py.  One launch for the n frames; it synchronises `stream` (it owns the scratch words).  NULL frames or box_dev, n < 1,
 * H or W outside 1 .. 16384, a limit outside 0 .. 219 and a misaligned pointer: PFNL_ERR_INVALID before any HIP call. */
int pfnl_op_content_box_u8(const uint8_t* frames, int n, int H, int W, int limit, int32_t* box_dev /*[n][4]*/,
                           uint32_t* rows_dev /*[n][H] or NULL*/, uint32_t* cols_dev /*[n][W] or NULL*/, void* stream);
int pfnl_op_content_box_u10(const uint16_t* frames, int n, int H, int W, int limit, int32_t* box_dev /*[n][4]*/,
                            uint32_t* rows_dev /*[n][H] or NULL*/, uint32_t* cols_dev /*[n][W] or NULL*/, void* stream);
/* The six _sited conversion hooks with the subsampling named (CHROMA FORMAT: PFNL_CHROMA_*), ahead of siting; with PFNL_CHROMA_420 each is
 * its _sited twin, refusals included.  fmt names the layout: PFNL_PIX_NV12 / PFNL_PIX_I420 for the u8 hooks, PFNL_PIX_P010 / PFNL_PIX_I010
 * for the u10 ones.  yuv holds n frames of 2 H W (4:2:2) or 3 H W (4:4:4) samples, a surface chroma planes of H rows.  Odd W at 4:2:2, an RGB
 * fmt, chroma / siting / matrix / full_range outside their enums, n < 1, H or W < 1, NULL, a short pitch and an odd pointer or pitch for
 * 16-bit samples: PFNL_ERR_INVALID before any HIP call, and pfnl_last_error names the argument. */
int pfnl_op_yuv_to_rgb_u8_chroma(const uint8_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* rgb, int chroma, int siting,
                                 void* stream);
int pfnl_op_yuv_to_rgb_u10_chroma(const uint16_t* yuv, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* rgb, int chroma,
                                  int siting, void* stream);
int pfnl_op_yuv_to_rgb_u8_surface_chroma(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint8_t* rgb, int chroma,
                                         int siting, void* stream);
int pfnl_op_yuv_to_rgb_u10_surface_chroma(const pfnl_surface* yuv, int fmt, int matrix, int full_range, int H, int W, uint16_t* rgb, int chroma,
                                          int siting, void* stream);
int pfnl_op_rgb_to_yuv_u8_chroma(const uint8_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint8_t* yuv, int chroma, int siting,
                                 void* stream);
int pfnl_op_rgb_to_yuv_u10_chroma(const uint16_t* rgb, int fmt, int matrix, int full_range, int n, int H, int W, uint16_t* yuv, int chroma,
                                  int siting, void* stream);
/* The two kernels of PACKED FORMATS on their own: n frames in ONE packed plane - frame f starts at plane + f * frame_stride, its rows lie
 * `pitch` bytes apart - <-> rgb [n][H][W][3], uint8 for the 8-bit packings (the _u8 hooks), uint16 values 0 .. 1023 for the 10-bit ones
 * (_u10).  Device pointers, asynchronous on `stream`.  An RGB packing ignores matrix, full_range and siting's value (all must still lie
 * in their enums).  NULL, a packing outside the enum or of the other depth, a width its unit does not divide, n / H / W < 1, a pitch below
 * the bytes of a row, a frame stride (n > 1) below H rows, a pointer, pitch or frame stride that is no multiple of 2 (y210) or 4
 * (x2rgb10, x2bgr10, v210), an odd rgb pointer at 10 bits: PFNL_ERR_INVALID before any HIP call.  Bytes between a row's end and the
 * pitch are never written. */
int pfnl_op_packed_to_rgb_u8(const void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H,
                             int W, uint8_t* rgb, void* stream);
int pfnl_op_packed_to_rgb_u10(const void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H,
                              int W, uint16_t* rgb, void* stream);
int pfnl_op_rgb_to_packed_u8(void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H, int W,
                             const uint8_t* rgb, void* stream);
int pfnl_op_rgb_to_packed_u10(void* plane, size_t pitch, int pack, int matrix, int full_range, int siting, int n, size_t frame_stride, int H, int W,
                              const uint16_t* rgb, void* stream);
/* The kernel of INTERLACED on its own: five decoded fields, tight [H/2][W][3] samples each (read-only; they may be one another, as at a
 * sequence's ends), `cur` of parity `parity` -> the progressive frame out [H][W][3] at cur's time; uint8, or uint16 whose samples are
 * taken as min(v, 1023) (_u10).  Device pointers, asynchronous on `stream`, any alignment a sample can have.  A NULL pointer, H < 2 or
 * odd, W < 1, a parity other than 0 or 1: PFNL_ERR_INVALID before any HIP call, with a message that names the argument. */
int pfnl_op_deinterlace_u8(const uint8_t* p2, const uint8_t* p1, const uint8_t* cur, const uint8_t* n1, const uint8_t* n2, int H, int W, int parity,
                           uint8_t* out, void* stream);
int pfnl_op_deinterlace_u10(const uint16_t* p2, const uint16_t* p1, const uint16_t* cur, const uint16_t* n1, const uint16_t* n2, int H, int W,
                            int parity, uint16_t* out, void* stream);
/* ... and the launch a field-rate session issues per push: fields[0 .. 5] are six consecutive fields k - 2 .. k + 3 (field k = fields[2]
 * of parity `parity`, field k + 1 of the other), out [2][H][W][3] the progressive frames at the times of fields k and k + 1, both made by
 * ONE launch.  The same refusals (the message names fields[i]). */
int pfnl_op_deinterlace_pair_u8(const uint8_t* const fields[6], int H, int W, int parity, uint8_t* out, void* stream);
int pfnl_op_deinterlace_pair_u10(const uint16_t* const fields[6], int H, int W, int parity, uint16_t* out, void* stream);
/* The kernels of TELECINE on their own.  A, Xc, Xp: the kept field of parity `parity` and its two candidate partners, tight [h][W][3]
 * samples each (read-only; they may be one another); uint8, or uint16 whose samples are taken as min(v, 1023) (_u10).  Device pointers,
 * any alignment a sample can have.  pfnl_op_fieldmatch_*: counts_dev[2] (8-byte aligned) = the comb counts of c and p; the hook owns its
 * scratch words and is complete on return.  pfnl_op_telecine_frame_*: the two launches a session issues per matched frame, asynchronous
 * on `stream` - counts, decision and weave: decision_dev[6] (8-byte aligned) = count of c, count of p, match (0: c, 1: p), post (0 | 1)
 * and two scratch words the caller zeroes before the first call and every call leaves zero (calls that share them must not overlap), and
 * out [2 h][W][3] the matched frame, which overlaps none of A, Xc, Xp (PFNL_ERR_INVALID).  With post != 0 the caller has put INTERLACED's
 * frame into `out`, and a flagged frame leaves it as it is - every byte of `out` unwritten.  params == NULL IS THE DEFAULTS, post = 1
 * among them: a caller who has no deinterlaced frame to offer passes params with post = 0, and the weave then always writes the frame.  comb_limit < 0: the default.  A NULL pointer, h < 1, W < 1, h 3 W >= 2^32, a parity other than 0 or 1,
 * a threshold outside 1 .. 255: PFNL_ERR_INVALID before any HIP call, with a message that names the argument. */
int pfnl_op_fieldmatch_u8(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, int threshold,
                          unsigned long long* counts_dev, void* stream);
int pfnl_op_fieldmatch_u10(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity, int threshold,
                           unsigned long long* counts_dev, void* stream);
int pfnl_op_telecine_frame_u8(const uint8_t* A, const uint8_t* Xc, const uint8_t* Xp, int h, int W, int parity, const pfnl_telecine_params* params,
                              uint8_t* out, unsigned long long* decision_dev, void* stream);
int pfnl_op_telecine_frame_u10(const uint16_t* A, const uint16_t* Xc, const uint16_t* Xp, int h, int W, int parity,
                               const pfnl_telecine_params* params, uint16_t* out, unsigned long long* decision_dev, void* stream);
/* Quality scores of the harness' uint8 frames on the device (what the reference leaves to matlab/compute_psnr.m, matlab/SSIM.m and
 * utils.py:213-246 AVG_PSNR after the PNGs are written): pred, truth [F,H,W,3] uint8 (device), per frame in one pass over the bytes
 *   Y = 16 + 0.256788235294118 R + 0.504129411764706 G + 0.097905882352941 B            (utils.py:194-211 _rgb2ycbcr, fp64),
 *   out[f][0] = sum of (Y_truth - Y_pred)^2 over the frame                              (matlab/compute_psnr.m:1-18, boundarypixels = 0),
 *   out[f][1] = the same over [sp_border : H - sp_border, sp_border : W - sp_border]    (utils.py:213-246, AVG_PSNR: 8),
 *   out[f][2] = sum of the SSIM map of modules/SSIM_Index.py:23-89 (11x11 Gaussian sigma 1.5, K = (0.01, 0.03), L = 255, 'reflect'),
 *   out[f][3] = its sum over [5 : H - 5, 5 : W - 5], what matlab/SSIM.m's filter2(..., 'valid') averages.
 * fp64 throughout; out [F,4] double (device); two calls on the same frames return identical bits.  11 <= H, W <= 65536, 1 <= F <= 65535,
 * 0 <= 2 * sp_border < H, W.  Asynchronous on stream, allocates nothing: scratch is pfnl_op_score_scratch_bytes(F, H, W) bytes of
 * device memory (8-byte aligned).  pfnl_amd/metrics.py sequence_scores turns the sums into PSNR_Y / SSIM / AVG_PSNR. */
int pfnl_op_score_scratch_bytes(int F, int H, int W, size_t* bytes);
int pfnl_op_score_y(const uint8_t* pred, const uint8_t* truth, int F, int H, int W, int sp_border, double* out, void* scratch,
                    void* stream);
/* tf.image.resize_images(method=2) of TF1.12 (model/pfnl.py:63): x [B,H,W,3] -> [B,sH,sW,3]. */
int pfnl_op_bicubic(const float* x, float* out, int B, int H, int W, int scale, void* stream);
/* The step before the path in test_video_truth / eval (reference utils.py:95-105,169-192:
 * DownSample_4D with BLUR): reflect-pad 6, 13x13 Gaussian sigma 1.6, stride `scale`, VALID.
 * hr [F,H,W,3] -> lr [F,ceil(H/scale),ceil(W/scale),3], device pointers, async on stream. */
int pfnl_op_blur_decimate(const float* hr, float* lr, int F, int H, int W, int scale, void* stream);
/* The two launches of the self-ensemble (SELF-ENSEMBLE above; pfnl_amd/csrc/dihedral.hip; the rule: pfnl_amd/ensemble.py), device
 * pointers, asynchronous on `stream`; NULL, k outside 0 .. 7, n_img < 1 and non-positive H or W are PFNL_ERR_INVALID before any HIP call.
 *   pfnl_op_dihedral: out = g_k(in) * scale.  in [n_img,H,W,3] -> out [n_img,H,W,3], or [n_img,W,H,3] for k >= 4; scale = 1 copies bits.
 *   pfnl_op_dihedral_accum: acc = fl32(acc + g_k^-1(y)) * scale.  acc [n_img,H,W,3]; y [n_img,H,W,3], or [n_img,W,H,3] for k >= 4
 *     (H, W are acc's); scale = 1 is the plain sum.  Every element of acc is read and written once, by one thread; no atomics.
 * in / y must not overlap out / acc.  16-byte accesses where W % 4 == 0 (the row length of both sides for k < 4) and both pointers are
 * 16-byte aligned; any alignment of whole floats otherwise. */
int pfnl_op_dihedral(const float* in, float* out, int n_img, int H, int W, int k, float scale, void* stream);
int pfnl_op_dihedral_accum(float* acc, const float* y, int n_img, int H, int W, int k, float scale, void* stream);
/* The two launches of a tiled forward's run (TILES above; pfnl_amd/csrc/tiles.hip; the rule: pfnl_amd/tiles.py), device pointers,
 * asynchronous on `stream`; NULL, a shape or tiling pfnl_forward_tiled would refuse, and tiles first .. first+count-1 that are not
 * tiles of the call are PFNL_ERR_INVALID before any HIP call.
 *   pfnl_op_tile_gather: in [B,T,H,W,3] -> tiles [count,T,th,tw,3], tiles first .. first+count-1 of the call.
 *   pfnl_op_tile_scatter: y [count,scale th,scale tw,3], the results of those tiles -> their owned rectangles inside out [B,scale H,
 *     scale W,3]; every element of them is stored once by one thread, nothing else in `out` is touched.  No atomics, no memset.
 * Both copy bits.  Rows are contiguous runs of floats and, origins and widths being even, 8-byte aligned relative to their base: 16-byte
 * accesses where the origins, the row lengths and both base pointers allow, else 8-byte, else 4-byte - chosen from the addresses. */
int pfnl_op_tile_gather(const float* in, float* tiles, int B, int T, int H, int W, const pfnl_tiling* t, int first, int count, void* stream);
int pfnl_op_tile_scatter(const float* y, float* out, int B, int H, int W, int scale, const pfnl_tiling* t, int first, int count, void* stream);
/* MFMA operand/accumulator layout self-test (asymmetric operands); returns 0 if the f32
 * 32x32x2 fragment maps this library assumes hold on the device. */
int pfnl_selftest_mfma(int device_id);

#ifdef __cplusplus
}
#endif
#endif /* PFNL_HIP_H */
