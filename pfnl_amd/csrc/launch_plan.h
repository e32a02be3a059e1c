// THE LAUNCH PLAN of a forward: the options that configure it (pfnl_set_option, the environment reads of pfnl_create), the rule that turns
// them and a shape into the kernels a forward launches, and the text pfnl_plan reports.  No HIP runtime calls: tests/test_plan_host.py
// compiles it for the host and walks the rule at any CU count.  capi.hip holds one Options in the handle and runs the plan.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "chain_order.h"

namespace pfnl {

// every field pfnl_set_option or an environment read in pfnl_create sets (the option table: kOptions, below)
struct Options {
    int graph_mode = 0;                                       // 0 off (default: measured slower), 1 auto (frames*H*W <= 65536 pixels), 2 on
    int conv_algo = 5;                                        // conv3x3: 5 auto (4 for large shapes, 3 for small), 0 direct, 1 winograd (4 waves / tile), 3 winograd_ws (persistent, wave-specialised), 4 split16 (f16 MFMA, split fp32 operands)
    int conv1x1_algo = 2;                                     // conv10: 2 streaming kernel on the f16 pipe, split operands (default), 1 streaming f32-MFMA kernel (conv1x1.hip), 0 LDS-tiled implicit GEMM
    bool conv2_grouped = true;                                // winograd: conv2_i as one grouped launch (option conv2=grouped|split)
    bool bf16 = false;                                        // option precision=bf16: progressive-fusion trunk in bf16 (conv_bf16.hip); NL, conv0 maths, merge, tail stay fp32
    bool bf16_fuse10 = true;                                  // bf16 trunk: conv10_i inside the conv1_i launch (option bf16_conv10=fused|separate)
    bool bf16_m16 = true;                                     // bf16 trunk: the two chained 3x3 launches on v_mfma_f32_16x16x32_bf16 (option bf16_mfma=16|32)
    int m1_algo = 0;                                          // convmerge1 with conv3x3=split16: 0 auto (= 1), 1 the split-f16 kernel's accumulating mode, 2 Winograd
    int nl_algo = 2;                                          // non-local block of the fp32 path: 0 f32 MFMA (nonlocal.hip), 1 split-f16 (nonlocal_f16.hip), 2 auto (1 from N = 1024 keys)
    int nl_type = -1;                                         // utils.NonLocalBlock nltype: -1 auto (0 with theta / phi variables, else 1 = PFNL's call), 0, 1, 2
    int nl_sub = 1;                                           // ... sub_sample (utils.py:27-28,35-36); PFNL's call: 1
    bool s16_m16 = true;                                      // option split16_mfma=16|32: the chain launch of conv2_i on v_mfma_f32_16x16x32_f16
    bool strict = false;                                      // option strict_fp32=on (env PFNL_STRICT_FP32): the f32-MFMA kernels from the start (the f16-pipe kernels' DOMAIN: pfnl_handle, capi.hip)
    int small_mode = 0;                                       // option small=auto|on|off: the small-shape trunk kernels (auto: when a launch has < 256 tiles of 8x32 pixels)
    bool small_c10 = true;                                    // ... with conv10_i inside the conv1_i launch (per-frame partials, summed in conv2_i's prologue); false: three launches (small3)
    bool sf_chain = true;                                     // ... and conv2_i is ONE launch (option split16_chain=on|off)
    bool sf_c10 = true;                                       // ... and conv1_i + conv10_i are ONE launch (option split16_c10=on|off)
    bool sf_mid = true;                                       // option split16_mid=auto|off: launches with fewer (clip, tile) chains than sf_mid_chains run the block as four per-tile launches
    int sf_mid_chains = 0;                                    // 0: kMidChains256 scaled by the device's CUs (measured crossover, tools/precision_ladder.py; env PFNL_SF_MID_CHAINS for sweeps)
    bool sf0 = false;                                         // option split16_sf0=off|on: in the two-launch block the chain kernel ALSO writes the block's output in the split
                                                              // format (`inp0sf`), and the next block's conv1_i + conv10_i launch takes its halo from there by LDS-DMA (round 6).
                                                              // Bit-identical; MEASURED SLOWER (configs[1], same box: 4.86 vs 4.45 ms - the chain kernel pays 22 us for the copy,
                                                              // conv1_i + conv10_i gains 0.6: DESIGN.md R6.1), hence off
    bool split_chains = true;                                 // option split16_splitchains=auto|off: in the two-launch block, a batch that is not a whole number of rounds of
                                                              // (clip, tile) chains runs its last, partial round as PARTS of chains cut by frames (conv_split16.h "SPLIT CHAINS")
    bool sf_path = true;                                      // option split16_sf=on|off: with conv3x3 = conv1x1 = split16, conv1_i and conv10_i write the
                                                              // split format (conv_split16.h) and both halves of conv2_i read it by LDS-DMA (conv_sf.hip)
};

// ---- the options of pfnl_set_option / pfnl_get_option: each key sets one int or bool field of Options (a bool takes 0 / 1) to the value
// of one of its names; the first name of a value is the one pfnl_get_option returns.  nl_sub_sample (an integer) and bf16_nonlocal (f16
// only) are the two keys outside the table (capi.hip).
struct OptionField {
    int Options::*i = nullptr;
    bool Options::*b = nullptr;
    constexpr OptionField(int Options::*f) : i(f) {}
    constexpr OptionField(bool Options::*f) : b(f) {}
    int get(const Options& o) const { return i ? o.*i : (int)(o.*b); }
    void set(Options& o, int v) const {
        if (i) o.*i = v;
        else o.*b = v != 0;
    }
};

struct OptionName {
    const char* name;   // (null: past the last name)
    int value;
};

struct OptionSpec {
    const char* key;
    OptionField field;
    OptionName names[8];
    const char* refusal;
    bool set_named(Options& o, const std::string& v) const {   // false: `v` names no value of this key
        for (const OptionName& n : names)
            if (n.name && v == n.name) {
                field.set(o, n.value);
                return true;
            }
        return false;
    }
    const char* name_in(const Options& o) const {              // the (first) name of the field's current value
        const int cur = field.get(o);
        for (const OptionName& n : names)
            if (n.name && n.value == cur) return n.name;
        return "";
    }
};

static const OptionSpec kOptions[] = {
    {"graph", &Options::graph_mode, {{"auto", 1}, {"on", 2}, {"off", 0}}, "graph must be auto, on or off"},
    {"conv3x3", &Options::conv_algo, {{"winograd", 3}, {"winograd_ws", 3}, {"winograd_tile", 1}, {"direct", 0}, {"split16", 4}, {"auto", 5}},
     "conv3x3 must be auto, split16, winograd, winograd_tile or direct"},
    {"strict_fp32", &Options::strict, {{"on", 1}, {"off", 0}}, "strict_fp32 must be on or off"},
    {"small", &Options::small_mode, {{"auto", 0}, {"on", 1}, {"off", 2}}, "small must be auto, on or off"},
    {"split16_chain", &Options::sf_chain, {{"on", 1}, {"off", 0}}, "split16_chain must be on or off"},
    {"split16_c10", &Options::sf_c10, {{"on", 1}, {"off", 0}}, "split16_c10 must be on or off"},
    {"split16_mid", &Options::sf_mid, {{"auto", 1}, {"off", 0}}, "split16_mid must be auto or off"},
    {"split16_sf0", &Options::sf0, {{"on", 1}, {"off", 0}}, "split16_sf0 must be on or off"},
    {"split16_splitchains", &Options::split_chains, {{"auto", 1}, {"off", 0}}, "split16_splitchains must be auto or off"},
    {"split16_sf", &Options::sf_path, {{"on", 1}, {"off", 0}}, "split16_sf must be on or off"},
    {"conv2", &Options::conv2_grouped, {{"grouped", 1}, {"split", 0}}, "conv2 must be grouped or split"},
    {"split16_mfma", &Options::s16_m16, {{"16", 1}, {"32", 0}}, "split16_mfma must be 16 or 32"},
    {"bf16_mfma", &Options::bf16_m16, {{"16", 1}, {"32", 0}}, "bf16_mfma must be 16 or 32"},
    {"bf16_conv10", &Options::bf16_fuse10, {{"fused", 1}, {"separate", 0}}, "bf16_conv10 must be fused or separate"},
    {"precision", &Options::bf16, {{"bf16", 1}, {"fp32", 0}}, "precision must be fp32 or bf16"},
    {"merge1", &Options::m1_algo, {{"auto", 0}, {"split16", 1}, {"winograd", 2}}, "merge1 must be auto, split16 or winograd"},
    {"nl_type", &Options::nl_type,
     {{"auto", -1}, {"0", 0}, {"embedded_gaussian", 0}, {"1", 1}, {"gaussian", 1}, {"2", 2}, {"dot_product", 2}},
     "nl_type: auto | 0 | 1 | 2 (nltype 3, 'concat', builds no graph in the reference either: utils.py:23)"},
    {"small_c10", &Options::small_c10, {{"on", 1}, {"off", 0}}, "small_c10 must be on or off"},
    {"nonlocal", &Options::nl_algo, {{"f32", 0}, {"split16", 1}, {"auto", 2}}, "nonlocal must be auto, f32 or split16"},
    {"conv1x1", &Options::conv1x1_algo, {{"stream", 1}, {"tiled", 0}, {"split16", 2}}, "conv1x1 must be split16, stream or tiled"},
};

inline const OptionSpec* find_option(const std::string& key) {
    for (const OptionSpec& o : kOptions)
        if (key == o.key) return &o;
    return nullptr;
}

// what the plan reads besides the options: the model's frame count, the device and the state of the handle's weights
struct PlanFacts {
    int num_frames = 7;
    int ncu = 0;                                              // CUs of the handle's device: the plan's thresholds and grid
    bool nl_theta = false;                                    // the weights hold the non-local block's theta / phi projections
    bool strict_once = false;                                 // this forward is a range rerun on the f32-MFMA kernels
    bool weights_f16_ok = true;                               // every weight inside binary16's range
};

// a 3x3 launch with fewer tiles of 8x32 pixels than this takes the small-shape trunk (conv_small.hip) under the default choices; from
// here on the split-f16 kernels' per-tile launches are faster (tools/precision_ladder.py: 210 - 224 tiles 1.99 - 2.14 -> 1.85 - 1.90 ms;
// 168 tiles 1.08 against 1.88).  256 (a tile per CU) until round 5.
// Both work-order thresholds were measured on the 256-CU part and are a fraction of the CUs a launch can occupy: they scale with
// the CU count of the handle's device (a CPX partition or a smaller device keeps the same tiles-per-CU crossover).
static constexpr int kSmallTiles256 = 200;                  // tiles of 8x32 pixels per 3x3 launch below which the small-shape trunk runs (0.78 per CU)
static constexpr int kMidChains256 = 136;                   // (clip, tile) chains below which a block runs as four per-tile launches (0.53 per CU)
inline int scaled_by_cus(int v256, int ncu) {
    return ncu > 0 && ncu != 256 ? std::max(1, (int)((long long)v256 * ncu / 256)) : v256;
}

// convmerge1 (model/pfnl.py:73-74): which launch computes it
enum Merge1Kind {
    M1_SMALL,         // conv_small.hip: T sources, cout 48 zero-padded to 64
    M1_BF16,          // the accumulating mode of the bf16 3x3 kernel
    M1_SPLIT16,       // the accumulating mode of conv3x3_split16_kernel
    M1_SPLIT16_CUT,   // ... with the trunk's split chains, + c10_finalize_kernel
    M1_WINOGRAD,      // the accumulating mode of the persistent Winograd kernel
    M1_DIRECT,        // conv_mfma: 3x3 over the concat of T frames, cout 48
};
static const char* const kMerge1Names[] = {"small", "bf16", "split16", "split16_cut", "winograd", "direct"};

// THE LAUNCH PLAN of a forward for a shape under the handle's current options: the one place the dispatch rule lives.
// forward_device runs it, pfnl_workspace_bytes sizes from it, pfnl_plan reports it (bench.py's byte model and the tests read it there).
struct TrunkPlan {
    bool bf16 = false;
    bool strict = false;                   // fp32: f32-MFMA kernels only (strict_fp32, a range rerun, weights beyond binary16): trunk, non-local block, conv0
    int nltype = 1;                        // utils.NonLocalBlock nltype, resolved (option nl_type -1 = auto)
    int nl_family = 0;                     // the non-local block's kernels: 0 the general form (nltype 0 / 2 or sub-sampling: f32 MFMA), 1 the f16 pipe with
                                           // exactly split operands (fp32 precision, from 1024 keys), 2 the f16 pipe on the hi parts (precision bf16), 3 f32 MFMA
    bool nl_fused_pack = false;            // families 1 / 2: one pack launch writes X fp32 + the binary16 K / V^T operands (round 6)
    // bf16 trunk
    bool bmid = false, fuse10 = false;
    // fp32 trunk
    int algo = 0, conv1x1_algo = 0;        // resolved 3x3 / 1x1 algorithm (conv_algo 5 = auto is resolved here)
    bool sf = false;                       // inp1 and base in the split format
    bool small = false, small_c10 = false; // conv_small.hip: 3 (2 with small_c10) launches per block
    bool mid = false;                      // four per-tile launches per block
    bool c10_fused = false;                // conv1_i + conv10_i in one launch (conv3x3_c1c10_kernel)
    bool chain = false;                    // conv2_i in one launch (conv3x3_sf_chain_kernel)
    bool sf0 = false;                      // chain2 only: split-format copy of the block output, conv1_i's halo by LDS-DMA
    bool conv2_grouped = false;            // Winograd: conv2_i as one grouped launch
    int n_full = 0, split_s = 0, split_q = 0;   // chain2 only: SPLIT CHAINS (conv_split16.h) - the chains behind the first n_full are cut into split_s parts of <= split_q frames
    int c1x1_launches = 0;                 // launches per block of class conv1x1 (conv10_i on its own / c10_finalize_kernel)
    int launches_per_block = 0;
    int tiles8x32 = 0, chains = 0;
    int mfma = 32;                         // MFMA shape of the chained 3x3 launches: 16 = v_mfma_f32_16x16x32_* (bf16: conv_bf16_v3.hip M16; fp32: the chain launch
                                           // of conv2_i, conv3x3_sf_chain16_kernel - whole rounds of at least a chain per CU only), 32 = 32x32x16
    int c1_mfma = 32;                      // fp32: MFMA shape of conv1_i's 3x3 stage in the fused conv1_i + conv10_i launch (conv3x3_c1c10_kernel; 16 exactly where mfma is)
    int merge1 = M1_DIRECT;                // convmerge1's launch (Merge1Kind)
    int merge_stride = 48;                 // floats per pixel of `merge` as convmerge1 writes it
    // the trunk's buffers that depend on the plan (floats): the small-shape trunk's conv10_i partials [B*T][H][W][64]; the split-format copy of
    // inp0 [B*T][H][W] x 256 B; split chains' partial sums [slot][8][32][64] (conv10_i's, then convmerge1's)
    size_t p10_floats = 0, inp0sf_floats = 0, c10part_floats = 0;
    const char* name = "";
};

inline void plan_bf16_trunk(const Options& opt, TrunkPlan& pl, int T, int grid, int mid_chains, bool fits32) {
    // MID shapes (as in the fp32 trunk): with fewer (clip, tile) chains than mid_chains the chained launches leave most CUs idle
    pl.bmid = opt.sf_mid && opt.bf16_fuse10 && pl.chains < mid_chains;
    pl.fuse10 = opt.bf16_fuse10 && !pl.bmid;
    pl.launches_per_block = pl.fuse10 ? 3 : 4;
    pl.c1x1_launches = pl.fuse10 ? 0 : 1;
    // SPLIT CHAINS of the two chained launches (chain_order.h, split_rule)
    if (pl.fuse10 && opt.split_chains && fits32 && split_rule(pl.chains, T, grid, pl.n_full, pl.split_s, pl.split_q)) {
        pl.launches_per_block += 1;                                     // c10_finalize_bf16_kernel
        pl.c1x1_launches = 1;
    }
    pl.name = pl.bmid ? "bf16_mid4" : (pl.fuse10 ? (pl.split_s ? "bf16_3_split" : "bf16_3") : "bf16_4");
    pl.mfma = opt.bf16_m16 ? 16 : 32;
    pl.merge1 = M1_BF16;
    pl.merge_stride = 64;
}

inline void plan_fp32_trunk(const Options& opt, int ncu, TrunkPlan& pl, int B, int H, int W, int T, int grid, int mid_chains, bool fits32) {
    // conv3x3 = auto (default): the split-f16 kernels when a launch has at least ~0.78 tiles per CU, the Winograd f32 kernel below
    const int small_tiles = scaled_by_cus(kSmallTiles256, ncu);
    const int algo0 = opt.conv_algo == 5 ? ((pl.tiles8x32 >= small_tiles && fits32) ? 4 : 3) : opt.conv_algo;
    pl.algo = (pl.strict && algo0 == 4) ? 3 : algo0;
    pl.conv1x1_algo = (pl.strict && opt.conv1x1_algo == 2) ? 1 : opt.conv1x1_algo;
    pl.sf = pl.algo == 4 && pl.conv1x1_algo == 2 && opt.sf_path;
    // small shapes (BASELINE.json configs[0], configs[4]): the trunk through conv_small.hip; only under the default algorithm choices
    pl.small = !pl.strict && fits32 &&
               (opt.small_mode == 1 || (opt.small_mode == 0 && opt.conv_algo == 5 && opt.conv1x1_algo == 2 && pl.tiles8x32 < small_tiles));
    pl.small_c10 = pl.small && opt.small_c10;
    if (pl.small) {
        pl.launches_per_block = pl.small_c10 ? 2 : 3;
        pl.c1x1_launches = pl.small_c10 ? 0 : 1;
        pl.name = pl.small_c10 ? "small2" : "small3";
        pl.merge1 = M1_SMALL;
        pl.merge_stride = 64;
        return;
    }
    pl.mid = pl.sf && opt.sf_mid && opt.conv_algo == 5 && opt.sf_c10 && opt.sf_chain && pl.chains < mid_chains;   // (only under the default choices, like `small`)
    pl.c10_fused = pl.sf && opt.sf_c10 && !pl.mid;
    pl.chain = pl.sf && opt.sf_chain && !pl.mid;
    pl.sf0 = pl.c10_fused && pl.chain && opt.sf0;
    // grouped / accumulating Winograd modes chain T(+1) units inside one workgroup: only worth it when there are enough (clip, 4x32-pixel tile)
    // groups to occupy the chip (below ~220 the split launches finish sooner)
    const int wino_groups = B * ((W + 31) / 32) * ((H + 3) / 4);
    pl.conv2_grouped = pl.algo == 3 && opt.conv2_grouped && wino_groups >= 224 && fits32;
    pl.launches_per_block = (pl.c10_fused ? 1 : 2) + ((pl.chain || pl.conv2_grouped) ? 1 : 2);
    pl.c1x1_launches = pl.c10_fused ? 0 : 1;
    // SPLIT CHAINS of conv1_i + conv10_i and conv2_i (chain_order.h, split_rule)
    if (pl.c10_fused && pl.chain && opt.split_chains && split_rule(pl.chains, T, grid, pl.n_full, pl.split_s, pl.split_q)) {
        pl.launches_per_block += 1;                                     // c10_finalize_kernel
        pl.c1x1_launches = 1;
    }
    // the chain launch on 16x16x32: where every CU has a chain the launch sits on the power cap and the shape's energy counts; below that (UDM10: 230
    // chains) its extra cycles do (+0.9 %); split chains and the split-format copy stay on the 32x32x16 kernel
    pl.mfma = (opt.s16_m16 && pl.c10_fused && pl.chain && !pl.sf0 && !pl.split_s && pl.chains >= grid) ? 16 : 32;
    pl.c1_mfma = pl.mfma;                                               // conv1_i's stage of the other launch of the block: the same rule
    pl.name = pl.mid ? "mid4" : (pl.c10_fused && pl.chain) ? (pl.sf0 ? "chain2_sf0" : (pl.split_s ? "chain2_split" : "chain2"))
            : pl.algo == 4 ? (pl.launches_per_block == 3 ? "split16_3" : "split16_4")
            : pl.algo == 3 ? (pl.conv2_grouped ? "winograd_ws3" : "winograd_ws4")
            : pl.algo == 1 ? "winograd_tile4" : "direct4";
    // convmerge1: on the f16 pipe with the split-f16 trunk (convmerge1's chains are the trunk's: a cut last round is cut here too), else the
    // persistent Winograd kernel where there are enough groups, else the direct kernel
    if (pl.algo == 4 && opt.m1_algo != 2 && fits32) pl.merge1 = pl.split_s ? M1_SPLIT16_CUT : M1_SPLIT16;
    else if ((pl.algo == 3 || pl.algo == 4) && wino_groups >= 224 && fits32) pl.merge1 = M1_WINOGRAD;
    pl.merge_stride = pl.merge1 == M1_DIRECT ? 48 : 64;
}

// H: the rows the trunk buffers hold (a strip's with its halo); Hfull: the frame's (the non-local block's keys are global);
// nl_fits: the packed operands of the non-local block's f16-pipe kernels fit one launch (nl_f16_fits_one_launch, nonlocal_f16.hip)
inline TrunkPlan trunk_plan(const Options& opt, const PlanFacts& facts, int B, int H, int W, int Hfull, bool nl_fits) {
    TrunkPlan pl;
    const int T = facts.num_frames;
    pl.bf16 = opt.bf16;
    pl.strict = !opt.bf16 && (opt.strict || facts.strict_once || !facts.weights_f16_ok);
    pl.tiles8x32 = B * T * ((W + 31) / 32) * ((H + 7) / 8);
    pl.chains = pl.tiles8x32 / T;
    const int grid = persistent_grid(facts.ncu);
    const int mid_chains = opt.sf_mid_chains > 0 ? opt.sf_mid_chains : scaled_by_cus(kMidChains256, facts.ncu);
    const bool fits32 = (long long)H * W * 256 < 0x7fffffffLL;
    if (opt.bf16) plan_bf16_trunk(opt, pl, T, grid, mid_chains, fits32);
    else plan_fp32_trunk(opt, facts.ncu, pl, B, H, W, T, grid, mid_chains, fits32);

    const int N = (Hfull / 2) * (W / 2);
    pl.nltype = opt.nl_type < 0 ? (facts.nl_theta ? 0 : 1) : opt.nl_type;
    pl.nl_family = (pl.nltype != 1 || opt.nl_sub > 1) ? 0
                 : opt.bf16 ? 2
                 : (!pl.strict && (opt.nl_algo == 1 || (opt.nl_algo == 2 && N >= 1024))) ? 1 : 3;
    pl.nl_fused_pack = (pl.nl_family == 1 || pl.nl_family == 2) && nl_fits;

    const size_t frame_floats = (size_t)B * T * H * W * 64;
    pl.p10_floats = pl.small_c10 ? frame_floats : 0;
    pl.inp0sf_floats = pl.sf0 ? frame_floats : 0;
    pl.c10part_floats = pl.split_s ? (size_t)(pl.chains - pl.n_full) * pl.split_s * 8 * 32 * 64 : 0;
    return pl;
}

// the text of pfnl_plan (include/pfnl_hip.h): the structure's name, then key=value fields
inline std::string plan_text(const TrunkPlan& pl) {
    static const char* const nln[] = {"general_f32", "split16", "f16", "f32"};
    static const char* const a3[] = {"direct", "winograd_tile", "?", "winograd", "split16"};
    static const char* const a1[] = {"tiled", "stream", "split16"};
    char tmp[384];
    if (pl.bf16)
        std::snprintf(tmp, sizeof tmp, "%s launches_per_block=%d c1x1=%d precision=bf16 tiles=%d chains=%d whole_chains=%d split_parts=%d part_frames=%d nl=%s nl_pack_fused=%d mfma=%d merge1=%s",
                      pl.name, pl.launches_per_block, pl.c1x1_launches, pl.tiles8x32, pl.chains, pl.split_s ? pl.n_full : pl.chains, pl.split_s, pl.split_q,
                      nln[pl.nl_family], pl.nl_fused_pack ? 1 : 0, pl.mfma, kMerge1Names[pl.merge1]);
    else
        std::snprintf(tmp, sizeof tmp, "%s launches_per_block=%d c1x1=%d precision=fp32 conv3x3=%s conv1x1=%s c10_fused=%d chain=%d sf0=%d strict=%d tiles=%d chains=%d "
                      "whole_chains=%d split_parts=%d part_frames=%d nl=%s nl_pack_fused=%d mfma=%d c1_mfma=%d merge1=%s",
                      pl.name, pl.launches_per_block, pl.c1x1_launches, pl.small ? "small" : a3[pl.algo < 0 || pl.algo > 4 ? 2 : pl.algo],
                      a1[pl.conv1x1_algo < 0 || pl.conv1x1_algo > 2 ? 0 : pl.conv1x1_algo], pl.c10_fused ? 1 : 0, pl.chain ? 1 : 0, pl.sf0 ? 1 : 0,
                      pl.strict ? 1 : 0, pl.tiles8x32, pl.chains, pl.split_s ? pl.n_full : pl.chains, pl.split_s, pl.split_q, nln[pl.nl_family],
                      pl.nl_fused_pack ? 1 : 0, pl.mfma, pl.c1_mfma, kMerge1Names[pl.merge1]);
    return tmp;
}

}  // namespace pfnl
