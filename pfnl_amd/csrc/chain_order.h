// The work order of the persistent 3x3 launches (conv_split16.hip, conv_sf.hip, conv_bf16_v3.hip) and the split-chain geometry the host plans
// and checks.  No HIP runtime calls: tests/test_chain_order.py compiles it for the host and walks the work order of every workgroup.
//
// A chain is the T frames of a clip at one 8 x 32 spatial tile.  The first n_full chains - a whole number of rounds of the grid - are dealt
// out whole, XCD by XCD (workgroup b runs on XCD b & 7; chains of neighbouring tiles share their halo rows in one L2).  SPLIT CHAINS (split_s
// > 0): every chain behind them is cut by frames into split_s parts of <= split_q frames, one part per workgroup (slot = xcd * cpx + xj ->
// chain n_full + slot / split_s, part slot % split_s).  A launch of 1.25 rounds of chains then takes 1 chain + 2 tiles instead of 2 chains.
#pragma once
#include <hip/hip_runtime.h>

namespace pfnl {

constexpr int CHAIN_TH = 8, CHAIN_TW = 32;                          // the spatial tile of a chain

// the grid of the persistent launches: whole XCDs (workgroup b runs on XCD b & 7), at least 8 - what split chains' n_full is a multiple of
inline int persistent_grid(int ncu) { return ncu >= 8 ? ncu / 8 * 8 : 8; }

// chain `ch` -> item = clip * T + f (f: a frame of the clip; T = 1, f = 0: the clip) and the origin of its tile (per_item = tiles_x * tiles_y
// chains per clip)
__host__ __device__ __forceinline__ void chain_tile(int ch, int per_item, int tiles_x, int T, int f, int& item, int& y0, int& x0) {
    const int clip = ch / per_item;
    const int sp = ch - clip * per_item;
    item = clip * T + f;
    const int ty = sp / tiles_x;
    y0 = ty * CHAIN_TH;
    x0 = (sp - ty * tiles_x) * CHAIN_TW;
}

// One workgroup's share: its whole chains, then (SPLIT) its part of a cut chain, frames [sp_f0, sp_f1).  A chain is T + LEAD tiles: with
// LEAD = 1 position 0 is the chain's shared half, which a part recomputes, and frame f sits at position f + 1; with LEAD = 0 position = frame.
// The XCD-major deal takes blockIdx.x & 7, blockIdx.x >> 3 and gridDim.x >> 3, unsigned and read by the caller in that order; nothing past the
// early exit of a launch without split chains is computed in front of it; L = T + LEAD is the caller's own value in every call.  That way the kernels'
// instruction streams stay those of the code once written out in each of them.
//   ChainShare<SPLIT> cs(blockIdx.x & 7, blockIdx.x >> 3, gridDim.x >> 3, nchains, p.n_full);  if (cs.idle()) return;  cs.deal(T + LEAD, s, q);
template <bool SPLIT, int LEAD = 0>
struct ChainShare {
    int nchains, n_full, xcd, xj, cpx, cbeg, ccnt;
    int nfc, nfull_tiles;                                           // whole chains of this workgroup, and their tiles
    int slot, sp_chain, sp_f0, sp_f1;                               // the part: chain sp_chain, frames [sp_f0, sp_f1), partial-sum slot
    bool has_part;
    int nt;                                                         // tiles of this workgroup

    __host__ __device__ __forceinline__ ChainShare(unsigned xcd_, unsigned xj_, unsigned cpx_, int nchains_, int n_full_) : nchains(nchains_) {
        xcd = xcd_;
        xj = xj_;
        cpx = cpx_;
        n_full = SPLIT ? n_full_ : nchains;
        const int per_xcd = (n_full + 7) >> 3;
        cbeg = xcd * per_xcd;
        ccnt = min(per_xcd, n_full - cbeg);
    }
    // without split chains: this workgroup has no chain (surplus workgroups exit at once)
    __host__ __device__ __forceinline__ bool idle() const { return !SPLIT && xj >= ccnt; }
    __host__ __device__ __forceinline__ void deal(int L, int split_s, int split_q) {              // L = T + LEAD: tiles of a whole chain
        nfc = (!SPLIT || xj < ccnt) ? (ccnt - xj + cpx - 1) / cpx : 0;
        nfull_tiles = nfc * L;
        slot = xcd * cpx + xj;
        has_part = SPLIT && slot < (nchains - n_full) * split_s;
        sp_chain = has_part ? n_full + slot / split_s : 0;
        sp_f0 = has_part ? (slot % split_s) * split_q : 0;
        sp_f1 = has_part ? min(L - LEAD, sp_f0 + split_q) : 0;
        nt = nfull_tiles + (has_part ? LEAD + sp_f1 - sp_f0 : 0);
    }

    // by tile: tile k (< nt) -> chain, position in the chain
    __host__ __device__ __forceinline__ void tile(int k, int L, int& ch, int& pos) const {
        if (!SPLIT || k < nfull_tiles) {
            const int ci = k / L;
            pos = k - ci * L;
            ch = cbeg + xj + ci * cpx;
        } else {
            const int kk = k - nfull_tiles;
            pos = (LEAD && kk == 0) ? 0 : sp_f0 + kk;
            ch = sp_chain;
        }
    }
    __host__ __device__ __forceinline__ bool in_part(int k) const { return SPLIT && k >= nfull_tiles; }
    // the position of tile k if it starts a chain (k = 0, or the tile behind a chain's end): a part without a shared half starts at sp_f0
    __host__ __device__ __forceinline__ int head_pos(int k) const { return (!LEAD && SPLIT && k == nfull_tiles) ? sp_f0 : 0; }
    // the position behind the last tile of the chain tile k is in
    __host__ __device__ __forceinline__ int end_pos(int k, int L) const { return in_part(k) ? sp_f1 + LEAD : L; }
};

// The geometry every split launch checks: n_full a multiple of `grid` (persistent_grid) below the chain count, 2 <= split_s <= 7 parts
// (7: what the finalize kernels add up) of <= split_q frames that are all non-empty and together the T frames, one part per workgroup.
inline bool split_geometry_ok(int H, int W, int items, int T, int n_full, int split_s, int split_q, int grid) {
    if (T < 1 || grid < 1) return false;
    const long long nchains = (long long)((W + CHAIN_TW - 1) / CHAIN_TW) * ((H + CHAIN_TH - 1) / CHAIN_TH) * (items / T);
    if (split_s < 2 || split_s > 7 || split_q < 1 || n_full < 0 || n_full % grid || n_full >= nchains) return false;
    if ((long long)split_s * split_q < T || (long long)(split_s - 1) * split_q >= T) return false;
    return (nchains - n_full) * split_s <= grid;
}

// The split rule of the trunk plan.  With R = chains mod grid chains in a last, partial round, a workgroup with one chain more than the others
// sets the time of the launch (5 clips of 128x128 = 1.25 rounds: 7.2 ms against 4.5 for 4).  When at least two parts of a chain fit the idle
// workgroups (R <= grid / 2), those R chains are cut by frames: s = grid / R parts of q = ceil(T / s) frames.  false: no cut.
inline bool split_rule(int chains, int T, int grid, int& n_full, int& split_s, int& split_q) {
    const int R = chains % grid;
    if (T > 7 || chains <= grid || R == 0 || grid / R < 2) return false;
    const int s0 = T < grid / R ? T : grid / R, q = (T + s0 - 1) / s0, s = (T + q - 1) / q;
    if (s < 2) return false;
    n_full = chains - R;
    split_s = s;
    split_q = q;
    return true;
}

}  // namespace pfnl
