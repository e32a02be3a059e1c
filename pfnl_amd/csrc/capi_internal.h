// Internal to libpfnl_hip: shared by the translation units of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pfnl_hip.h"
#include "common.h"

int pfnl_internal_fail(int code, const std::string& msg);   // records msg for pfnl_last_error(); returns code

// return PFNL_ERR_HIP from the enclosing C-ABI function when a HIP call fails
#define HIPCHK(expr)                                                                                                \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess) return pfnl_internal_fail(PFNL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// What the streaming session (capi_stream.hip) needs of a handle, whose layout stays private to capi.hip: its geometry and state, its own
// stream, and the slot that holds the handle's one open session (NULL: none).
struct pfnl_handle;
struct pfnl_stream;
struct pfnl_handle_view {
    int num_frames, scale, device_id;
    bool finalized;
    hipStream_t stream;
    pfnl_stream** session;
};
pfnl_handle_view pfnl_internal_view(pfnl_handle* h);

// An NV12 / I420 surface that surface_refused (surface_geom.h) has passed, as the decode kernel's one frame of planes
inline pfnl::YuvPlanes pfnl_internal_yuv_planes(const pfnl_surface& sf, bool nv12) {
    return pfnl::YuvPlanes{static_cast<const uint8_t*>(sf.plane[0]), static_cast<const uint8_t*>(sf.plane[1]),
                           nv12 ? nullptr : static_cast<const uint8_t*>(sf.plane[2]), sf.pitch[0], sf.pitch[1], nv12 ? 0 : sf.pitch[2], 0};
}

// The 1x1 convolutions of the non-local block folded on the host in fp64 (reference utils.py:18-71), as pfnl_finalize_weights and the op
// hooks use them.  Inputs are [C][C] row-major (in, out); the folded matrices are written with row stride CP (>= C + 1).
// W' = Wg Ww, b' = bg Ww + bw (the rows of the attention sum to 1, so g's bias passes through it)
void pfnl_nl_fold_gw(const float* wg, const float* bg, const float* ww, const float* bw, int C, int CP, float* Wf, float* bf);
// M = Wt Wp^T, c = bt Wp^T (the logits' bilinear form, see nl_qproj_kernel); with bp, also column C (a pad column):
// theta_i . b_phi = X_i (Wt b_phi) + bt . b_phi - the per-query constant of the logits that cancels in the softmax of nltype 0 and does
// not under the relu of nltype 2 (nl_attn_kernel<., DOT>)
void pfnl_nl_fold_theta_phi(const float* wt, const float* bt, const float* wp, const float* bp, int C, int CP, float* Mf, float* cf);
