"""Single-op entry points of libpfnl_hip (the TF kernels the reference calls), on torch-ROCm
device tensors.  Used by the per-op parity tests; ``PFNLEngine.forward`` does not go through here.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _capi


def _req(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous float32 tensor on the GPU")
    return C.c_void_p(t.data_ptr())


def _req16(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous bfloat16 tensor on the GPU")
    return C.c_void_p(t.data_ptr())


def _host(a, name) -> Optional[np.ndarray]:
    if a is None:
        return None
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _out(out, shape, dtype, device, name="out"):
    """``out`` where the caller gave one (a tensor of exactly that shape and type, written in place), else a fresh tensor."""
    import torch
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device:
        raise ValueError(f"{name} must be a {dtype} tensor of shape {tuple(shape)} on {device}")
    return out


def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def conv2d(x, kernel, bias=None, act=True, frames_per_item=1, addend=None, add_div=1, resid=None, out=None):
    """tf.layers.Conv2D(k in {1,3}, 'same') [+ bias] [+ addend] [lrelu] [+ resid] via the MFMA kernel.

    x: [items*frames_per_item, H, W, 64] (cuda) viewed as [items, H, W, 64*fpi]; kernel: HWIO host
    array [k,k,64*fpi,cout], cout <= 64.  Reference: model/pfnl.py:49-52 applied at :66-74."""
    import torch
    lib = _capi.load_library()
    k = _host(kernel, "kernel")
    b = _host(bias, "bias")
    ks, _, cin, cout = k.shape
    F, H, W, c = x.shape
    if c != 64 or cin != 64 * frames_per_item or F % frames_per_item:
        raise ValueError("conv2d: channel / frame grouping mismatch")
    items = F // frames_per_item
    out = _out(out, (items, H, W, cout), torch.float32, x.device)
    _capi.check(lib.pfnl_op_conv2d(
        _req(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
        _req(addend, "addend") if addend is not None else None, int(add_div),
        _req(resid, "resid") if resid is not None else None, _req(out, "out"),
        items, frames_per_item, H, W, ks, cout, 1 if act else 0, _stream(x)))
    return out


def conv2_grouped(x, base, kernel, bias, resid, frames_per_clip, act=True, out=None):
    """conv2_i of the reference in one launch: resid + act(conv3x3(concat([base[clip], x[frame]])) + bias).
    x/resid [clips*T, H, W, 64], base [clips, H, W, 64] (cuda); kernel HWIO [3,3,128,64].
    Reference: model/pfnl.py:51, :69-71."""
    import torch
    lib = _capi.load_library()
    k = _host(kernel, "kernel")
    b = _host(bias, "bias")
    F, H, W, c = x.shape
    if k.shape != (3, 3, 128, 64) or c != 64 or F % frames_per_clip or base.shape != (F // frames_per_clip, H, W, 64):
        raise ValueError("conv2_grouped: geometry mismatch")
    out = _out(out, x.shape, torch.float32, x.device)
    _capi.check(lib.pfnl_op_conv2_grouped(
        _req(x, "x"), _req(base, "base"), k.ctypes.data_as(C.c_void_p),
        b.ctypes.data_as(C.c_void_p) if b is not None else None, _req(resid, "resid"), _req(out, "out"),
        F // frames_per_clip, frames_per_clip, H, W, 1 if act else 0, _stream(x)))
    return out


def conv3x3_accum(x, kernel, bias=None, act=True, frames_per_clip=1, variant="winograd", out=None):
    """convmerge1: 3x3 over the concat of `frames_per_clip` frames, (64*fpc) -> cout <= 64, one accumulating
    launch of the persistent Winograd kernel (variant "winograd": even H, W) or of the split-f16 kernel ("split16").
    x [clips*fpc, H, W, 64] (cuda); kernel HWIO [3,3,64*fpc,cout]; returns [clips, H, W, cout].
    Reference: model/pfnl.py:52, :73-74."""
    import torch
    lib = _capi.load_library()
    k = _host(kernel, "kernel")
    b = _host(bias, "bias")
    F, H, W, c = x.shape
    cout = k.shape[3]
    if k.shape[:3] != (3, 3, 64 * frames_per_clip) or c != 64 or F % frames_per_clip or cout > 64:
        raise ValueError("conv3x3_accum: geometry mismatch")
    out = _out(out, (F // frames_per_clip, H, W, 64), torch.float32, x.device)    # (all 64 channels; the result is its first cout)
    fn = lib.pfnl_op_conv3x3_accum_split16 if variant == "split16" else lib.pfnl_op_conv3x3_accum
    _capi.check(fn(
        _req(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
        _req(out, "out"), F // frames_per_clip, frames_per_clip, H, W, cout, 1 if act else 0, _stream(x)))
    return out[..., :cout]


def conv3x3_bf16(x, kernel, bias=None, act=True, addend=None, add_div=1, resid=None, out=None):
    """bf16 trunk: 3x3 64->64 'same' convolution on bf16 MFMA, fp32 accumulation; out = act(conv + bias + addend) + resid.
    x / addend / resid / result: bfloat16 [items, H, W, 64] (cuda); kernel fp32 HWIO [3,3,64,64] (rounded inside).
    Reference: model/pfnl.py:49,51 applied at :66,69-71."""
    import torch
    lib = _capi.load_library()
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    F, H, W, c = x.shape
    if k.shape != (3, 3, 64, 64) or c != 64 or (addend is None) != (resid is None):
        raise ValueError("conv3x3_bf16: geometry mismatch")
    out = _out(out, x.shape, torch.bfloat16, x.device)
    _capi.check(lib.pfnl_op_conv3x3_bf16(
        _req16(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
        _req16(addend, "addend") if addend is not None else None, add_div,
        _req16(resid, "resid") if resid is not None else None, _req16(out, "out"), F, H, W, 1 if act else 0, _stream(x)))
    return out


def conv1_conv10_bf16(x, k1, b1, k10, b10, frames_per_clip, out1=None, base=None):
    """bf16 trunk: conv1_i + conv10_i in one launch.  x bfloat16 [clips*T, H, W, 64] -> (lrelu(conv3x3(x)+b1) bfloat16,
    lrelu(conv1x1 over the T outputs + b10) bfloat16 [clips, H, W, 64]).  Reference: model/pfnl.py:66-68."""
    import torch
    lib = _capi.load_library()
    k1h, b1h, k10h, b10h = _host(k1, "k1"), _host(b1, "b1"), _host(k10, "k10"), _host(b10, "b10")
    F, H, W, c = x.shape
    T = frames_per_clip
    if k1h.shape != (3, 3, 64, 64) or k10h.shape != (1, 1, 64 * T, 64) or c != 64 or F % T:
        raise ValueError("conv1_conv10_bf16: geometry mismatch")
    out1 = _out(out1, x.shape, torch.bfloat16, x.device, "out1")
    base = _out(base, (F // T, H, W, 64), torch.bfloat16, x.device, "base")
    _capi.check(lib.pfnl_op_conv1_conv10_bf16(
        _req16(x, "x"), k1h.ctypes.data_as(C.c_void_p), b1h.ctypes.data_as(C.c_void_p) if b1h is not None else None,
        k10h.ctypes.data_as(C.c_void_p), b10h.ctypes.data_as(C.c_void_p) if b10h is not None else None,
        _req16(out1, "out1"), _req16(base, "base"), F // T, T, H, W, _stream(x)))
    return out1, base


def conv3x3_accum_bf16(x, kernel, bias=None, act=True, frames_per_clip=7, out=None):
    """bf16 trunk -> convmerge1: 3x3 over the concat of `frames_per_clip` frames, (64*fpc) -> cout <= 64, fp32 out
    [clips, H, W, 64] (channels >= cout hold act(0)).  x bfloat16 [clips*fpc, H, W, 64]; kernel fp32 HWIO [3,3,64*fpc,cout].
    Reference: model/pfnl.py:52, :73-74."""
    import torch
    lib = _capi.load_library()
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    F, H, W, c = x.shape
    T = frames_per_clip
    if k.shape[:3] != (3, 3, 64 * T) or k.shape[3] > 64 or c != 64 or F % T:
        raise ValueError("conv3x3_accum_bf16: geometry mismatch")
    out = _out(out, (F // T, H, W, 64), torch.float32, x.device)
    _capi.check(lib.pfnl_op_conv3x3_accum_bf16(
        _req16(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
        _req(out, "out"), F // T, T, H, W, int(k.shape[3]), 1 if act else 0, _stream(x)))
    return out


def conv1x1_bf16(x, kernel, bias=None, act=True, frames_per_item=7, out=None):
    """bf16 trunk: conv10_i, 1x1 over the concat of `frames_per_item` frames.  x bfloat16 [items*fpi, H, W, 64];
    kernel fp32 HWIO [1,1,64*fpi,64].  Reference: model/pfnl.py:50, :67-68."""
    import torch
    lib = _capi.load_library()
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    F, H, W, c = x.shape
    if k.shape != (1, 1, 64 * frames_per_item, 64) or c != 64 or F % frames_per_item:
        raise ValueError("conv1x1_bf16: geometry mismatch")
    items = F // frames_per_item
    out = _out(out, (items, H, W, 64), torch.bfloat16, x.device)
    _capi.check(lib.pfnl_op_conv1x1_bf16(
        _req16(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
        _req16(out, "out"), items, frames_per_item, H * W, 1 if act else 0, _stream(x)))
    return out


def conv1x1_stream(x, kernel, bias=None, act=True, frames_per_item=1, variant="stream", out=None):
    """conv10_i: 1x1 over the concat of `frames_per_item` frames, (64*fpi) -> 64, streaming kernel.
    x: [items*fpi, H, W, 64] (cuda); kernel HWIO [1,1,64*fpi,64].  Reference: model/pfnl.py:50, :67-68."""
    import torch
    lib = _capi.load_library()
    k = _host(kernel, "kernel")
    b = _host(bias, "bias")
    F, H, W, c = x.shape
    if k.shape != (1, 1, 64 * frames_per_item, 64) or c != 64 or F % frames_per_item:
        raise ValueError("conv1x1_stream: geometry mismatch")
    items = F // frames_per_item
    out = _out(out, (items, H, W, 64), torch.float32, x.device)
    if variant.startswith("split16_sf"):                  # "split16_sf:io" - i, o in {0, 1}: input / output in the split format
        i_sf, o_sf = int(variant[-2]), int(variant[-1])
        _capi.check(lib.pfnl_op_conv1x1_split16_sf(
            _req(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
            _req(out, "out"), items, frames_per_item, H * W, 1 if act else 0, i_sf, o_sf, _stream(x)))
        return out
    fn = lib.pfnl_op_conv1x1_split16 if variant == "split16" else lib.pfnl_op_conv1x1_stream
    _capi.check(fn(
        _req(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
        _req(out, "out"), items, frames_per_item, H * W, 1 if act else 0, _stream(x)))
    return out


def conv_small(b, kernel, bias=None, a=None, a_div=1, b_mul=1, resid=None, items=None, act=True, out=None):
    """The small-shape trunk kernel (conv_small.hip): out[i] = act(sum_s conv(src(i, s)) + bias) (+ resid[i]) with
    src(i, s) = a[i // a_div] for s < nA (nA = 1 if `a` is given) else b[i * b_mul + s - nA]; kernel HWIO [ks, ks, 64 * nsrc, cout]."""
    import torch
    lib = _capi.load_library()
    k = _host(kernel, "kernel")
    bs = _host(bias, "bias")
    ks, _, cin, cout = k.shape
    nsrc = cin // 64
    nA = 1 if a is not None else 0
    Fb, H, W, c = b.shape
    if items is None:
        items = Fb // b_mul
    if out is None:
        out = torch.zeros((items, H, W, 64), dtype=torch.float32, device=b.device)
    else:
        _out(out, (items, H, W, 64), torch.float32, b.device)
    _capi.check(lib.pfnl_op_conv_small(
        _req(a, "a") if a is not None else None, _req(b, "b"), nA, int(a_div), int(b_mul), nsrc, k.ctypes.data_as(C.c_void_p),
        bs.ctypes.data_as(C.c_void_p) if bs is not None else None, _req(resid, "resid") if resid is not None else None,
        _req(out, "out"), items, H, W, ks, cout, 1 if act else 0, _stream(b)))
    return out


def conv_small_pf_block(x, k1, b1, k10, b10, k2, b2, T, inp1=None, out=None):
    """One progressive-fusion block on the small-shape kernels, two launches (pfnl_op_conv_small_pf_block; reference
    model/pfnl.py:66-71): x [clips*T,H,W,64] (cuda) -> (inp1, x + inp2)."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = x.shape
    hs = [_host(a, n) for a, n in ((k1, "k1"), (b1, "b1"), (k10, "k10"), (b10, "b10"), (k2, "k2"), (b2, "b2"))]
    inp1 = _out(inp1, x.shape, torch.float32, x.device, "inp1")
    out = _out(out, x.shape, torch.float32, x.device)
    _capi.check(lib.pfnl_op_conv_small_pf_block(_req(x, "x"), *[a.ctypes.data_as(C.c_void_p) for a in hs], _req(inp1, "inp1"), _req(out, "out"),
                                                F // T, int(T), H, W, _stream(x)))
    return inp1, out


def conv3x3_winograd(x, kernel, bias=None, act=True, addend=None, add_div=1, resid=None, variant="winograd", out=None):
    """The 3x3 64->64 'same' convolution through the fused Winograd F(2x2,3x3) kernel (even H, W)."""
    import torch
    lib = _capi.load_library()
    k = _host(kernel, "kernel")
    b = _host(bias, "bias")
    if k.shape != (3, 3, 64, 64) and variant != "split16_sf_chain":
        raise ValueError("winograd path is 3x3, 64 -> 64 only")
    F, H, W, c = x.shape
    out = _out(out, (F, H, W, 64), torch.float32, x.device)
    if variant in ("split16_sf_in", "split16_sf_out", "split16_sf_chain"):   # the split-format kernels (conv_sf.hip / conv1_i writing SF), fp32 at this interface
        if variant != "split16_sf_chain" and k.shape != (3, 3, 64, 64):
            raise ValueError("3x3, 64 -> 64 only")
        _capi.check(lib.pfnl_op_conv3x3_split16_sf(
            {"split16_sf_in": 0, "split16_sf_out": 1, "split16_sf_chain": 2}[variant],
            _req(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
            _req(addend, "addend") if addend is not None else None, int(add_div),
            _req(resid, "resid") if resid is not None else None, _req(out, "out"), F, H, W, 1 if act else 0, _stream(x)))
        return out
    fn = {"winograd": lib.pfnl_op_conv3x3_winograd, "winograd_ws": lib.pfnl_op_conv3x3_winograd_ws,
          "split16": lib.pfnl_op_conv3x3_split16}[variant]
    _capi.check(fn(
        _req(x, "x"), k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
        _req(addend, "addend") if addend is not None else None, int(add_div),
        _req(resid, "resid") if resid is not None else None, _req(out, "out"), F, H, W, 1 if act else 0, _stream(x)))
    return out


def nonlocal_residual(x, wg, bg, ww, bw, precision="fp32", out=None):
    """x [B,T,H,W,3] (cuda) -> [B,H,W,3T] = stack + depth_to_space(NonLocalBlock(space_to_depth(stack)))
    (reference utils.py:18-71 with nltype=1, model/pfnl.py:55-60)."""
    import torch
    lib = _capi.load_library()
    B, T, H, W, c = x.shape
    C_ = 12 * T
    arrs = [_host(a, n) for a, n in ((wg, "wg"), (bg, "bg"), (ww, "ww"), (bw, "bw"))]
    if arrs[0].size != C_ * C_ or arrs[2].size != C_ * C_ or arrs[1].size != C_ or arrs[3].size != C_:
        raise ValueError("nonlocal: weight shapes do not match 12*T channels")
    out = _out(out, (B, H, W, 3 * T), torch.float32, x.device)
    fn = {"split16": lib.pfnl_op_nonlocal_split16, "f16": lib.pfnl_op_nonlocal_f16}.get(precision, lib.pfnl_op_nonlocal)
    _capi.check(fn(_req(x, "x"), *[a.ctypes.data_as(C.c_void_p) for a in arrs],
                                     _req(out, "out"), B, T, H, W, _stream(x)))
    return out


def bicubic(x, scale: int, out=None):
    """TF1.12 legacy ResizeBicubic (reference model/pfnl.py:63): x [B,H,W,3] (cuda) -> [B,sH,sW,3]."""
    import torch
    lib = _capi.load_library()
    B, H, W, c = x.shape
    if c != 3:
        raise ValueError("bicubic expects 3 channels")
    out = _out(out, (B, scale * H, scale * W, 3), torch.float32, x.device)
    _capi.check(lib.pfnl_op_bicubic(_req(x, "x"), _req(out, "out"), B, H, W, scale, _stream(x)))
    return out


def _dihedral_shape(x, k, name):
    if not (isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 0 <= int(k) <= 7):
        raise ValueError(f"member k must lie in 0 .. 7, got {k!r}")
    if x.dim() < 3 or x.shape[-1] != 3 or x.numel() == 0:
        raise ValueError(f"{name}: expected [..., H, W, 3], got {tuple(x.shape)}")
    H, W = int(x.shape[-3]), int(x.shape[-2])
    return int(k), x.numel() // (H * W * 3), H, W


def dihedral(x, k: int, out=None, scale: float = 1.0):
    """Member k of the self-ensemble's group (pfnl_amd/ensemble.py transform): x [..., H, W, 3] (cuda) -> [..., H, W, 3], or
    [..., W, H, 3] for k >= 4, times ``scale`` (1: the bits as they are).  ``out``: a contiguous tensor of that shape to fill."""
    import torch
    lib = _capi.load_library()
    k, n, H, W = _dihedral_shape(x, k, "x")
    shape = tuple(x.shape[:-3]) + ((W, H, 3) if k & 4 else (H, W, 3))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out must have shape {shape}, got {tuple(out.shape)}")
    _capi.check(lib.pfnl_op_dihedral(_req(x, "x"), _req(out, "out"), n, H, W, k, float(scale), _stream(x)))
    return out


def dihedral_accum(acc, y, k: int, scale: float = 1.0):
    """acc = (acc + inverse(y, k)) * scale in place, float32, one thread per element (pfnl_amd/ensemble.py inverse; the step of
    ``combine``): acc [..., H, W, 3] (cuda), y of the same shape, or [..., W, H, 3] for k >= 4.  Returns acc."""
    lib = _capi.load_library()
    k, n, H, W = _dihedral_shape(acc, k, "acc")
    want = tuple(acc.shape[:-3]) + ((W, H, 3) if k & 4 else (H, W, 3))
    if tuple(y.shape) != want:
        raise ValueError(f"y must have shape {want}, got {tuple(y.shape)}")
    _capi.check(lib.pfnl_op_dihedral_accum(_req(acc, "acc"), _req(y, "y"), n, H, W, k, float(scale), _stream(acc)))
    return acc


def _tile_run(B, H, W, tile, first, count):
    """(the tiling as the C-ABI takes it, th, tw, first, count) for tiles first .. first+count-1 (count None: all from ``first`` on) of a
    call [B,.,H,W,3]; ValueError as pfnl_amd/tiles.py ``check``."""
    from . import tiles
    t = tiles.check(H, W, tile)
    th, tw, rows, cols = tiles.grid(H, W, t)
    total = B * len(rows) * len(cols)
    first = int(first)
    count = total - first if count is None else int(count)
    if first < 0 or count < 1 or first + count > total:
        raise ValueError(f"tiles {first} .. {first + count - 1} are not tiles of the call (it has {total})")
    return _capi.pfnl_tiling(*t), th, tw, first, count


def tile_gather(x, tile, first: int = 0, count=None, out=None):
    """Tiles first .. first+count-1 of x [B,T,H,W,3] (cuda) as a stack [count,T,th,tw,3] (pfnl_amd/tiles.py split; ``count`` None: all
    from ``first`` on).  ``out``: a contiguous tensor of that shape to fill."""
    import torch
    lib = _capi.load_library()
    if x.dim() != 5 or x.shape[-1] != 3 or x.numel() == 0:
        raise ValueError(f"x: expected [B,T,H,W,3], got {tuple(x.shape)}")
    B, T, H, W = (int(v) for v in x.shape[:4])
    t, th, tw, first, count = _tile_run(B, H, W, tile, first, count)
    shape = (count, T, th, tw, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out must have shape {shape}, got {tuple(out.shape)}")
    _capi.check(lib.pfnl_op_tile_gather(_req(x, "x"), _req(out, "out"), B, T, H, W, C.byref(t), first, count, _stream(x)))
    return out


def tile_scatter(y, out, tile, scale: int, first: int = 0):
    """The owned rectangles of the tile results y [count,(1,)s*th,s*tw,3] (cuda), tiles first .. first+count-1 of the call, into ``out``
    [B,(1,)s*H,s*W,3] in place (pfnl_amd/tiles.py assemble); every element of the rectangles is stored once, nothing else of ``out`` is
    touched.  Returns ``out``."""
    lib = _capi.load_library()
    s = int(scale)
    if s < 1 or out.dim() < 4 or out.shape[-1] != 3 or out.shape[-3] % s or out.shape[-2] % s or out.numel() == 0:
        raise ValueError(f"out: expected [B,(1,){s}*H,{s}*W,3], got {tuple(out.shape)}")
    H, W = int(out.shape[-3]) // s, int(out.shape[-2]) // s
    B = out.numel() // (s * H * s * W * 3)
    if y.dim() < 4 or y.numel() == 0:
        raise ValueError(f"y: expected [count,(1,)s*th,s*tw,3], got {tuple(y.shape)}")
    t, th, tw, first, count = _tile_run(B, H, W, tile, first, int(y.shape[0]))
    if tuple(y.shape[-3:]) != (s * th, s * tw, 3) or y.numel() != count * s * th * s * tw * 3:
        raise ValueError(f"y must be {count} tile results of ({s * th}, {s * tw}, 3), got {tuple(y.shape)}")
    _capi.check(lib.pfnl_op_tile_scatter(_req(y, "y"), _req(out, "out"), B, H, W, s, C.byref(t), first, count, _stream(out)))
    return out


def blur_decimate(hr, scale: int = 4, out=None):
    """reference utils.py:169-192 (DownSample_4D with BLUR): hr [F,H,W,3] (cuda) -> [F,ceil(H/s),ceil(W/s),3]."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = hr.shape
    if c != 3:
        raise ValueError("blur_decimate expects 3 channels")
    out = _out(out, (F, -(-H // scale), -(-W // scale), 3), torch.float32, hr.device)
    _capi.check(lib.pfnl_op_blur_decimate(_req(hr, "hr"), _req(out, "out"), F, H, W, scale, _stream(hr)))
    return out


def selftest_mfma(device: int = 0) -> None:
    _capi.check(_capi.load_library().pfnl_selftest_mfma(device))


def _hp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def nonlocal_embedded(x, wg, bg, ww, bw, wt, bt, wp, bp):
    """The embedded-Gaussian form (reference utils.py:18-71 with nltype=0: theta = conv(x; wt, bt), phi = conv(x; wp, bp)):
    x [B,T,H,W,3] (cuda) -> [B,H,W,3T] = stack + depth_to_space(NonLocalBlock_0(space_to_depth(stack)))."""
    import torch
    lib = _capi.load_library()
    B, T, H, W, c = x.shape
    C_ = 12 * T
    arrs = [_host(a, "w") for a in (wg, bg, ww, bw, wt, bt, wp, bp)]
    for a, n in zip(arrs, (C_ * C_, C_) * 4):
        if a.size != n:
            raise ValueError("nonlocal_embedded: weight shapes do not match 12*T channels")
    out = torch.empty((B, H, W, 3 * T), dtype=torch.float32, device=x.device)
    _capi.check(lib.pfnl_op_nonlocal_embedded(_req(x, "x"), *[_hp(a) for a in arrs], _req(out, "out"), B, T, H, W, _stream(x)))
    return out


def conv1_conv10_split16(x, k1, b1, k10, b10, frames_per_clip: int, sf0: bool = False, out1=None, base=None):
    """conv1_i + conv10_i of a progressive-fusion block as one launch (reference model/pfnl.py:66-68): x [clips*T,H,W,64] (cuda) ->
    (inp1 [clips*T,H,W,64], base [clips,H,W,64]), both activated; k1 HWIO [3,3,64,64], k10 HWIO [1,1,64T,64].  sf0: the input is
    converted to the split format first and the kernel takes its halo from there by LDS-DMA (bit-identical results)."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = x.shape
    T = int(frames_per_clip)
    k1h, k10h = _host(k1, "k1"), _host(k10, "k10")
    if c != 64 or F % T or k1h.size != 9 * 64 * 64 or k10h.size != 64 * T * 64:
        raise ValueError("conv1_conv10_split16: geometry mismatch")
    out1 = _out(out1, (F, H, W, 64), torch.float32, x.device, "out1")
    base = _out(base, (F // T, H, W, 64), torch.float32, x.device, "base")
    fn = lib.pfnl_op_conv1_conv10_split16_sf0 if sf0 else lib.pfnl_op_conv1_conv10_split16
    _capi.check(fn(_req(x, "x"), _hp(k1h), _hp(_host(b1, "b1")), _hp(k10h), _hp(_host(b10, "b10")),
                                                 _req(out1, "out1"), _req(base, "base"), F // T, T, H, W, _stream(x)))
    return out1, base


def conv2_chain_sf0(x, kernel, bias, base, resid, add_div: int, act: bool = True):
    """The whole of conv2_i in one launch with the split-format copy of its output (reference model/pfnl.py:69-71; option split16_sf0):
    x = inp1 [F,H,W,64], kernel HWIO [3,3,128,64], base [F/add_div,H,W,64], resid [F,H,W,64] (all cuda fp32) ->
    (out [F,H,W,64] fp32, out_sf [F,H,W,128] int16 bit patterns of binary16: per pixel [channel half][hi 32 | lo' 32])."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = x.shape
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    if c != 64 or k.shape != (3, 3, 128, 64) or F % add_div:
        raise ValueError("conv2_chain_sf0: geometry mismatch")
    out = torch.empty((F, H, W, 64), dtype=torch.float32, device=x.device)
    out_sf = torch.empty((F, H, W, 128), dtype=torch.int16, device=x.device)
    _capi.check(lib.pfnl_op_conv2_chain_sf0(_req(x, "x"), _hp(k), _hp(b) if b is not None else None, _req(base, "base"), int(add_div),
                                            _req(resid, "resid"), _req(out, "out"), C.c_void_p(out_sf.data_ptr()), F, H, W, 1 if act else 0, _stream(x)))
    return out, out_sf


def nonlocal_block(x, wg, bg, ww, bw, theta=None, phi=None, nltype: int = 1, sub_sample: int = 1, out=None):
    """utils.NonLocalBlock(input_x, out_channels, sub_sample, nltype) in its general form (reference utils.py:18-71) inside the
    wrapper of model/pfnl.py:55-60: x [B,T,H,W,3] (cuda) -> [B,H,W,3T] = stack + depth_to_space(NonLocalBlock(space_to_depth(stack))).
    ``theta`` / ``phi`` = (kernel [C,C] or [1,1,C,C], bias [C]) of the two projections (nltype 0 and 2)."""
    import torch
    lib = _capi.load_library()
    B, T, H, W, c = x.shape
    C_ = 12 * T
    if nltype not in (0, 1, 2):
        raise ValueError("nltype must be 0, 1 or 2 (3, 'concat', builds no graph in the reference: utils.py:23)")
    if nltype != 1 and (theta is None or phi is None):
        raise ValueError("nltype 0 / 2 need the theta and phi projections")
    arrs = [_host(a, "w") for a in (wg, bg, ww, bw)]
    proj = [None] * 4
    if nltype != 1:
        proj = [_host(a, "w") for a in (theta[0], theta[1], phi[0], phi[1])]
    for a, n in zip(arrs + [p for p in proj if p is not None], (C_ * C_, C_) * 4):
        if a.size != n:
            raise ValueError("nonlocal_block: weight shapes do not match 12*T channels")
    out = _out(out, (B, H, W, 3 * T), torch.float32, x.device)
    _capi.check(lib.pfnl_op_nonlocal_block(_req(x, "x"), *[_hp(a) for a in arrs], *[_hp(a) for a in proj], int(nltype),
                                           int(sub_sample), _req(out, "out"), B, T, H, W, _stream(x)))
    return out


def conv0(x, kernel, bias=None, f32=False, out=None):
    """conv0 (reference model/pfnl.py:48,61-62): x [B,T,H,W,3] (cuda) -> lrelu(conv5x5(frame) + b) [B*T,H,W,64].
    f32: the fp32 VALU kernel of strict_fp32=on instead of the default split-f16 MFMA kernel."""
    import torch
    lib = _capi.load_library()
    B, T, H, W, c = x.shape
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    if k.shape != (5, 5, 3, 64) or c != 3:
        raise ValueError("conv0: geometry mismatch")
    out = _out(out, (B * T, H, W, 64), torch.float32, x.device)
    _capi.check(lib.pfnl_op_conv0_ex(_req(x, "x"), _hp(k), _hp(b), _req(out, "out"), B, T, H, W, 1 if f32 else 0, _stream(x)))
    return out


def conv0_bf16(x, kernel, bias=None, out=None):
    """conv0 as precision=bf16 runs it (pfnl_op_conv0_bf16): the default kernel of `conv0`, its result rounded once to bf16 at the
    store.  x [B,T,H,W,3] float32 (cuda) -> [B*T,H,W,64] bfloat16."""
    import torch
    lib = _capi.load_library()
    B, T, H, W, c = x.shape
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    if k.shape != (5, 5, 3, 64) or c != 3:
        raise ValueError("conv0_bf16: geometry mismatch")
    out = _out(out, (B * T, H, W, 64), torch.bfloat16, x.device)
    _capi.check(lib.pfnl_op_conv0_bf16(_req(x, "x"), _hp(k), _hp(b), _req16(out, "out"), B, T, H, W, _stream(x)))
    return out


def tail(merge, x, kernel, bias, scale: int, out=None):
    """The tail (reference model/pfnl.py:53,63,76-80): merge [B,H,W,48] (cuda), x [B,T,H,W,3] (cuda) -> [B,1,sH,sW,3]."""
    import torch
    lib = _capi.load_library()
    B, T, H, W, c = x.shape
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    if merge.shape != (B, H, W, 48) or k.shape != (3, 3, 12, 12 if scale == 4 else 3):
        raise ValueError("tail: geometry mismatch")
    out = _out(out, (B, 1, scale * H, scale * W, 3), torch.float32, x.device)
    _capi.check(lib.pfnl_op_tail(_req(merge, "merge"), _req(x, "x"), _hp(k), _hp(b), _req(out, "out"), B, T, H, W, scale, _stream(x)))
    return out


def gather_windows(frames, first: int, count: int, num_frames: int, out=None):
    """frames [F,H,W,3] (cuda) -> [count,T,H,W,3]: the clamped sliding windows of frames first..first+count-1
    (reference model/pfnl.py:238-242)."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = frames.shape
    if c != 3:
        raise ValueError("gather_windows expects [F,H,W,3]")
    out = _out(out, (count, num_frames, H, W, 3), torch.float32, frames.device)
    _capi.check(lib.pfnl_op_gather_windows(_req(frames, "frames"), _req(out, "out"), F, first, count, num_frames, H, W, _stream(frames)))
    return out


def gather_windows_u8(ring, last: int, first: int, count: int, num_frames: int, out=None):
    """ring [cap,H,W,3] uint8 (cuda), frame f in slot f % cap -> [count,T,H,W,3] float32: the clamped sliding windows of frames
    first..first+count-1 of a sequence whose newest frame is ``last``, dequantised as the harness does, (u8 / 255.).astype(np.float32)
    (pfnl_op_gather_windows_u8: the streaming session's input side; reference model/pfnl.py:238-242, :287)."""
    import torch
    lib = _capi.load_library()
    if not (isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dtype == torch.uint8 and ring.is_contiguous()):
        raise TypeError("ring must be a contiguous uint8 tensor on the GPU")
    cap, H, W, c = ring.shape
    if c != 3:
        raise ValueError("gather_windows_u8 expects [cap,H,W,3]")
    out = _out(out, (count, num_frames, H, W, 3), torch.float32, ring.device)
    _capi.check(lib.pfnl_op_gather_windows_u8(C.c_void_p(ring.data_ptr()), _req(out, "out"), cap, int(last), int(first), count, num_frames,
                                              H, W, _stream(ring)))
    return out


def gather_windows_u8_scenes(ring, scene_first, last: int, first: int, count: int, num_frames: int):
    """gather_windows_u8 with the windows kept inside the centre's scene: scene_first [cap] int64 (cuda), slot f % cap = the first frame
    of frame f's scene (pfnl_op_gather_windows_u8_scenes; the rule: pfnl_amd/scene.py scene_windows_index)."""
    import torch
    lib = _capi.load_library()
    if not (isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dtype == torch.uint8 and ring.is_contiguous()):
        raise TypeError("ring must be a contiguous uint8 tensor on the GPU")
    cap, H, W, c = ring.shape
    if c != 3:
        raise ValueError("gather_windows_u8_scenes expects [cap,H,W,3]")
    if not (isinstance(scene_first, torch.Tensor) and scene_first.device == ring.device and scene_first.dtype == torch.int64
            and scene_first.is_contiguous() and tuple(scene_first.shape) == (cap,)):
        raise TypeError("scene_first must be a contiguous int64 tensor [cap] on the ring's device")
    out = torch.empty((count, num_frames, H, W, 3), dtype=torch.float32, device=ring.device)
    _capi.check(lib.pfnl_op_gather_windows_u8_scenes(C.c_void_p(ring.data_ptr()), C.c_void_p(scene_first.data_ptr()), _req(out, "out"), cap,
                                                     int(last), int(first), count, num_frames, H, W, _stream(ring)))
    return out


def scene_sad_u8(a, b) -> int:
    """sum |Y(a) - Y(b)| of two [H,W,3] uint8 frames (cuda), Y = (66 R + 129 G + 25 B + 128) >> 8, as a Python int: the streaming session's
    scene score (pfnl_op_scene_sad_u8; exact: pfnl_amd/scene.py frame_sad).  Synchronises."""
    import torch
    lib = _capi.load_library()
    for t, name in ((a, "a"), (b, "b")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous uint8 tensor on the GPU")
    if a.dim() != 3 or a.shape[2] != 3 or b.shape != a.shape or b.device != a.device:
        raise ValueError("scene_sad_u8 expects two [H,W,3] frames on one device")
    out = torch.zeros((1,), dtype=torch.int64, device=a.device)
    _capi.check(lib.pfnl_op_scene_sad_u8(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.shape[0], a.shape[1],
                                         C.c_void_p(out.data_ptr()), _stream(a)))
    return int(out.item())


def _req_u8(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous uint8 tensor on the GPU")
    return C.c_void_p(t.data_ptr())


def _yuv_ids(fmt, matrix, full_range):
    if fmt not in ("nv12", "i420"):
        raise ValueError(f'fmt: "nv12" or "i420", got {fmt!r}')
    if matrix not in _capi.YUV_MATRICES:
        raise ValueError(f"matrix: one of {sorted(_capi.YUV_MATRICES)}, got {matrix!r}")
    return _capi.PIXEL_FORMATS[fmt], _capi.YUV_MATRICES[matrix], int(bool(full_range))


def _siting_id(siting):
    if siting not in _capi.CHROMA_SITINGS:
        raise ValueError(f"siting: one of {sorted(_capi.CHROMA_SITINGS)}, got {siting!r}")
    return _capi.CHROMA_SITINGS[siting]


def yuv420_to_rgb(frames, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, out=None, siting="left"):
    """n tightly packed NV12 / I420 frames, a uint8 tensor (cuda) of n * H*W*3/2 elements in any shape -> [n,H,W,3] uint8, byte for byte
    pfnl_amd/yuv.py to_rgb (pfnl_op_yuv420_to_rgb_u8_sited: the streaming session's input edge).  Any alignment; ``out``: write there;
    ``siting``: "left" | "center" | "topleft"."""
    import torch
    lib = _capi.load_library()
    ids = _yuv_ids(fmt, matrix, full_range)
    sid = _siting_id(siting)
    src = _req_u8(frames, "frames")
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"H and W must be even and at least 2, got {H} x {W}")
    fb = H * W * 3 // 2
    n = frames.numel() // fb
    if n < 1 or n * fb != frames.numel():
        raise ValueError(f"frames must hold a whole number of {fb}-byte frames, got {frames.numel()} bytes")
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=frames.device)
    elif out.numel() != n * H * W * 3 or out.device != frames.device:
        raise ValueError("out must hold n * H * W * 3 bytes on the frames' device")
    _capi.check(lib.pfnl_op_yuv420_to_rgb_u8_sited(src, ids[0], ids[1], ids[2], n, H, W, _req_u8(out, "out"), sid, _stream(frames)))
    return out.view(n, H, W, 3)


def yuv420_to_rgb_surface(planes, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, out=None, siting="left"):
    """One NV12 / I420 frame given as its planes - uint8 tensors (cuda), each a strided view with a row pitch of its own, as
    pfnl_amd/surface.py describes them: typically ``surface[:H, :W]`` of a decoder's pitched allocation -> [H,W,3] uint8, byte for byte
    pfnl_amd/yuv.py to_rgb of the packed frame (pfnl_op_yuv420_to_rgb_u8_surface: the kernel a device push_planes runs).  Any pointer and
    any pitch; ``out``: write there; ``siting`` as for yuv420_to_rgb."""
    import torch
    from . import surface as _surface
    lib = _capi.load_library()
    ids = _yuv_ids(fmt, matrix, full_range)
    sid = _siting_id(siting)
    planes = tuple(planes)
    for k, p in enumerate(planes):
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.device == planes[0].device):
            raise TypeError(f"plane {k} must be a tensor on the GPU, all on one device")
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"H and W must be even and at least 2, got {H} x {W}")
    sf = _surface.as_struct(planes, fmt, H, W)
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=planes[0].device)
    elif out.numel() != H * W * 3 or out.device != planes[0].device:
        raise ValueError("out must hold H * W * 3 bytes on the planes' device")
    _capi.check(lib.pfnl_op_yuv420_to_rgb_u8_surface_sited(C.byref(sf), ids[0], ids[1], ids[2], H, W, _req_u8(out, "out"), sid,
                                                           _stream(planes[0])))
    return out.view(H, W, 3)


def rgb_to_yuv420(frames, fmt: str, matrix: str = "bt709", full_range=False, out=None, siting="left"):
    """[n,H,W,3] (or [H,W,3]) uint8 (cuda) -> [n, H*3/2, W] uint8: tightly packed NV12 / I420 frames, byte for byte pfnl_amd/yuv.py from_rgb
    (pfnl_op_rgb_to_yuv420_u8_sited: the streaming session's output edge).  H, W even; any alignment; ``out``: write there; ``siting``:
    "left" | "center" | "topleft"."""
    import torch
    lib = _capi.load_library()
    ids = _yuv_ids(fmt, matrix, full_range)
    sid = _siting_id(siting)
    src = _req_u8(frames, "frames")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("rgb_to_yuv420 expects [n,H,W,3]")
    n, H, W, _ = frames.shape
    if n < 1 or H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"n >= 1, H and W even and at least 2, got {n} x {H} x {W}")
    if out is None:
        out = torch.empty((n, H * 3 // 2, W), dtype=torch.uint8, device=frames.device)
    elif out.numel() != n * H * W * 3 // 2 or out.device != frames.device:
        raise ValueError("out must hold n * H * W * 3 / 2 bytes on the frames' device")
    _capi.check(lib.pfnl_op_rgb_to_yuv420_u8_sited(src, ids[0], ids[1], ids[2], n, H, W, _req_u8(out, "out"), sid, _stream(frames)))
    return out.view(n, H * 3 // 2, W)


def resize_u8(frames, out_size, out=None):
    """[n,H,W,3] (or [H,W,3]) uint8 (cuda) -> [n,oH,oW,3] uint8, ``out_size`` = (oH, oW): byte for byte pfnl_amd/resize.py resize
    (pfnl_op_resize_u8: the streaming session's resampler).  Each axis between a quarter and twice its input; any alignment; ``out``:
    write there."""
    import torch
    from . import resize as _resize
    lib = _capi.load_library()
    src = _req_u8(frames, "frames")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError("resize_u8 expects [n,H,W,3]")
    n, H, W, _ = frames.shape
    oH, oW = (int(v) for v in out_size)
    _resize.check_limits(H, oH)
    _resize.check_limits(W, oW)
    if out is None:
        out = torch.empty((n, oH, oW, 3), dtype=torch.uint8, device=frames.device)
    elif out.numel() != n * oH * oW * 3 or out.device != frames.device:
        raise ValueError("out must hold n * oH * oW * 3 bytes on the frames' device")
    _capi.check(lib.pfnl_op_resize_u8(src, n, H, W, oH, oW, _req_u8(out, "out"), _stream(frames)))
    return out.view(n, oH, oW, 3)


def quantise_u8(sr, out=None):
    """uint8(np.round(np.clip(sr * 255, 0, 255))) on the device (reference model/pfnl.py:254-257)."""
    import torch
    lib = _capi.load_library()
    _req(sr, "sr")
    out = _out(out, sr.shape, torch.uint8, sr.device)
    _capi.check(lib.pfnl_op_quantise_u8(C.c_void_p(sr.data_ptr()), C.c_void_p(out.data_ptr()), sr.numel(), _stream(sr)))
    return out


def _req_u16(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint16 and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous uint16 tensor on the GPU")
    return C.c_void_p(t.data_ptr())


def quantise_u10(sr, out=None):
    """uint16(np.round(np.clip(sr * 1023, 0, 1023))) on the device, the product in float32 (pfnl_op_quantise_u10; sample for sample
    pfnl_amd/depth10.py quantise10; NaN gives 0).  sr.numel() a multiple of 4."""
    import torch
    lib = _capi.load_library()
    _req(sr, "sr")
    out = _out(out, sr.shape, torch.uint16, sr.device)
    _capi.check(lib.pfnl_op_quantise_u10(C.c_void_p(sr.data_ptr()), C.c_void_p(out.data_ptr()), sr.numel(), _stream(sr)))
    return out


def quantise_colour(x, src: str, dst: str, bits: int = 8, out=None):
    """[..., 3] float32 (cuda) -> the levels of quantise_u8 / quantise_u10 taken from the primaries ``src`` to ``dst``, uint8 or uint16 of
    the same shape: sample for sample pfnl_amd/colour.py ``convert(quantise(x), src, dst, bits)`` (pfnl_op_quantise_colour_u8 / _u10: stage
    0 of a session whose two sides differ in primaries).  A pixel count that is a multiple of 4; ``src == dst`` is the plain quantise."""
    import torch
    from . import colour as _colour
    lib = _capi.load_library()
    ids = _colour.primaries_id(src), _colour.primaries_id(dst)
    if isinstance(bits, bool) or bits not in (8, 10):
        raise ValueError(f"bits: 8 or 10, got {bits!r}")
    _req(x, "x")
    if x.dim() < 1 or x.shape[-1] != 3:
        raise ValueError("quantise_colour expects [..., 3]")
    out = _out(out, x.shape, torch.uint8 if bits == 8 else torch.uint16, x.device)
    hook = lib.pfnl_op_quantise_colour_u8 if bits == 8 else lib.pfnl_op_quantise_colour_u10
    _capi.check(hook(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.numel() // 3, ids[0], ids[1], _stream(x)))
    return out


def rgb_to_yuv420_u10(frames, fmt: str, matrix: str = "bt709", full_range=False, out=None, siting="left"):
    """[n,H,W,3] (or [H,W,3]) uint16 (cuda) with values 0 .. 1023 -> [n, H*3/2, W] uint16: tightly packed P010 / I010 frames, sample for
    sample pfnl_amd/depth10.py from_rgb10 (pfnl_op_rgb_to_yuv420_u10: the streaming session's 10-bit output edge).  H, W even; any
    alignment; ``out``: write there; ``siting`` as for rgb_to_yuv420."""
    import torch
    lib = _capi.load_library()
    sid = _siting_id(siting)
    if fmt not in ("p010", "i010"):
        raise ValueError(f'fmt: "p010" or "i010", got {fmt!r}')
    if matrix not in _capi.YUV_MATRICES:
        raise ValueError(f"matrix: one of {sorted(_capi.YUV_MATRICES)}, got {matrix!r}")
    src = _req_u16(frames, "frames")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("rgb_to_yuv420_u10 expects [n,H,W,3]")
    n, H, W, _ = frames.shape
    if n < 1 or H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"n >= 1, H and W even and at least 2, got {n} x {H} x {W}")
    if out is None:
        out = torch.empty((n, H * 3 // 2, W), dtype=torch.uint16, device=frames.device)
    elif out.numel() != n * H * W * 3 // 2 or out.device != frames.device:
        raise ValueError("out must hold n * H * W * 3 / 2 samples on the frames' device")
    _capi.check(lib.pfnl_op_rgb_to_yuv420_u10_sited(src, _capi.PIXEL_FORMATS[fmt], _capi.YUV_MATRICES[matrix], int(bool(full_range)), n, H, W,
                                                    _req_u16(out, "out"), sid, _stream(frames)))
    return out.view(n, H * 3 // 2, W)


def _yuv10_ids(fmt, matrix, full_range):
    if fmt not in ("p010", "i010"):
        raise ValueError(f'fmt: "p010" or "i010", got {fmt!r}')
    if matrix not in _capi.YUV_MATRICES:
        raise ValueError(f"matrix: one of {sorted(_capi.YUV_MATRICES)}, got {matrix!r}")
    return _capi.PIXEL_FORMATS[fmt], _capi.YUV_MATRICES[matrix], int(bool(full_range))


def yuv420_to_rgb10(frames, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, out=None, siting="left"):
    """n tightly packed P010 / I010 frames, a uint16 tensor (cuda) of n * H*W*3/2 samples in any shape -> [n,H,W,3] uint16 with values
    0 .. 1023, sample for sample pfnl_amd/depth10.py to_rgb10 (pfnl_op_yuv420_to_rgb_u10_sited: the streaming session's input edge at an
    input depth of 10).  P010's low six bits are ignored, an I010 sample above 1023 counts as 1023.  Any alignment of whole samples;
    ``out``: write there; ``siting``: "left" | "center" | "topleft"."""
    import torch
    lib = _capi.load_library()
    ids = _yuv10_ids(fmt, matrix, full_range)
    sid = _siting_id(siting)
    src = _req_u16(frames, "frames")
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"H and W must be even and at least 2, got {H} x {W}")
    fs = H * W * 3 // 2
    n = frames.numel() // fs
    if n < 1 or n * fs != frames.numel():
        raise ValueError(f"frames must hold a whole number of frames of {fs} samples, got {frames.numel()} samples")
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint16, device=frames.device)
    elif out.numel() != n * H * W * 3 or out.device != frames.device:
        raise ValueError("out must hold n * H * W * 3 samples on the frames' device")
    _capi.check(lib.pfnl_op_yuv420_to_rgb_u10_sited(src, ids[0], ids[1], ids[2], n, H, W, _req_u16(out, "out"), sid, _stream(frames)))
    return out.view(n, H, W, 3)


def yuv420_to_rgb10_surface(planes, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, out=None, siting="left"):
    """One P010 / I010 frame given as its planes - uint16 tensors (cuda), each a strided view with a row pitch of its own
    (pfnl_amd/surface.py) -> [H,W,3] uint16, sample for sample pfnl_amd/depth10.py to_rgb10 of the packed frame
    (pfnl_op_yuv420_to_rgb_u10_surface_sited: the kernel a device push_planes runs at an input depth of 10).  Even pointers and pitches."""
    import torch
    from . import surface as _surface
    lib = _capi.load_library()
    ids = _yuv10_ids(fmt, matrix, full_range)
    sid = _siting_id(siting)
    planes = tuple(planes)
    for k, p in enumerate(planes):
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.device == planes[0].device):
            raise TypeError(f"plane {k} must be a tensor on the GPU, all on one device")
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"H and W must be even and at least 2, got {H} x {W}")
    sf = _surface.as_struct(planes, fmt, H, W)
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint16, device=planes[0].device)
    elif out.numel() != H * W * 3 or out.device != planes[0].device:
        raise ValueError("out must hold H * W * 3 samples on the planes' device")
    _capi.check(lib.pfnl_op_yuv420_to_rgb_u10_surface_sited(C.byref(sf), ids[0], ids[1], ids[2], H, W, _req_u16(out, "out"), sid,
                                                            _stream(planes[0])))
    return out.view(H, W, 3)


# ---- 4:2:2 and 4:4:4 (include/pfnl_hip.h CHROMA FORMAT): the conversions with the subsampling named ------------------------------------------
def _chroma_id(chroma):
    if chroma not in _capi.CHROMA_FORMATS:
        raise ValueError(f"chroma: one of {sorted(_capi.CHROMA_FORMATS)}, got {chroma!r}")
    return _capi.CHROMA_FORMATS[chroma]


def _yuv_to_rgb(frames, ids, H, W, chroma, siting, out, req, dtype, hook):
    import torch
    from . import yuv as _yuv
    cid, sid = _chroma_id(chroma), _siting_id(siting)
    src = req(frames, "frames")
    _yuv.check_size(H, W, chroma)
    fs = _yuv.frame_bytes(H, W, chroma)
    n = frames.numel() // fs
    if n < 1 or n * fs != frames.numel():
        raise ValueError(f"frames must hold a whole number of frames of {fs} samples, got {frames.numel()} samples")
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=dtype, device=frames.device)
    elif out.numel() != n * H * W * 3 or out.device != frames.device:
        raise ValueError("out must hold n * H * W * 3 samples on the frames' device")
    _capi.check(hook(src, ids[0], ids[1], ids[2], n, H, W, req(out, "out"), cid, sid, _stream(frames)))
    return out.view(n, H, W, 3)


def yuv_to_rgb(frames, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, chroma="420", siting="left", out=None):
    """yuv420_to_rgb with the subsampling named: n tightly packed frames in the layout ``fmt`` ("nv12" | "i420") at ``chroma`` "420" |
    "422" (NV16 / I422, 2 H W bytes a frame, W even) | "444" (NV24 / I444, 3 H W bytes, any H and W) -> [n,H,W,3] uint8, byte for byte
    pfnl_amd/yuv.py to_rgb(..., chroma=) (pfnl_op_yuv_to_rgb_u8_chroma).  Any alignment; ``out``: write there."""
    import torch
    lib = _capi.load_library()
    return _yuv_to_rgb(frames, _yuv_ids(fmt, matrix, full_range), H, W, chroma, siting, out, _req_u8, torch.uint8, lib.pfnl_op_yuv_to_rgb_u8_chroma)


def yuv_to_rgb_u10(frames, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, chroma="420", siting="left", out=None):
    """yuv_to_rgb on uint16 samples: ``fmt`` "p010" (P210 / P410 at 4:2:2 / 4:4:4; the low six bits ignored) | "i010" (yuv422p10le /
    yuv444p10le; above 1023 = 1023) -> [n,H,W,3] uint16 in 0 .. 1023, sample for sample pfnl_amd/depth10.py to_rgb10(..., chroma=)
    (pfnl_op_yuv_to_rgb_u10_chroma)."""
    import torch
    lib = _capi.load_library()
    return _yuv_to_rgb(frames, _yuv10_ids(fmt, matrix, full_range), H, W, chroma, siting, out, _req_u16, torch.uint16,
                       lib.pfnl_op_yuv_to_rgb_u10_chroma)


def _yuv_to_rgb_surface(planes, fmt, ids, H, W, chroma, siting, out, req, dtype, hook):
    import torch
    from . import surface as _surface
    cid, sid = _chroma_id(chroma), _siting_id(siting)
    planes = tuple(planes)
    for k, p in enumerate(planes):
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.device == planes[0].device):
            raise TypeError(f"plane {k} must be a tensor on the GPU, all on one device")
    sf = _surface.as_struct(planes, fmt, H, W, chroma)
    if out is None:
        out = torch.empty((H, W, 3), dtype=dtype, device=planes[0].device)
    elif out.numel() != H * W * 3 or out.device != planes[0].device:
        raise ValueError("out must hold H * W * 3 samples on the planes' device")
    _capi.check(hook(C.byref(sf), ids[0], ids[1], ids[2], H, W, req(out, "out"), cid, sid, _stream(planes[0])))
    return out.view(H, W, 3)


def yuv_to_rgb_surface(planes, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, chroma="420", siting="left", out=None):
    """yuv420_to_rgb_surface with the subsampling named: one frame as its planes (pfnl_amd/surface.py plane_shapes(..., chroma)), each a
    strided uint8 view with a pitch of its own -> [H,W,3] uint8, byte for byte yuv_to_rgb of the packed frame
    (pfnl_op_yuv_to_rgb_u8_surface_chroma)."""
    import torch
    lib = _capi.load_library()
    return _yuv_to_rgb_surface(planes, fmt, _yuv_ids(fmt, matrix, full_range), H, W, chroma, siting, out, _req_u8, torch.uint8,
                               lib.pfnl_op_yuv_to_rgb_u8_surface_chroma)


def yuv_to_rgb_surface_u10(planes, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, chroma="420", siting="left", out=None):
    """yuv_to_rgb_surface on uint16 planes ("p010" | "i010"; even pointers and pitches) -> [H,W,3] uint16
    (pfnl_op_yuv_to_rgb_u10_surface_chroma)."""
    import torch
    lib = _capi.load_library()
    return _yuv_to_rgb_surface(planes, fmt, _yuv10_ids(fmt, matrix, full_range), H, W, chroma, siting, out, _req_u16, torch.uint16,
                               lib.pfnl_op_yuv_to_rgb_u10_surface_chroma)


def _rgb_to_yuv(frames, ids, chroma, siting, out, req, dtype, hook):
    import torch
    from . import yuv as _yuv
    cid, sid = _chroma_id(chroma), _siting_id(siting)
    src = req(frames, "frames")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError("expected [n,H,W,3]")
    n, H, W, _ = frames.shape
    _yuv.check_size(H, W, chroma)
    rows = _yuv.frame_bytes(H, W, chroma) // W
    if out is None:
        out = torch.empty((n, rows, W), dtype=dtype, device=frames.device)
    elif out.numel() != n * rows * W or out.device != frames.device:
        raise ValueError(f"out must hold n * {rows} * W samples on the frames' device")
    _capi.check(hook(src, ids[0], ids[1], ids[2], n, H, W, req(out, "out"), cid, sid, _stream(frames)))
    return out.view(n, rows, W)


def rgb_to_yuv(frames, fmt: str, matrix: str = "bt709", full_range=False, chroma="420", siting="left", out=None):
    """rgb_to_yuv420 with the subsampling named: [n,H,W,3] (or [H,W,3]) uint8 -> [n, H*3/2 | 2H | 3H, W] uint8, tightly packed frames in
    the layout ``fmt`` at ``chroma``, byte for byte pfnl_amd/yuv.py from_rgb(..., chroma=) (pfnl_op_rgb_to_yuv_u8_chroma).  Any
    alignment; ``out``: write there."""
    import torch
    lib = _capi.load_library()
    return _rgb_to_yuv(frames, _yuv_ids(fmt, matrix, full_range), chroma, siting, out, _req_u8, torch.uint8, lib.pfnl_op_rgb_to_yuv_u8_chroma)


def rgb_to_yuv_u10(frames, fmt: str, matrix: str = "bt709", full_range=False, chroma="420", siting="left", out=None):
    """rgb_to_yuv on uint16 samples with values 0 .. 1023 -> "p010" (every value << 6) | "i010" at ``chroma``, sample for sample
    pfnl_amd/depth10.py from_rgb10(..., chroma=) (pfnl_op_rgb_to_yuv_u10_chroma)."""
    import torch
    lib = _capi.load_library()
    return _rgb_to_yuv(frames, _yuv10_ids(fmt, matrix, full_range), chroma, siting, out, _req_u16, torch.uint16,
                       lib.pfnl_op_rgb_to_yuv_u10_chroma)


# ---- packed formats (include/pfnl_hip.h PACKED FORMATS; the rule: pfnl_amd/packed.py) ------------------------------------------------------
def _packed_args(name, matrix, full_range, siting, H, W, pitch):
    from . import packed as _packed
    _packed.check(name, H, W)
    if matrix not in _capi.YUV_MATRICES:
        raise ValueError(f"matrix: one of {sorted(_capi.YUV_MATRICES)}, got {matrix!r}")
    pitch = _packed.tight_row_bytes(name, W) if pitch is None else int(pitch)
    if pitch < _packed.row_bytes(name, W):
        raise ValueError(f"pitch {pitch} is below the {_packed.row_bytes(name, W)} bytes of a row")
    ten = _packed.bits(name) == 10
    return _capi.PACKINGS[name], _capi.YUV_MATRICES[matrix], 1 if full_range else 0, _siting_id(siting), pitch, ten


def packed_to_rgb(frames, name: str, H: int, W: int, matrix: str = "bt709", full_range=False, siting="left", pitch=None, out=None):
    """n frames in the packing ``name`` (pfnl_amd/packed.py PACKINGS) -> [n,H,W,3], uint8 for an 8-bit packing and uint16 in 0 .. 1023 for a
    10-bit one: the depth follows the packing, byte for byte packed.to_rgb (pfnl_op_packed_to_rgb_u8 / _u10).  ``frames``: a contiguous
    uint8 tensor on the GPU of n * H * pitch bytes, rows ``pitch`` bytes apart (default: the tight frame's, packed.tight_row_bytes); its
    address may be any the packing allows (y210: even, x2rgb10 / x2bgr10 / v210: a multiple of 4).  ``out``: write there."""
    import torch
    lib = _capi.load_library()
    pid, mid, fr, sid, pitch, ten = _packed_args(name, matrix, full_range, siting, H, W, pitch)
    src = _req_u8(frames, "frames")
    n = frames.numel() // (H * pitch)
    if n < 1 or n * H * pitch != frames.numel():
        raise ValueError(f"frames must hold a whole number of frames of {H} rows of {pitch} bytes, got {frames.numel()} bytes")
    dtype = torch.uint16 if ten else torch.uint8
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=dtype, device=frames.device)
    elif out.numel() != n * H * W * 3 or out.device != frames.device:
        raise ValueError("out must hold n * H * W * 3 samples on the frames' device")
    hook = lib.pfnl_op_packed_to_rgb_u10 if ten else lib.pfnl_op_packed_to_rgb_u8
    _capi.check(hook(src, pitch, pid, mid, fr, sid, n, H * pitch, H, W, (_req_u16 if ten else _req_u8)(out, "out"), _stream(frames)))
    return out.view(n, H, W, 3)


def rgb_to_packed(frames, name: str, matrix: str = "bt709", full_range=False, siting="left", pitch=None, out=None):
    """[n,H,W,3] (or [H,W,3]) - uint8 for an 8-bit packing, uint16 with values 0 .. 1023 for a 10-bit one - -> [n, H, pitch] uint8: n frames
    in the packing ``name``, rows ``pitch`` bytes apart (default: the tight frame's), byte for byte packed.from_rgb (pfnl_op_rgb_to_packed_u8
    / _u10).  Bytes between a row's end and the pitch are never written: a fresh result holds 0 there (a tight v210 frame's padding), ``out``
    keeps what it held."""
    import torch
    lib = _capi.load_library()
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError("expected [n,H,W,3]")
    n, H, W, _ = frames.shape
    pid, mid, fr, sid, pitch, ten = _packed_args(name, matrix, full_range, siting, H, W, pitch)
    src = (_req_u16 if ten else _req_u8)(frames, "frames")
    if out is None:
        out = torch.zeros((n, H, pitch), dtype=torch.uint8, device=frames.device)
    elif out.numel() != n * H * pitch or out.device != frames.device:
        raise ValueError(f"out must hold n * H * {pitch} bytes on the frames' device")
    hook = lib.pfnl_op_rgb_to_packed_u10 if ten else lib.pfnl_op_rgb_to_packed_u8
    _capi.check(hook(_req_u8(out, "out"), pitch, pid, mid, fr, sid, n, H * pitch, H, W, src, _stream(frames)))
    return out.view(n, H, pitch)


# ---- interlaced input (include/pfnl_hip.h INTERLACED; the rule: pfnl_amd/deinterlace.py) ---------------------------------------------------
DEINTERLACE_STRIP_ROWS = 4                                  # csrc/field_geom.h DEINT_STRIP_ROWS: the rows of the progressive frame a lane walks down


def _deinterlace(fields, parity, out, req, dtype, hook):
    names = ("p2", "p1", "cur", "n1", "n2")
    ptrs = [req(f, n) for f, n in zip(fields, names)]
    cur = fields[2]
    if cur.dim() != 3 or cur.shape[2] != 3 or any(tuple(f.shape) != tuple(cur.shape) or f.device != cur.device for f in fields):
        raise ValueError("the five fields are [H/2, W, 3] tensors of one shape on one device")
    if parity not in (0, 1):
        raise ValueError(f"parity: 0 or 1, got {parity!r}")
    h, W, _ = cur.shape
    out = _out(out, (2 * h, W, 3), dtype, cur.device)
    _capi.check(hook(*ptrs, 2 * h, W, int(parity), req(out, "out"), _stream(cur)))
    return out


def deinterlace(p2, p1, cur, n1, n2, parity, out=None):
    """Five decoded fields, contiguous uint8 [H/2,W,3] tensors on the GPU (they may be one another, and start at any address), ``cur`` of
    parity ``parity`` -> the progressive frame [H,W,3] at cur's time, byte for byte pfnl_amd/deinterlace.py interpolate
    (pfnl_op_deinterlace_u8: the kernel ahead of the streaming session's ring).  ``out``: write there."""
    import torch
    return _deinterlace((p2, p1, cur, n1, n2), parity, out, _req_u8, torch.uint8, _capi.load_library().pfnl_op_deinterlace_u8)


def deinterlace_pair(fields, parity, out=None):
    """Six consecutive fields k - 2 .. k + 3, [H/2,W,3] uint8 (or all uint16: min(v, 1023)) tensors on the GPU, field k = ``fields[2]`` of
    parity ``parity`` -> [2,H,W,3]: the progressive frames at the times of fields k and k + 1, made by ONE launch
    (pfnl_op_deinterlace_pair_u8 / _u10: what a field-rate session issues per push)."""
    import torch
    fields = list(fields)
    if len(fields) != 6:
        raise ValueError("six consecutive fields")
    ten = fields[2].dtype == torch.uint16
    req = _req_u16 if ten else _req_u8
    ptrs = (C.c_void_p * 6)(*(req(f, f"fields[{k}]") for k, f in enumerate(fields)))
    cur = fields[2]
    if cur.dim() != 3 or cur.shape[2] != 3 or any(tuple(f.shape) != tuple(cur.shape) or f.device != cur.device for f in fields):
        raise ValueError("the six fields are [H/2, W, 3] tensors of one shape on one device")
    if parity not in (0, 1):
        raise ValueError(f"parity: 0 or 1, got {parity!r}")
    h, W, _ = cur.shape
    out = _out(out, (2, 2 * h, W, 3), cur.dtype, cur.device)
    lib = _capi.load_library()
    _capi.check((lib.pfnl_op_deinterlace_pair_u10 if ten else lib.pfnl_op_deinterlace_pair_u8)(ptrs, 2 * h, W, int(parity), req(out, "out"), _stream(cur)))
    return out


def deinterlace_u10(p2, p1, cur, n1, n2, parity, out=None):
    """``deinterlace`` on uint16 fields, every sample taken as min(v, 1023) (pfnl_op_deinterlace_u10; interpolate with maxv = 1023)."""
    import torch
    return _deinterlace((p2, p1, cur, n1, n2), parity, out, _req_u16, torch.uint16, _capi.load_library().pfnl_op_deinterlace_u10)


# ---- inverse telecine (include/pfnl_hip.h TELECINE; the rule: pfnl_amd/telecine.py) --------------------------------------------------------
def _telecine_fields(A, Xc, Xp, parity):
    import torch
    ten = A.dtype == torch.uint16
    req = _req_u16 if ten else _req_u8
    ptrs = [req(f, n) for f, n in zip((A, Xc, Xp), ("A", "Xc", "Xp"))]
    if A.dim() != 3 or A.shape[2] != 3 or any(tuple(f.shape) != tuple(A.shape) or f.device != A.device for f in (Xc, Xp)):
        raise ValueError("the three fields are [H/2, W, 3] tensors of one shape on one device")
    if parity not in (0, 1):
        raise ValueError(f"parity: 0 or 1, got {parity!r}")
    return ten, req, ptrs


def fieldmatch(A, Xc, Xp, parity, threshold=10):
    """The kept field ``A`` of parity ``parity`` and its two candidate partners, contiguous [H/2,W,3] uint8 (or all uint16: min(v, 1023))
    tensors on the GPU at any address -> (count of c, count of p): pfnl_amd/telecine.py comb_count of each, exactly
    (pfnl_op_fieldmatch_u8 / _u10: the match launch of the streaming session's inverse telecine)."""
    import torch
    ten, _, ptrs = _telecine_fields(A, Xc, Xp, parity)
    h, W, _ = A.shape
    counts = torch.zeros(2, dtype=torch.int64, device=A.device)
    lib = _capi.load_library()
    _capi.check((lib.pfnl_op_fieldmatch_u10 if ten else lib.pfnl_op_fieldmatch_u8)(*ptrs, h, W, int(parity), int(threshold),
                                                                                  C.c_void_p(counts.data_ptr()), _stream(A)))
    return tuple(int(v) for v in counts.cpu())


def telecine_frame(A, Xc, Xp, parity, threshold=None, post=False, comb_limit=None, out=None):
    """Counts, decision and weave of one pushed frame (pfnl_op_telecine_frame_u8 / _u10) -> (the matched frame [H,W,3], {"count_c",
    "count_p", "match": 0 (c) | 1 (p), "post": 0 | 1}).  With ``post`` the caller passes the deinterlaced frame as ``out``: a flagged frame
    leaves it as it is.  ``threshold`` / ``comb_limit`` None: the defaults of pfnl_amd/telecine.py."""
    import torch
    ten, req, ptrs = _telecine_fields(A, Xc, Xp, parity)
    h, W, _ = A.shape
    if post and out is None:
        raise ValueError("with post the deinterlaced frame is passed as out")
    out = _out(out, (2 * h, W, 3), A.dtype, A.device)
    par = _capi.pfnl_telecine_params(10 if threshold is None else int(threshold), int(bool(post)), -1 if comb_limit is None else int(comb_limit))
    decision = torch.zeros(6, dtype=torch.int64, device=A.device)   # (the last two: the launches' scratch)
    lib = _capi.load_library()
    _capi.check((lib.pfnl_op_telecine_frame_u10 if ten else lib.pfnl_op_telecine_frame_u8)(*ptrs, h, W, int(parity), C.byref(par), req(out, "out"),
                                                                                          C.c_void_p(decision.data_ptr()), _stream(A)))
    d = [int(v) for v in decision.cpu()]
    assert d[4] == d[5] == 0
    return out, {"count_c": d[0], "count_p": d[1], "match": d[2], "post": d[3]}


def _ring_u10(ring, name):
    _req_u16(ring, "ring")
    if ring.dim() != 4 or ring.shape[3] != 3:
        raise ValueError(f"{name} expects [cap,H,W,3]")
    return ring.shape[:3]


def gather_windows_u10(ring, last: int, first: int, count: int, num_frames: int, out=None):
    """gather_windows_u8 on a ring [cap,H,W,3] uint16 (cuda) at 10 bits: the windows dequantised as pfnl_amd/depth10.py dequantise10 does,
    (min(u10, 1023) / 1023.).astype(np.float32) (pfnl_op_gather_windows_u10)."""
    import torch
    lib = _capi.load_library()
    cap, H, W = _ring_u10(ring, "gather_windows_u10")
    out = _out(out, (count, num_frames, H, W, 3), torch.float32, ring.device)
    _capi.check(lib.pfnl_op_gather_windows_u10(C.c_void_p(ring.data_ptr()), _req(out, "out"), cap, int(last), int(first), count, num_frames,
                                               H, W, _stream(ring)))
    return out


def gather_windows_u10_scenes(ring, scene_first, last: int, first: int, count: int, num_frames: int):
    """gather_windows_u8_scenes on a ring [cap,H,W,3] uint16 (cuda) at 10 bits (pfnl_op_gather_windows_u10_scenes)."""
    import torch
    lib = _capi.load_library()
    cap, H, W = _ring_u10(ring, "gather_windows_u10_scenes")
    if not (isinstance(scene_first, torch.Tensor) and scene_first.device == ring.device and scene_first.dtype == torch.int64
            and scene_first.is_contiguous() and tuple(scene_first.shape) == (cap,)):
        raise TypeError("scene_first must be a contiguous int64 tensor [cap] on the ring's device")
    out = torch.empty((count, num_frames, H, W, 3), dtype=torch.float32, device=ring.device)
    _capi.check(lib.pfnl_op_gather_windows_u10_scenes(C.c_void_p(ring.data_ptr()), C.c_void_p(scene_first.data_ptr()), _req(out, "out"), cap,
                                                      int(last), int(first), count, num_frames, H, W, _stream(ring)))
    return out


def scene_sad_u10(a, b) -> int:
    """sum |Y(a) - Y(b)| of two [H,W,3] uint16 frames (cuda) at 10 bits, Y = (66 R + 129 G + 25 B + 512) >> 10 on min(sample, 1023), as a
    Python int (pfnl_op_scene_sad_u10; exact: pfnl_amd/scene.py frame_sad10).  Synchronises."""
    import torch
    lib = _capi.load_library()
    _req_u16(a, "a")
    _req_u16(b, "b")
    if a.dim() != 3 or a.shape[2] != 3 or b.shape != a.shape or b.device != a.device:
        raise ValueError("scene_sad_u10 expects two [H,W,3] frames on one device")
    out = torch.zeros((1,), dtype=torch.int64, device=a.device)
    _capi.check(lib.pfnl_op_scene_sad_u10(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.shape[0], a.shape[1],
                                          C.c_void_p(out.data_ptr()), _stream(a)))
    return int(out.item())


def resize_u10(frames, out_size, out=None):
    """[n,H,W,3] (or [H,W,3]) uint16 (cuda) with values 0 .. 1023 -> [n,oH,oW,3] uint16, ``out_size`` = (oH, oW): sample for sample
    pfnl_amd/depth10.py resize10 (pfnl_op_resize_u10: the streaming session's resampler at 10 bits).  Each axis between a quarter and
    twice its input; any alignment; ``out``: write there."""
    import torch
    from . import resize as _resize
    lib = _capi.load_library()
    src = _req_u16(frames, "frames")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError("resize_u10 expects [n,H,W,3]")
    n, H, W, _ = frames.shape
    oH, oW = (int(v) for v in out_size)
    _resize.check_limits(H, oH)
    _resize.check_limits(W, oW)
    if out is None:
        out = torch.empty((n, oH, oW, 3), dtype=torch.uint16, device=frames.device)
    elif out.numel() != n * oH * oW * 3 or out.device != frames.device:
        raise ValueError("out must hold n * oH * oW * 3 samples on the frames' device")
    _capi.check(lib.pfnl_op_resize_u10(src, n, H, W, oH, oW, _req_u16(out, "out"), _stream(frames)))
    return out.view(n, oH, oW, 3)


def _resize_place(frames, canvas, src, dst, fill, out, name, req, dtype, limit, hook):
    """Both depths of the placement op: the argument checks of resize_u8 / resize_u10, the rectangles by fit.check_rects."""
    import torch
    from . import fit as _fit
    ptr = req(frames, "frames")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError(f"{name} expects [n,H,W,3]")
    n, H, W, _ = frames.shape
    oH, oW = (int(v) for v in canvas)
    _fit.check_rects(H, W, oH, oW, _fit.as_rect(src, "src", H, W), _fit.as_rect(dst, "dst", oH, oW))
    fill = _fit.as_fill(fill, limit)
    if out is None:
        out = torch.empty((n, oH, oW, 3), dtype=dtype, device=frames.device)
    elif out.numel() != n * oH * oW * 3 or out.device != frames.device:
        raise ValueError("out must hold n * oH * oW * 3 samples on the frames' device")
    ctype = C.c_uint8 if limit == 255 else C.c_uint16
    _capi.check(hook(ptr, n, H, W, oH, oW, _capi.rect_arg(src), _capi.rect_arg(dst), (ctype * 3)(*fill), req(out, "out"), _stream(frames)))
    return out.view(n, oH, oW, 3)


def resize_place_u8(frames, canvas, src=None, dst=None, fill=(0, 0, 0), out=None):
    """[n,H,W,3] (or [H,W,3]) uint8 (cuda) -> [n,oH,oW,3] uint8, ``canvas`` = (oH, oW): ``fill`` everywhere and the resize of the
    rectangle ``src`` = (y, x, h, w) of each frame (None: the whole frame) at the rectangle ``dst`` of the canvas (None: the whole canvas),
    byte for byte pfnl_amd/fit.py place (pfnl_op_resize_place_u8: the streaming session's placement, one launch).  Per axis dst between a
    quarter and twice src; any alignment; ``out``: write there."""
    import torch
    return _resize_place(frames, canvas, src, dst, fill, out, "resize_place_u8", _req_u8, torch.uint8, 255,
                         _capi.load_library().pfnl_op_resize_place_u8)


def resize_place_u10(frames, canvas, src=None, dst=None, fill=(0, 0, 0), out=None):
    """resize_place_u8 on uint16 samples 0 .. 1023: sample for sample pfnl_amd/depth10.py place10 (pfnl_op_resize_place_u10).  ``fill`` holds
    sample values, 0 .. 1023 (depth10.fill10 of an 8-bit colour)."""
    import torch
    return _resize_place(frames, canvas, src, dst, fill, out, "resize_place_u10", _req_u16, torch.uint16, 1023,
                         _capi.load_library().pfnl_op_resize_place_u10)


def score_y(pred_u8, truth_u8, sp_border: int = 8, out=None):
    """Y-channel quality sums of uint8 RGB frame pairs on the device (pfnl_op_score_y): pred_u8, truth_u8 [F,H,W,3] uint8 (cuda)
    -> [F,4] float64 (cuda): sum_d2_full, sum_d2_crop (spatial border sp_border), ssim_sum_full, ssim_sum_valid.
    metrics.sequence_scores turns them into PSNR_Y / SSIM / AVG_PSNR (matlab/compute_psnr.m, modules/SSIM_Index.py:23-89,
    utils.py:213-246).  Asynchronous on the current stream; the partials scratch comes from torch's allocator."""
    import torch
    lib = _capi.load_library()
    for t, name in ((pred_u8, "pred_u8"), (truth_u8, "truth_u8")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous uint8 tensor on the GPU")
    if pred_u8.dim() != 4 or pred_u8.shape[3] != 3 or truth_u8.shape != pred_u8.shape or truth_u8.device != pred_u8.device:
        raise ValueError("score_y expects two [F,H,W,3] tensors of one shape on one device")
    F, H, W, _ = pred_u8.shape
    nbytes = C.c_size_t(0)
    _capi.check(lib.pfnl_op_score_scratch_bytes(F, H, W, C.byref(nbytes)))
    scratch = torch.empty((nbytes.value // 8,), dtype=torch.float64, device=pred_u8.device)
    out = _out(out, (F, 4), torch.float64, pred_u8.device)
    _capi.check(lib.pfnl_op_score_y(C.c_void_p(pred_u8.data_ptr()), C.c_void_p(truth_u8.data_ptr()), F, H, W, int(sp_border),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), _stream(pred_u8)))
    return out


def conv2_chain_ex(x, kernel, bias, base, resid, add_div: int, act: bool = True, mfma: int = 32, split=(0, 0, 0), out=None):
    """The whole of conv2_i in one launch (reference model/pfnl.py:69-71) with the MFMA shape and the split-chain geometry given explicitly
    (pfnl_op_conv2_chain_ex): x = inp1 [F,H,W,64], base [F/add_div,H,W,64], resid [F,H,W,64] (cuda fp32), kernel HWIO [3,3,128,64] ->
    lrelu(conv3x3(concat([base, x])) + bias) + resid.  split = (n_full, split_s, split_q); split_s = 0: no cut.  `out` (optional) is
    written in place."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = x.shape
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    if c != 64 or k.shape != (3, 3, 128, 64) or F % add_div:
        raise ValueError("conv2_chain_ex: geometry mismatch")
    if out is None:
        out = torch.empty((F, H, W, 64), dtype=torch.float32, device=x.device)
    n_full, s, q = (int(v) for v in split)
    _capi.check(lib.pfnl_op_conv2_chain_ex(_req(x, "x"), _hp(k), _hp(b), _req(base, "base"), int(add_div), _req(resid, "resid"),
                                           _req(out, "out"), F, H, W, 1 if act else 0, int(mfma), n_full, s, q, _stream(x)))
    return out


def conv1_conv10_split16_ex(x, k1, b1, k10, b10, frames_per_clip: int, split=(0, 0, 0), out1=None, base=None):
    """conv1_i + conv10_i in one launch (pfnl_op_conv1_conv10_split16_ex; reference model/pfnl.py:66-68) with the split-chain geometry
    split = (n_full, split_s, split_q) given explicitly; results as conv1_conv10_split16."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = x.shape
    T = int(frames_per_clip)
    k1h, k10h = _host(k1, "k1"), _host(k10, "k10")
    if c != 64 or F % T or k1h.size != 9 * 64 * 64 or k10h.size != 64 * T * 64:
        raise ValueError("conv1_conv10_split16_ex: geometry mismatch")
    if out1 is None:
        out1 = torch.empty((F, H, W, 64), dtype=torch.float32, device=x.device)
    if base is None:
        base = torch.empty((F // T, H, W, 64), dtype=torch.float32, device=x.device)
    n_full, s, q = (int(v) for v in split)
    _capi.check(lib.pfnl_op_conv1_conv10_split16_ex(_req(x, "x"), _hp(k1h), _hp(_host(b1, "b1")), _hp(k10h), _hp(_host(b10, "b10")),
                                                    _req(out1, "out1"), _req(base, "base"), F // T, T, H, W, n_full, s, q, _stream(x)))
    return out1, base


def conv1_conv10_split16_mfma(x, k1, b1, k10, b10, frames_per_clip: int, mfma: int = 16, split=(0, 0, 0), out1=None, base=None):
    """conv1_conv10_split16_ex with the MFMA shape of conv1_i's 3x3 stage given (pfnl_op_conv1_conv10_split16_mfma): mfma = 16 runs the
    16x16x32 form of conv3x3_c1c10_kernel (whole rounds only: split must be (0, 0, 0)), 32 the 32x32x16 kernel."""
    import torch
    lib = _capi.load_library()
    F, H, W, c = x.shape
    T = int(frames_per_clip)
    k1h, k10h = _host(k1, "k1"), _host(k10, "k10")
    if c != 64 or F % T or k1h.size != 9 * 64 * 64 or k10h.size != 64 * T * 64:
        raise ValueError("conv1_conv10_split16_mfma: geometry mismatch")
    if out1 is None:
        out1 = torch.empty((F, H, W, 64), dtype=torch.float32, device=x.device)
    if base is None:
        base = torch.empty((F // T, H, W, 64), dtype=torch.float32, device=x.device)
    n_full, s, q = (int(v) for v in split)
    _capi.check(lib.pfnl_op_conv1_conv10_split16_mfma(_req(x, "x"), _hp(k1h), _hp(_host(b1, "b1")), _hp(k10h), _hp(_host(b10, "b10")),
                                                      _req(out1, "out1"), _req(base, "base"), F // T, T, H, W, int(mfma), n_full, s, q,
                                                      _stream(x)))
    return out1, base


def conv3x3_accum_split16_ex(x, kernel, bias=None, act=True, frames_per_clip=1, split=(0, 0, 0), out=None):
    """convmerge1 on the split-f16 kernel (pfnl_op_conv3x3_accum_split16_ex; reference model/pfnl.py:52, :73-74) with the split-chain
    geometry split = (n_full, split_s, split_q) given explicitly.  x [clips*fpc,H,W,64]; kernel HWIO [3,3,64*fpc,cout];
    returns [clips,H,W,64] (channels >= cout: act(0))."""
    import torch
    lib = _capi.load_library()
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    F, H, W, c = x.shape
    T = int(frames_per_clip)
    if k.shape[:3] != (3, 3, 64 * T) or c != 64 or F % T or k.shape[3] > 64:
        raise ValueError("conv3x3_accum_split16_ex: geometry mismatch")
    if out is None:
        out = torch.empty((F // T, H, W, 64), dtype=torch.float32, device=x.device)
    n_full, s, q = (int(v) for v in split)
    _capi.check(lib.pfnl_op_conv3x3_accum_split16_ex(_req(x, "x"), _hp(k), _hp(b), _req(out, "out"), F // T, T, H, W, int(k.shape[3]),
                                                     1 if act else 0, n_full, s, q, _stream(x)))
    return out


def conv3x3_bf16_ex(x, kernel, bias, addend, add_div, resid, act=True, mfma: int = 32, split=(0, 0, 0), out=None):
    """The fused mode of the bf16 3x3 kernel (out = act(conv + bias + addend[item / add_div]) + resid; reference model/pfnl.py:69-71) on the
    third-generation kernel with the MFMA shape and the split-chain geometry given explicitly (pfnl_op_conv3x3_bf16_ex)."""
    import torch
    lib = _capi.load_library()
    k, b = _host(kernel, "kernel"), _host(bias, "bias")
    F, H, W, c = x.shape
    if k.shape != (3, 3, 64, 64) or c != 64 or F % add_div:
        raise ValueError("conv3x3_bf16_ex: geometry mismatch")
    if out is None:
        out = torch.empty_like(x)
    n_full, s, q = (int(v) for v in split)
    _capi.check(lib.pfnl_op_conv3x3_bf16_ex(_req16(x, "x"), _hp(k), _hp(b), _req16(addend, "addend"), int(add_div), _req16(resid, "resid"),
                                            _req16(out, "out"), F, H, W, 1 if act else 0, int(mfma), n_full, s, q, _stream(x)))
    return out


def conv1_conv10_bf16_ex(x, k1, b1, k10, b10, frames_per_clip, mfma: int = 32, split=(0, 0, 0), out1=None, base=None):
    """conv1_i + conv10_i in one launch of the bf16 kernel (reference model/pfnl.py:66-68) on the third-generation kernel with the MFMA
    shape and the split-chain geometry given explicitly (pfnl_op_conv1_conv10_bf16_ex); results as conv1_conv10_bf16."""
    import torch
    lib = _capi.load_library()
    k1h, b1h, k10h, b10h = _host(k1, "k1"), _host(b1, "b1"), _host(k10, "k10"), _host(b10, "b10")
    F, H, W, c = x.shape
    T = int(frames_per_clip)
    if k1h.shape != (3, 3, 64, 64) or k10h.shape != (1, 1, 64 * T, 64) or c != 64 or F % T:
        raise ValueError("conv1_conv10_bf16_ex: geometry mismatch")
    if out1 is None:
        out1 = torch.empty_like(x)
    if base is None:
        base = torch.empty((F // T, H, W, 64), dtype=torch.bfloat16, device=x.device)
    n_full, s, q = (int(v) for v in split)
    _capi.check(lib.pfnl_op_conv1_conv10_bf16_ex(_req16(x, "x"), _hp(k1h), _hp(b1h), _hp(k10h), _hp(b10h), _req16(out1, "out1"),
                                                 _req16(base, "base"), F // T, T, H, W, int(mfma), n_full, s, q, _stream(x)))
    return out1, base



# ---- the content box (include/pfnl_hip.h BARS) ------------------------------------------------------------------------------------------------
def content_box(frames, limit: int = 8, sums: bool = False):
    """Where the picture of each frame lies inside letterbox or pillarbox bars: frames [n,H,W,3] (or one [H,W,3]) uint8, or uint16 at 10
    bits, contiguous on the GPU at any alignment -> an int32 tensor [n,4] of boxes (y0, x0, h, w) on the frames' device, exact against
    pfnl_amd/bars.py frame_box (pfnl_op_content_box_u8 / _u10; one launch for all frames).  ``sums``: also the uint32 sums of luma along
    the rows [n,H] and the columns [n,W] (bars.line_sums), as ``(boxes, rows, cols)``.  Synchronises."""
    import torch
    from . import bars as _bars
    lib = _capi.load_library()
    limit = _bars.check_limit(limit)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype in (torch.uint8, torch.uint16) and frames.is_contiguous()):
        raise TypeError("frames must be a contiguous uint8 or uint16 tensor on the GPU")
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError("content_box expects frames [n,H,W,3]")
    n, H, W = (int(v) for v in frames.shape[:3])
    if not (1 <= H <= _bars.MAX_SIDE and 1 <= W <= _bars.MAX_SIDE):
        raise ValueError(f"content_box: H and W in 1 .. {_bars.MAX_SIDE}")
    box = torch.empty((n, 4), dtype=torch.int32, device=frames.device)
    rows = torch.empty((n, H), dtype=torch.uint32, device=frames.device) if sums else None
    cols = torch.empty((n, W), dtype=torch.uint32, device=frames.device) if sums else None
    hook = lib.pfnl_op_content_box_u8 if frames.dtype == torch.uint8 else lib.pfnl_op_content_box_u10
    _capi.check(hook(C.c_void_p(frames.data_ptr()), n, H, W, limit, C.c_void_p(box.data_ptr()),
                     C.c_void_p(rows.data_ptr()) if sums else None, C.c_void_p(cols.data_ptr()) if sums else None, _stream(frames)))
    return (box, rows, cols) if sums else box
