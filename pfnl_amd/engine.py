"""PFNLEngine — the host-side owner of one libpfnl_hip handle (one GPU).

This is the thin Python layer above the C-ABI: shape/dtype validation, weight hand-over, and the
numpy / torch container handling that ``PFNL.forward`` (pfnl_amd/model.py) needs.  All arithmetic
happens in the HIP kernels behind ``pfnl_forward``; nothing here computes.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import _capi, tiles as _tiles
from .ensemble import members as _members
from .spec import PFNLGeometry, check_weights


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class _PinnedPool:
    """Free page-locked blocks by size.  Thread-safe; blocks in use are owned by their numpy arrays (a finalizer on the array's base
    returns them here)."""

    def __init__(self):
        import threading
        self._free = {}                       # nbytes -> [ptr, ...]
        self._free_bytes = 0
        # re-entrant: the finalizer (_give) takes the lock too, and the cyclic GC may run it on the thread that already holds it inside
        # array() or _give() (a pinned result caught in a reference cycle)
        self._lock = threading.RLock()

    def _cap(self) -> int:
        return int(float(os.environ.get("PFNL_PINNED_POOL_MB", "256")) * (1 << 20))

    def array(self, shape, nbytes: int) -> Optional[np.ndarray]:
        import weakref
        lib = _capi.load_library()
        ptr = None
        with self._lock:
            lst = self._free.get(nbytes)
            if lst:
                ptr = lst.pop()
                self._free_bytes -= nbytes
        if ptr is None:
            p = C.c_void_p()
            if lib.pfnl_host_alloc(nbytes, C.byref(p)) != 0 or not p.value:
                return None                    # no pinned memory to be had: the caller falls back to pageable memory
            ptr = p.value
        base = (C.c_float * (nbytes // 4)).from_address(ptr)
        fin = weakref.finalize(base, self._give, ptr, nbytes)
        fin.atexit = False                     # at interpreter exit the HIP runtime may be gone already: the OS reclaims the blocks
        return np.ctypeslib.as_array(base).reshape(shape)

    def _give(self, ptr: int, nbytes: int) -> None:
        keep = False
        with self._lock:
            if self._free_bytes + nbytes <= self._cap():
                self._free.setdefault(nbytes, []).append(ptr)
                self._free_bytes += nbytes
                keep = True
        if not keep:
            try:
                _capi.load_library().pfnl_host_free(C.c_void_p(ptr))
            except Exception:                  # interpreter shutdown: the OS takes the memory back
                pass

    def free_bytes(self) -> int:
        return self._free_bytes


_pinned_pool = _PinnedPool()


def ensemble_members(n) -> int:
    """``n`` as the C-ABI takes it; ValueError for anything but 1, 2, 4, 8 (the host rule's own check: pfnl_amd/ensemble.py members)."""
    _members(n)
    return int(n)


def tile_argument(tile, shape):
    """``tile`` ((th, tw), (th, tw, pad), (th, tw, pad, batch) or None) for an input of ``shape`` [B,T,H,W,3] as the C-ABI takes it: a
    ``_capi.pfnl_tiling``, or None for None.  ValueError for what pfnl_amd/tiles.py ``check`` refuses; needs no device."""
    if tile is None:
        return None
    t = _tiles.tiling(tile)
    if len(shape) == 5:
        t = _tiles.check(int(shape[2]), int(shape[3]), t)
    return _capi.pfnl_tiling(*t)


class PFNLEngine:
    def __init__(self, geom: PFNLGeometry = PFNLGeometry(), device: int = 0):
        self.geom = geom
        self.device = int(device)
        self._lib = _capi.load_library()
        cfg = _capi.pfnl_config(geom.num_frames, geom.scale, geom.mf, geom.num_block, self.device,
                                (C.c_int32 * 3)(0, 0, 0))
        h = C.c_void_p()
        _capi.check(self._lib.pfnl_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._ready = False
        self._options: Dict[str, str] = {}       # what set_option was called with (the library's own view: get_option)
        self.ensemble = 1                        # members of forward()'s self-ensemble when the call names none (pfnl_amd/ensemble.py)
        self.tile = None                         # forward()'s tiling when the call names none (pfnl_amd/tiles.py); None: the whole frame

    # ---- lifetime --------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.pfnl_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- weights (TF names, HWIO float32) --------------------------------
    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        check_weights(self.geom, weights)
        opt = [(n, s) for n, s in self.geom.optional_weight_shapes() if n in weights]    # theta / phi (nltype 0)
        for name, shape in list(self.geom.weight_shapes()) + opt:
            arr = np.ascontiguousarray(weights[name], dtype=np.float32)
            shp = (C.c_int64 * len(shape))(*shape)
            _capi.check(self._lib.pfnl_set_weight(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p),
                                                  shp, len(shape)))
        _capi.check(self._lib.pfnl_finalize_weights(self._h))
        self._ready = True

    def copy_weights_from(self, other: "PFNLEngine") -> None:
        """Device-to-device replica of ``other``'s packed weights (pfnl_copy_weights): no host tensors, no re-packing."""
        _capi.check(self._lib.pfnl_copy_weights(self._h, other._h))
        self._ready = True

    OPTION_KEYS = ("precision", "strict_fp32", "conv3x3", "conv1x1", "conv2", "merge1", "nonlocal", "nl_type", "nl_sub_sample", "small", "small_c10",
                   "split16_sf", "split16_chain", "split16_c10", "split16_mid", "split16_sf0", "split16_splitchains", "bf16_conv10", "bf16_mfma", "split16_mfma", "graph")

    def clone(self) -> "PFNLEngine":
        """A second handle on the same device with the same weights (device-to-device copy of the packed blobs: pfnl_copy_weights) and the
        same option values as the library holds them now (pfnl_get_option).  Handles are independent: two of them on two streams keep two
        forwards in flight (the harness's small batches, model.py)."""
        other = PFNLEngine(self.geom, device=self.device)
        for k in self.OPTION_KEYS:
            other.set_option(k, self.get_option(k))
        other.copy_weights_from(self)
        other.ensemble = self.ensemble
        other.tile = self.tile
        return other

    def set_option(self, key: str, value: str) -> None:
        """e.g. ("conv3x3", "auto" | "split16" | "winograd" | "winograd_tile" | "direct"); see include/pfnl_hip.h."""
        _capi.check(self._lib.pfnl_set_option(self._h, key.encode(), value.encode()))
        self._options[key] = value

    def option(self, key: str, default: Optional[str] = None) -> Optional[str]:
        """The value this engine's ``set_option(key, ...)`` last took (None / default: never set, the library's default applies)."""
        return self._options.get(key, default)

    def missing_weights(self) -> int:
        n = C.c_int(0)
        _capi.check(self._lib.pfnl_missing_weights(self._h, C.byref(n)))
        return n.value

    # ---- forward ------------------------------------------------------------------------------
    def _check_input(self, shape, dtype_ok: bool):
        if len(shape) != 5:
            raise ValueError(f"expected [B,T,H,W,3], got shape {tuple(shape)}")
        B, T, H, W, c = (int(s) for s in shape)
        if c != 3 or T != self.geom.num_frames:
            raise ValueError(f"expected [B,{self.geom.num_frames},H,W,3], got {tuple(shape)}")
        if B < 1 or H < 2 or W < 2:
            raise ValueError(f"empty or degenerate input {tuple(shape)}")
        if H % 2 or W % 2:
            raise ValueError("H and W must be even (tf.space_to_depth(2), reference model/pfnl.py:57)")
        if not dtype_ok:
            raise TypeError("input must be float32")
        if not self._ready:
            raise RuntimeError("weights have not been loaded")
        return B, T, H, W

    def out_shape(self, B: int, H: int, W: int):
        s = self.geom.scale
        return (B, 1, s * H, s * W, 3)

    def forward(self, x, ensemble=None, tile=None):
        """x: [B,T,H,W,3] float32 (numpy array, torch CPU tensor or torch tensor on this engine's
        GPU) -> [B,1,sH,sW,3] float32 in the same kind of container (reference model/pfnl.py:39-80).
        Host containers: synchronous (H2D + kernels + D2H inside pfnl_forward).  Device tensors:
        enqueued on torch's current stream.  ``ensemble``: 1, 2, 4 or 8 members of the geometric self-ensemble
        (pfnl_forward_ensemble; the rule: pfnl_amd/ensemble.py); None: ``self.ensemble``, 1 unless set - the plain forward.
        ``tile``: (th, tw), (th, tw, pad) or (th, tw, pad, batch) - the frame as runs of ``batch`` overlapping tiles of th x tw with margin
        ``pad`` (pfnl_forward_tiled; the rule: pfnl_amd/tiles.py); None: ``self.tile``, None unless set - the whole frame."""
        n = ensemble_members(self.ensemble if ensemble is None else ensemble)
        t = tile_argument(self.tile if tile is None else tile, np.shape(x))
        if _is_torch(x):
            import torch
            if x.is_cuda:
                B, T, H, W = self._check_input(x.shape, x.dtype == torch.float32)
                if x.device.index != self.device:
                    raise ValueError(f"tensor on {x.device}, engine on cuda:{self.device}")
                x = x.contiguous()
                out = torch.empty(self.out_shape(B, H, W), dtype=torch.float32, device=x.device)
                stream = torch.cuda.current_stream(x.device).cuda_stream
                _capi.check(self._forward(n, C.c_void_p(x.data_ptr()), 1, C.c_void_p(out.data_ptr()), 1, B, H, W, C.c_void_p(stream), t))
                return out
            return torch.from_numpy(self.forward(x.detach().numpy(), ensemble=n, tile=None if t is None else (t.tile_h, t.tile_w, t.pad, t.batch)))
        x = np.asarray(x)
        B, T, H, W = self._check_input(x.shape, x.dtype == np.float32)
        x = np.ascontiguousarray(x)
        out = self._host_output(self.out_shape(B, H, W))
        _capi.check(self._forward(n, x.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.c_void_p), 0, B, H, W, None, t))
        return out

    def _forward(self, n: int, inp, in_is_device: int, out, out_is_device: int, B: int, H: int, W: int, stream, t=None) -> int:
        """pfnl_forward on this handle, pfnl_forward_ensemble with n > 1 members, or pfnl_forward_tiled with a tiling ``t``; the status."""
        if t is not None:
            return self._lib.pfnl_forward_tiled(self._h, inp, in_is_device, out, out_is_device, B, H, W, C.byref(t), n, stream)
        if n == 1:
            return self._lib.pfnl_forward(self._h, inp, in_is_device, out, out_is_device, B, H, W, stream)
        return self._lib.pfnl_forward_ensemble(self._h, inp, in_is_device, out, out_is_device, B, H, W, n, stream)

    @staticmethod
    def _host_output(shape) -> np.ndarray:
        """The numpy array a host-pointer forward fills.  Large results are page-locked (pfnl_host_alloc: pfnl_forward then lets the
        copy engine write the result straight into the array instead of staging it through the handle's pinned strip), from a small pool
        owned by this module: a block goes back to the pool when the last view of its array dies, and the pool keeps at most
        PFNL_PINNED_POOL_MB (default 256) of free blocks - anything beyond that is returned to the OS, so many distinct output shapes do
        not accumulate page-locked memory.  No torch involved.  PFNL_HOST_OUTPUT=pageable: plain numpy memory (staged inside the library)."""
        nbytes = int(np.prod(shape)) * 4
        if nbytes >= (512 << 10) and os.environ.get("PFNL_HOST_OUTPUT", "pinned") != "pageable":
            arr = _pinned_pool.array(shape, nbytes)
            if arr is not None:
                return arr
        return np.empty(shape, np.float32)

    @staticmethod
    def host_output_mode() -> str:
        """"pinned" (pool of pfnl_host_alloc blocks) or "pageable": what bench.py records next to its host-pointer line."""
        return "pageable" if os.environ.get("PFNL_HOST_OUTPUT", "pinned") == "pageable" else "pinned (pfnl_host_alloc pool)"

    def forward_device(self, in_ptr: int, out_ptr: int, B: int, H: int, W: int, stream: int = 0, ensemble: int = 1, tile=None) -> None:
        """Raw device-pointer form (asynchronous on ``stream``; 0 = the legacy null stream, i.e. torch's default stream).
        Asynchronous calls cannot re-run on the f32 kernels when the f16-pipe range flag fires: check ``sync()``.
        ``ensemble``, ``tile``: as for ``forward``; the defaults are the plain forward of the whole frame whatever ``self.ensemble`` and
        ``self.tile`` hold."""
        t = tile_argument(tile, (B, 0, H, W, 3))
        self._check_input((B, self.geom.num_frames, H, W, 3), True)
        _capi.check(self._forward(ensemble_members(ensemble), C.c_void_p(in_ptr), 1, C.c_void_p(out_ptr), 1, B, H, W,
                                  C.c_void_p(stream) if stream else None, t))

    def forward_strip(self, x, out, row0: int, nrows: int) -> None:
        """Single-clip sharding: x [B,T,H,W,3] float32 cuda tensor (the whole clip), out [B,1,sH,sW,3] float32 cuda tensor
        (full size); fills rows [s*row0, s*(row0+nrows)) of ``out`` (pfnl_forward_strip; asynchronous on torch's stream)."""
        import torch
        B, T, H, W = self._check_input(x.shape, x.dtype == torch.float32)
        if not (x.is_cuda and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == self.out_shape(B, H, W)
                and x.is_contiguous() and out.is_contiguous()):
            raise ValueError("forward_strip needs contiguous float32 cuda tensors, out of the full output shape")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _capi.check(self._lib.pfnl_forward_strip(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), B, H, W,
                                                 int(row0), int(nrows), C.c_void_p(stream) if stream else None))

    def open_stream(self, H: int, W: int, batch: int = 1, scene_cut=None, pixel_format="rgb24", out_format=None, matrix="bt709",
                    full_range=False, out_size=None, crop=None, fit=None, place=None, sar=(1, 1), fill=(0, 0, 0),
                    chroma_siting="left", out_chroma_siting=None, in_depth=8, chroma="420", out_chroma=None, packing=None,
                 out_packing=None, interlaced=None, field_order="tff", telecine=None, telecine_params=None, out_matrix=None,
                    out_full_range=None, primaries="bt709", out_primaries=None, bars=None, ensemble=1):
        """A streaming session on this engine (pfnl_stream_open; pfnl_amd/stream.py VideoStream): uint8 LR frames [H,W,3] pushed one at
        a time, uint8 SR frames popped in order, ``batch`` windows per forward.  One open session per engine.  ``scene_cut``: None,
        "manual" or a detector threshold - windows that stay inside a scene (VideoStream).  ``pixel_format`` / ``out_format`` "nv12" or "i420":
        YUV 4:2:0 frames in / out, converted on the device with ``matrix`` and ``full_range`` (pfnl_amd/yuv.py).  ``out_size`` (oH, oW): the raster of the
        delivered frames, resampled on the device (pfnl_amd/resize.py).  ``out_format`` "rgb10", "p010" or "i010": uint16 frames with 10-bit
        values, quantised, resampled and converted at that depth (pfnl_amd/depth10.py).  ``crop`` / ``fit`` / ``place`` / ``sar`` / ``fill``: a
        rectangle of the SR raster on the ``out_size`` canvas - crop, letterbox, aspect fit - in one launch (pfnl_amd/fit.py; VideoStream).
        ``ensemble``: 1, 2, 4 or 8 - every batch's forward as a self-ensemble of that many members (pfnl_amd/ensemble.py); 1: off.
        ``chroma_siting`` / ``out_chroma_siting``: "left", "center" or "topleft" - where a 4:2:0 side's chroma samples sit (pfnl_amd/yuv.py).
        ``in_depth``: 8, or 10 - pushed frames are uint16 in ``pixel_format``'s layout at 10 bits (pfnl_amd/depth10.py; VideoStream).
        ``chroma`` / ``out_chroma``: "420", "422" or "444" - how a YUV side's chroma planes are subsampled (pfnl_amd/yuv.py CHROMAS);
        ``out_chroma`` None: the input's.  ``packing`` / ``out_packing``: None, or a name of pfnl_amd/packed.py PACKINGS - that side as one plane
        of interleaved samples (yuyv422, v210, bgra, ...; VideoStream).  ``interlaced`` None | "frame" | "field", ``field_order`` "tff" | "bff": woven
        frames in, progressive frames into the ring at frame or field rate (pfnl_amd/deinterlace.py; VideoStream).  ``telecine`` None | "match" |
        "decimate" with ``telecine_params``: film under 3:2 pulldown in, its frames into the ring (pfnl_amd/telecine.py; VideoStream).
        ``out_matrix`` / ``out_full_range`` / ``primaries`` / ``out_primaries`` (None: the input's): a colour description per side, the
        primaries converted on the device where they differ (pfnl_amd/colour.py; VideoStream).  ``bars``: None, or a limit in 0 .. 219 - every
        ring frame is measured for letterbox and pillarbox bars on the device (pfnl_amd/bars.py; ``last_info["box"]``, ``content_box``)."""
        from .stream import VideoStream
        return VideoStream(self, H, W, batch, scene_cut, pixel_format, out_format, matrix, full_range, out_size, crop, fit, place, sar, fill,
                           chroma_siting, out_chroma_siting, in_depth, chroma, out_chroma, packing, out_packing, interlaced, field_order,
                           telecine, telecine_params, out_matrix, out_full_range, primaries, out_primaries, bars, ensemble)

    def sync(self) -> None:
        """Synchronise the engine's streams; raises if a device-pointer forward left the f16-pipe kernels' range
        (PFNL_ERR_RANGE, include/pfnl_hip.h "strict_fp32")."""
        _capi.check(self._lib.pfnl_sync(self._h))

    def range_flagged(self) -> bool:
        """Reads and clears the range flag of the device-pointer forwards WITHOUT synchronising (pfnl_range_flag): the caller has
        waited (an event of its own) for the forwards it asks about.  What a pipelined harness checks once per batch."""
        f = C.c_int(0)
        _capi.check(self._lib.pfnl_range_flag(self._h, C.byref(f)))
        return bool(f.value)

    def range_reruns(self) -> int:
        """Host-pointer forwards that were redone on the f32-MFMA kernels (range flag set)."""
        n = C.c_longlong(0)
        _capi.check(self._lib.pfnl_range_reruns(self._h, C.byref(n)))
        return n.value

    def workspace_bytes(self, B: int, H: int, W: int) -> int:
        n = C.c_size_t(0)
        _capi.check(self._lib.pfnl_workspace_bytes(self._h, B, H, W, C.byref(n)))
        return n.value

    def plan(self, B: int, H: int, W: int) -> Dict[str, object]:
        """The launch plan of the progressive-fusion trunk for this shape under the current options (pfnl_plan: the one statement of the
        dispatch rule).  {"structure": "chain2_sf0", "launches_per_block": 2, "conv3x3": "split16", "sf0": 1, ...}."""
        toks = self.plan_text(B, H, W).split()
        d: Dict[str, object] = {"structure": toks[0]}
        for t in toks[1:]:
            k, v = t.split("=", 1)
            d[k] = int(v) if v.lstrip("-").isdigit() else v
        return d

    def plan_text(self, B: int, H: int, W: int) -> str:
        """The string pfnl_plan returns, as it is."""
        buf = C.create_string_buffer(512)
        _capi.check(self._lib.pfnl_plan(self._h, B, H, W, buf, 512))
        return buf.value.decode()

    def get_option(self, key: str) -> str:
        """The CURRENT value of an option (pfnl_get_option): whatever set it - set_option, the environment at pfnl_create, the default."""
        buf = C.create_string_buffer(64)
        _capi.check(self._lib.pfnl_get_option(self._h, key.encode(), buf, 64))
        return buf.value.decode()

    # ---- measurement / debugging ---------------------------------------------------------------
    def profile(self, enable) -> None:
        """False/0: off; True/1: HIP events around every launch; 2: sampled (PF blocks 3, 13, ... from ten blocks up, every 4th below);
        3: the launches of one PF block only (the dominant classes, 3 events per forward)."""
        _capi.check(self._lib.pfnl_profile_enable(self._h, int(enable)))

    def profile_reset(self) -> None:
        _capi.check(self._lib.pfnl_profile_reset(self._h))

    def profile_read(self) -> Dict[str, Dict[str, float]]:
        n = len(_capi.K_NAMES)
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        _capi.check(self._lib.pfnl_profile_read(self._h, ms, cnt))
        return {k: {"ms": ms[i], "launches": int(cnt[i])} for i, k in enumerate(_capi.K_NAMES)}

    def tap(self, name: str, B: int, H: int, W: int) -> np.ndarray:
        T = self.geom.num_frames
        shape = {"nl_out": (B, H, W, 3 * T), "trunk": (B, T, H, W, 64), "merge1": (B, H, W, 48)}[name]
        out = np.empty(shape, np.float32)
        _capi.check(self._lib.pfnl_debug_tap(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.size))
        return out
