"""``python -m pfnl_amd.upscale IN OUT``: a Y4M stream through the streaming session, end to end.

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m pfnl_amd.upscale --checkpoint DIR - - | ffmpeg -f yuv4mpegpipe -i - out.mkv

The stream's header (pfnl_amd/y4m.py) names the raster, the chroma siting, the range and the sample aspect ratio; the frames are the
session's ``i420`` frames as they are, converted on the device with that siting (pfnl_amd/yuv.py), and what the session delivers is written
as ``i420`` - or ``i010`` with ``--bits 10`` - under a header of the output's raster, siting and aspect.  A ``C420p10`` stream (``ffmpeg
-pix_fmt yuv420p10le -f yuv4mpegpipe``) is taken at its own depth - uint16 frames into a session opened with ``in_depth=10`` - and wants
``--bits 10``: at the default of 8 the ten bits are kept on the way in and cut on the way out.  Y4M carries no matrix: ``--matrix
auto`` takes BT.601 up to 576 lines and BT.709 above.  4:2:2 and 4:4:4 streams (``C422``, ``C444``, ``C422p10``, ``C444p10``) are taken
where ``--chroma`` names them (or ``any``) - without it such a stream exits 1 naming its tag - and ``--out-chroma`` sets the subsampling of
the output apart from the input's; a ``C422`` stream is horizontally co-sited, so a 4:2:2 output is written with the siting "left".  Interlaced streams (``It`` / ``Ib``, what ``ffmpeg -f yuv4mpegpipe`` writes for DVD and broadcast material) are taken with
``--deinterlace frame|field`` - without it such a stream exits 1 naming its tag -: the frames are woven, the field order is the header's, the
session deinterlaces on the device (pfnl_amd/deinterlace.py) and the output is ``Ip``, at field rate with twice the frames and ``F`` doubled.
A colour description per side (pfnl_amd/colour.py): ``--primaries``, ``--out-matrix``, ``--out-range`` and ``--out-primaries``; ``auto`` takes
480 / 486 lines as bt601-525, 576 as bt601-625 and anything else as bt709 on the way in, and on the way out BT.709 above 576 delivered
lines, else the input's.  A DVD to HD, in the colours an HD stream is read as:

    ffmpeg -i dvd.vob -f yuv4mpegpipe - | python -m pfnl_amd.upscale --checkpoint DIR --deinterlace frame --out-size 1080x1440 \\
        --primaries auto --out-matrix auto --out-primaries auto - - | ffmpeg -f yuv4mpegpipe -i - -colorspace bt709 -color_primaries bt709 hd.mkv

Letterbox and pillarbox bars (pfnl_amd/bars.py): ``--crop auto`` reads up to ``--crop-probe`` frames, measures on the device where their
picture lies (``--crop-limit``: the mean luma a bar stays under), says ``crop Y,X,H,W (from K frames)`` on stderr and opens the session at
that size; ``--crop Y,X,H,W`` names the rectangle, in input pixels on bars.align()'s grid.  Each frame is then pushed as a window of its
planes, so the network never sees the bars, and ``--out-size`` / ``--fit`` work on the cropped picture.  A non-anamorphic widescreen DVD:

    ffmpeg -i dvd.vob -f yuv4mpegpipe - | python -m pfnl_amd.upscale --checkpoint DIR --deinterlace frame --crop auto - - | ffmpeg -f yuv4mpegpipe -i - film.mkv

``upscale()`` is the loop, ``main()`` the command line; nothing here computes.
"""
from __future__ import annotations

import argparse
import sys
import time

from . import bars as _bars, colour as _colour, telecine as _telecine, y4m as _y4m

OUT_FORMATS = {8: "i420", 10: "i010"}


def auto_matrix(height: int) -> str:
    """What a stream without a matrix tag is taken to be: BT.601 up to 576 lines (SD), BT.709 above."""
    return "bt601" if height <= 576 else "bt709"


def session_keywords(header, **session_kw) -> dict:
    """``open_stream``'s keywords for a stream with this header: the caller's (``batch``, ``scene_cut``, ``out_format`` "i420" | "i010",
    ``out_size``, ``fit``, ``out_chroma_siting``, ``out_chroma``, ``ensemble``, ``matrix`` with "auto", ``full_range`` True to override the
    header), and from the header the input siting, the range, ``in_depth=10`` for a 10-bit stream (and no such key for an 8-bit one),
    ``chroma`` for a 4:2:2 / 4:4:4 stream (and no such key for a 4:2:0 one; ``out_chroma`` likewise only where the caller names one) and -
    with ``fit`` alone - the sample aspect ratio.  A 4:2:2 output is co-sited across, as ``C422`` says: ``out_chroma_siting`` becomes "left"
    where the caller names none.  ``deinterlace`` ("frame" | "field") becomes ``interlaced`` with the header's field order for an ``It`` / ``Ib``
    stream (and no such key for a progressive one); without it such a stream is a ValueError that names its tag.  ``ivtc`` ("match" |
    "decimate") becomes ``telecine`` with the header's field order instead - the stream is film under 3:2 pulldown (pfnl_amd/telecine.py) -;
    the two are exclusive.  ``out_matrix`` ("auto" | "bt601" | "bt709"), ``out_range`` ("limited" | "full"), ``primaries`` and ``out_primaries``
    ("auto" | a name of pfnl_amd/colour.py PRIMARIES) become ``open_stream``'s colour keywords, each only where the caller names it
    (colour.side_keywords; ``scale``, 4 unless given, says how many lines a session without ``out_size`` delivers - of ``crop_height``
    lines where a crop ahead of the network leaves fewer than the header's).  ValueError for what a Y4M stream cannot hold."""
    kw = dict(session_kw)
    for fixed in ("pixel_format", "chroma_siting", "sar", "in_depth", "chroma", "interlaced", "field_order", "telecine"):
        if fixed in kw:
            raise ValueError(f"{fixed} comes from the stream's header")
    kw.setdefault("batch", 1)
    named = {k: kw.pop(k, None) for k in ("out_matrix", "out_range", "primaries", "out_primaries")}
    scale = kw.pop("scale", 4)
    lines = kw.pop("crop_height", None) or header.height
    rate = kw.pop("deinterlace", None)                # "frame" | "field": what an It / Ib stream needs; a progressive stream ignores it
    if rate not in (None, "frame", "field"):
        raise ValueError(f'deinterlace: None, "frame" or "field", got {rate!r}')
    ivtc = kw.pop("ivtc", None)                       # "match" | "decimate": an It / Ib stream that carries film
    if ivtc not in (None, "match", "decimate"):
        raise ValueError(f'ivtc: None, "match" or "decimate", got {ivtc!r}')
    if ivtc is not None and rate is not None:
        raise ValueError("--ivtc and --deinterlace are exclusive: film carried in fields is matched, video is deinterlaced")
    if header.interlace in ("t", "b"):
        if rate is None and ivtc is None:
            raise ValueError(f"y4m: an interlaced stream (I{header.interlace}) needs --deinterlace frame or field, or --ivtc")
        kw["telecine" if rate is None else "interlaced"] = ivtc if rate is None else rate
        kw["field_order"] = "tff" if header.interlace == "t" else "bff"
    if kw.get("out_format") is None:
        kw["out_format"] = "i420"
    if kw["out_format"] not in OUT_FORMATS.values():
        raise ValueError(f"out_format: a Y4M stream holds {sorted(OUT_FORMATS.values())}, got {kw['out_format']!r}")
    if kw.get("matrix", "auto") == "auto":
        kw["matrix"] = auto_matrix(header.height)
    kw["full_range"] = bool(kw.get("full_range")) or header.full_range
    out_size = kw.get("out_size")
    kw.update(_colour.side_keywords(header.height, out_size[0] if out_size is not None else scale * lines, kw["matrix"], **named))
    kw["pixel_format"] = "i420"
    kw["chroma_siting"] = header.siting
    if header.bits == 10:
        kw["in_depth"] = 10
    in_chroma = header.chroma
    if in_chroma != "420":
        kw["chroma"] = in_chroma
    if kw.get("out_chroma") is None:
        kw.pop("out_chroma", None)
    elif kw["out_chroma"] not in _y4m.CHROMAS:
        raise ValueError(f"out_chroma: one of {_y4m.CHROMAS}, got {kw['out_chroma']!r}")
    if kw.get("out_chroma", in_chroma) == "422":
        if kw.get("out_chroma_siting") is None:
            kw["out_chroma_siting"] = "left"
        elif kw["out_chroma_siting"] == "center":
            raise ValueError("out_chroma_siting: a Y4M C422 stream is horizontally co-sited (\"left\"), got 'center'")
    if kw.get("fit") is not None:
        kw["sar"] = header.sar
    return kw


def frame_planes(frame, header) -> tuple:
    """(Y, Cb, Cr) of a frame as y4m.Y4MReader yields it: views, nothing is copied."""
    H, W = header.height, header.width
    ch, cw = (H // 2 if header.chroma == "420" else H), (W if header.chroma == "444" else W // 2)
    flat = frame.reshape(-1)
    return flat[:H * W].reshape(H, W), flat[H * W:H * W + ch * cw].reshape(ch, cw), flat[H * W + ch * cw:].reshape(ch, cw)


def window_planes(frame, header, box) -> tuple:
    """The window ``box`` = (y0, x0, h, w), on bars.align()'s grid, of a frame's planes: strided views for ``push_planes``."""
    y0, x0, h, w = box
    sy, sx = (2 if header.chroma == "420" else 1), (1 if header.chroma == "444" else 2)
    y, cb, cr = frame_planes(frame, header)
    return (y[y0:y0 + h, x0:x0 + w], cb[y0 // sy:(y0 + h) // sy, x0 // sx:(x0 + w) // sx], cr[y0 // sy:(y0 + h) // sy, x0 // sx:(x0 + w) // sx])


def measure_on_device(frames, header, limit, matrix="bt601", full_range=False, chunk=16) -> list:
    """The content box of every frame of a Y4M stream (pfnl_amd/bars.py), measured on the GPU: decoded as they are - woven frames too:
    bars are black in both fields - by ``ops.yuv_to_rgb`` / ``yuv_to_rgb_u10`` and boxed by ``ops.content_box``, ``chunk`` frames a launch."""
    import numpy as np
    import torch
    from . import ops
    decode, fmt = (ops.yuv_to_rgb_u10, "i010") if header.bits == 10 else (ops.yuv_to_rgb, "i420")
    boxes = []
    for k in range(0, len(frames), chunk):
        host = np.stack([np.asarray(f).reshape(-1) for f in frames[k:k + chunk]])
        packed = torch.from_numpy(host.view(np.int16)).cuda().view(torch.uint16) if header.bits == 10 else torch.from_numpy(host).cuda()
        rgb = decode(packed.reshape(-1), fmt, header.height, header.width, matrix, full_range, header.chroma, header.siting)
        boxes += [tuple(b) for b in ops.content_box(rgb, limit).cpu().tolist()]
    return boxes


def resolve_crop(reader, crop, limit=_bars.LIMIT, probe=120, measure=None, matrix="bt601", full_range=False, log=None):
    """(box or None, the frames read ahead): ``crop`` "auto" reads up to ``probe`` frames, has ``measure(frames, header, limit)`` box them
    (measure_on_device unless given), applies bars.decide on bars.align()'s grid and says so on ``log``; a rectangle is checked against
    the frame and that grid (ValueError naming the reason).  None: the whole frame - no crop, the session as it always was."""
    header = reader.header
    H, W = header.height, header.width
    ay, ax = _bars.align(header.chroma, header.interlace in ("t", "b"))
    ahead = []
    if crop == "auto":
        limit = _bars.check_limit(limit)
        if int(probe) < 1:
            raise ValueError(f"crop-probe: at least 1 frame, got {probe!r}")
        while len(ahead) < int(probe):
            frame = reader.read_frame()
            if frame is None:
                break
            ahead.append(frame)
        if measure is None:
            measure = lambda frames, head, lim: measure_on_device(frames, head, lim, matrix, full_range)   # noqa: E731
        box = _bars.decide(measure(ahead, header, limit) if ahead else [], H, W, ay, ax)
        print("crop %d,%d,%d,%d (from %d frames)" % (*box, len(ahead)), file=sys.stderr if log is None else log)
    else:
        box = _bars.check_crop(crop, H, W, ay, ax)
    return (None if box == (0, 0, H, W) else box), ahead


def upscale(reader, writer, open_stream, tile=None, log=None, crop=None, crop_limit=_bars.LIMIT, crop_probe=120, measure=None,
            **session_kw) -> int:
    """Every frame of ``reader`` (y4m.Y4MReader) through a session, into ``writer`` (y4m.Y4MWriter); returns the frame count.
    ``open_stream`` is ``PFNLEngine.open_stream`` or anything with its keywords; ``session_kw`` as ``session_keywords`` takes them;
    ``tile`` is ``set_tiling``'s arguments.  The output header is written once the session exists - its raster, siting and aspect are the
    session's - and frames in index order as ``push`` and ``end`` return them.  One line with frames, seconds and fps goes to ``log``.
    ``crop`` ("auto" | (y0, x0, h, w) in input pixels; ``resolve_crop`` with ``crop_limit``, ``crop_probe`` and ``measure``): the session is
    opened at the cropped size and every frame goes in as a window of its planes (``push_planes``), the frames read ahead first; a crop
    that is the whole frame, and no ``crop``, is the loop as it always was."""
    header = reader.header
    kw = session_keywords(header, **session_kw)
    box, ahead = None, []
    if crop is not None:
        box, ahead = resolve_crop(reader, crop, crop_limit, crop_probe, measure, kw["matrix"], kw["full_range"], log)
        if box is not None:
            kw = session_keywords(header, crop_height=box[2], **session_kw)
    in_h, in_w = (header.height, header.width) if box is None else box[2:]
    batch = kw.pop("batch")
    t0 = time.perf_counter()
    done = 0
    with open_stream(in_h, in_w, batch, **kw) as vs:
        if tile is not None:
            vs.set_tiling(*tile)
        out_h, out_w = vs.out_size if vs.out_size is not None else (vs.scale * in_h, vs.scale * in_w)
        out_chroma = kw.get("out_chroma", kw.get("chroma", "420"))
        writer.write_header(header.for_output(out_w, out_h, siting=vs.out_chroma_siting, bits=10 if kw["out_format"] == "i010" else 8,
                                              sar=(1, 1) if kw.get("fit") is not None else header.sar, full_range=kw.get("out_full_range", kw["full_range"]), chroma=out_chroma,
                                              progressive="interlaced" in kw or "telecine" in kw, double_rate=kw.get("interlaced") == "field",
                                              film_rate=kw.get("telecine") == "decimate"))

        def deliver(frames):
            nonlocal done
            for index, frame in frames:
                if index != done:
                    raise RuntimeError(f"frame {index} delivered where {done} was due")
                writer.write_frame(frame)
                done += 1

        def frames():
            yield from ahead
            yield from reader

        for frame in frames():
            deliver(vs.push(frame) if box is None else vs.push_planes(*window_planes(frame, header, box)))
        deliver(vs.end())
    due = reader.frames * (2 if kw.get("interlaced") == "field" else 1)
    if kw.get("telecine") is not None:
        due = _telecine.deliverable(kw["telecine"], reader.frames, True)
    if done != due:
        raise RuntimeError(f"{reader.frames} frames read, {done} delivered where {due} were due")
    seconds = time.perf_counter() - t0
    print(f"pfnl_amd.upscale: {done} frames in {seconds:.2f} s ({done / seconds if seconds > 0 else 0.0:.2f} fps)",
          file=sys.stderr if log is None else log)
    return done


def _size(text):
    try:
        h, w = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"HxW, got {text!r}") from None
    return h, w


def _tile(text):
    try:
        t = tuple(int(v) for v in text.split(","))
    except ValueError:
        t = ()
    if not 2 <= len(t) <= 4:
        raise argparse.ArgumentTypeError(f"TH,TW[,PAD[,BATCH]], got {text!r}")
    return t


def _crop(text):
    try:
        return _bars.parse_crop(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _scene_cut(text):
    if text == "manual":
        raise argparse.ArgumentTypeError("a Y4M stream carries no cut marks: give the detector's threshold")
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a threshold in (0, 255], got {text!r}") from None


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m pfnl_amd.upscale", description="Upscale a Y4M stream 4x with PFNL on the GPU.")
    ap.add_argument("input", metavar="IN", help="a Y4M file, or - for stdin")
    ap.add_argument("output", metavar="OUT", help="the Y4M file to write, or - for stdout")
    w = ap.add_mutually_exclusive_group(required=True)
    w.add_argument("--checkpoint", metavar="DIR", help="the directory of a trained checkpoint")
    w.add_argument("--synthetic-weights", metavar="SEED", type=int, help="seeded random weights (for trying the pipeline)")
    ap.add_argument("--num-block", type=int, default=20)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--matrix", choices=("auto", "bt601", "bt709"), default="auto", help="auto: bt601 up to 576 lines, else bt709")
    ap.add_argument("--full-range", action="store_true", help="full-range samples whatever the header says")
    ap.add_argument("--out-matrix", choices=("auto", "bt601", "bt709"), default=None, help="the output's matrix (default: the input's); auto: bt709 above 576 delivered lines")
    ap.add_argument("--out-range", choices=("limited", "full"), default=None, help="the output's range (default: the input's)")
    ap.add_argument("--primaries", choices=("auto",) + _colour.PRIMARIES, default=None,
                    help="the input's primaries (default: bt709); auto: bt601-525 at 480 / 486 lines, bt601-625 at 576, else bt709")
    ap.add_argument("--out-primaries", choices=("auto",) + _colour.PRIMARIES, default=None,
                    help="the output's primaries (default: the input's), converted on the device; auto: bt709 above 576 delivered lines")
    ap.add_argument("--batch", type=int, default=1, help="windows per forward")
    ap.add_argument("--scene-cut", type=_scene_cut, default=None, metavar="THRESHOLD", help="keep windows inside a scene: the cut detector's threshold")
    ap.add_argument("--bits", type=int, choices=(8, 10), default=8, help="10: yuv420p10le out (what a 10-bit source wants)")
    ap.add_argument("--out-size", type=_size, default=None, metavar="HxW")
    ap.add_argument("--fit", choices=("contain", "cover"), default=None, help="keep the aspect ratio on the --out-size canvas")
    ap.add_argument("--out-siting", choices=("left", "center", "topleft"), default=None, help="the output's chroma siting (default: the input's)")
    ap.add_argument("--chroma", choices=("420", "422", "444", "any"), default="420", help="the subsampling of the input stream that is taken")
    ap.add_argument("--out-chroma", choices=("420", "422", "444"), default=None, help="the output's subsampling (default: the input's)")
    ap.add_argument("--ensemble", type=int, choices=(1, 2, 4, 8), default=1)
    ap.add_argument("--deinterlace", choices=("frame", "field"), default=None,
                    help="take an interlaced (It / Ib) stream: one progressive frame per frame, or per field (twice the frames and the rate)")
    ap.add_argument("--ivtc", action="store_true",
                    help="take an It / Ib stream that carries film under 3:2 pulldown: match the fields and drop the repeat (4/5 of the frames and the rate; needs --batch 2 or more)")
    ap.add_argument("--no-decimate", action="store_true", help="with --ivtc: match the fields and keep every frame")
    ap.add_argument("--tile", type=_tile, default=None, metavar="TH,TW[,PAD[,BATCH]]")
    ap.add_argument("--crop", type=_crop, default=None, metavar="auto|Y,X,H,W",
                    help="crop ahead of the network, in input pixels: auto measures the letterbox / pillarbox bars of the first frames on the device")
    ap.add_argument("--crop-limit", type=int, default=_bars.LIMIT, metavar="L", help="with --crop auto: the mean luma (0 .. 219, black 0) a bar stays under")
    ap.add_argument("--crop-probe", type=int, default=120, metavar="N", help="with --crop auto: the frames that are measured")
    return ap


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    from ._capi import PFNLHipError
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
    eng = None
    try:
        reader = _y4m.Y4MReader(fin, depths=(8, 10), chromas=_y4m.CHROMAS if a.chroma == "any" else (a.chroma,),
                                   interlaced=a.deinterlace is not None or a.ivtc)
        if a.no_decimate and not a.ivtc:
            raise ValueError("--no-decimate goes with --ivtc")
        if a.crop is not None and a.crop != "auto":   # (ahead of the engine: a bad rectangle needs no device to be named)
            head = reader.header
            _bars.check_crop(a.crop, head.height, head.width, *_bars.align(head.chroma, head.interlace in ("t", "b")))
        from . import checkpoint, synth
        from .engine import PFNLEngine
        from .spec import PFNLGeometry
        geom = PFNLGeometry(num_block=a.num_block)
        if a.checkpoint is not None:
            found = checkpoint.load_checkpoint(a.checkpoint, geom)
            if found is None:
                raise ValueError(f"no checkpoint in {a.checkpoint!r}")
            weights = found[1]
        else:
            weights = synth.synthetic_weights(geom, seed=a.synthetic_weights)
        eng = PFNLEngine(geom, device=0)
        eng.load_weights(weights)
        if a.precision != "fp32":
            eng.set_option("precision", a.precision)
        upscale(reader, _y4m.Y4MWriter(fout), eng.open_stream, tile=a.tile, batch=a.batch, scene_cut=a.scene_cut, matrix=a.matrix,
                full_range=a.full_range, out_format=OUT_FORMATS[a.bits], out_size=a.out_size, fit=a.fit, out_chroma_siting=a.out_siting,
                ensemble=a.ensemble, out_chroma=a.out_chroma, deinterlace=a.deinterlace,
                ivtc=("match" if a.no_decimate else "decimate") if a.ivtc else None, scale=geom.scale,
                **({} if a.crop is None else {"crop": a.crop, "crop_limit": a.crop_limit, "crop_probe": a.crop_probe}),
                **{k: v for k, v in (("out_matrix", a.out_matrix), ("out_range", a.out_range), ("primaries", a.primaries),
                                     ("out_primaries", a.out_primaries)) if v is not None})
        fout.flush()
    except (ValueError, PFNLHipError) as e:
        print(f"pfnl_amd.upscale: {e}", file=sys.stderr)
        return 1
    finally:
        if eng is not None:
            eng.close()
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
