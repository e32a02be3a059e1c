"""``python -m pfnl_amd.rawvideo --in-format yuyv422 --size HxW IN OUT``: headerless packed frames through the streaming session.

    ffmpeg -i in.mov -f rawvideo -pix_fmt yuyv422 - | python -m pfnl_amd.rawvideo --in-format yuyv422 --size 270x480 --checkpoint DIR - - \\
        | ffmpeg -f rawvideo -pix_fmt yuyv422 -s 1920x1080 -i - out.mkv

A raw stream is frames of ``packed.frame_bytes`` one behind the other and nothing else (pfnl_amd/packed.py; what ``ffmpeg -f rawvideo
-pix_fmt NAME -s WxH`` speaks - its names are this module's: bgr24, rgba, bgra, yuyv422, uyvy422, x2rgb10le = x2rgb10, x2bgr10le = x2bgr10,
y210le = y210; v210 comes from ``-c:v v210``), so format, size, matrix, range and siting are the command line's.  A colour description per side (pfnl_amd/colour.py):
``--primaries``, ``--out-matrix``, ``--out-range``, ``--out-primaries``, as pfnl_amd/upscale.py takes them - a DVD's capture to HD is
``--matrix bt601 --primaries auto --out-matrix auto --out-primaries auto``.  ``RawReader`` /
``RawWriter`` move the frames, ``session_keywords`` turns two packing names into ``open_stream``'s keywords - each side's family, depth and
chroma format follow from its packing -, ``run()`` is the loop (it mirrors pfnl_amd/upscale.py ``upscale``), ``main()`` the command line;
nothing here computes.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from . import colour as _colour, packed as _packed, telecine as _telecine


class RawReader:
    """Frames of ``packed.frame_bytes(name, H, W)`` from a binary file object, as uint8 arrays of ``packed.frame_shape``.  The stream ends
    at a frame boundary; a short last frame is a ValueError that names the frame.  ``frames`` counts what has been read."""

    def __init__(self, file, name: str, H: int, W: int):
        self.name, self.height, self.width = name, int(H), int(W)
        self.shape = _packed.frame_shape(name, self.height, self.width)          # (ValueError for a size the packing does not take)
        self.frame_bytes = _packed.frame_bytes(name, self.height, self.width)
        self.frames = 0
        self._file = file

    def __iter__(self):
        return self

    def __next__(self):
        data = b""
        while len(data) < self.frame_bytes:                                      # (a pipe hands over what it has)
            more = self._file.read(self.frame_bytes - len(data))
            if not more:
                break
            data += more
        if not data:
            raise StopIteration
        if len(data) != self.frame_bytes:
            raise ValueError(f"frame {self.frames}: {len(data)} bytes where a {self.name} frame of {self.height} x {self.width} has {self.frame_bytes}")
        self.frames += 1
        return np.frombuffer(data, np.uint8).reshape(self.shape)


class RawWriter:
    """Frames to a binary file object as their bytes, one behind the other."""

    def __init__(self, file):
        self.frames = 0
        self._file = file

    def write_frame(self, frame) -> None:
        self._file.write(np.ascontiguousarray(frame).tobytes())
        self.frames += 1


def side_keywords(name: str) -> dict:
    """What a side that carries the packing ``name`` is set to: ``format`` (the layout name that says its family and, on the output side,
    its depth), ``depth`` and ``chroma``."""
    yuv, depth = _packed.is_yuv(name), _packed.bits(name)
    return {"format": ("i420" if yuv else "rgb24") if depth == 8 else ("i010" if yuv else "rgb10"), "depth": depth, "chroma": "422" if yuv else "420"}


def session_keywords(in_format: str, out_format=None, **session_kw) -> dict:
    """``open_stream``'s keywords for raw frames of ``in_format`` in and ``out_format`` out (None: the same): the caller's (``batch``,
    ``matrix``, ``full_range``, ``chroma_siting``, ``out_chroma_siting``, ``out_size``, ...) and, from the two packings, the layouts, the
    input depth and the chroma formats.  ValueError for a pair the session does not take (an RGB 10-bit output goes with RGB input)."""
    kw = dict(session_kw)
    for fixed in ("pixel_format", "out_format", "in_depth", "chroma", "out_chroma", "packing", "out_packing"):
        if fixed in kw:
            raise ValueError(f"{fixed} follows from the two formats")
    out_format = in_format if out_format is None else out_format
    a, b = side_keywords(in_format), side_keywords(out_format)
    kw.setdefault("batch", 1)
    kw["pixel_format"] = {"i010": "i420", "rgb10": "rgb24"}.get(a["format"], a["format"])   # (the input's depth is a keyword of its own)
    kw["out_format"] = b["format"]
    if kw["out_format"] == "rgb10" and kw["pixel_format"] != "rgb24":
        raise ValueError(f"--out-format {out_format}: a 10-bit RGB output goes with RGB input, got {in_format}")
    if a["depth"] == 10:
        kw["in_depth"] = 10
    if a["chroma"] != "420" or b["chroma"] != "420":
        kw["chroma"], kw["out_chroma"] = a["chroma"], b["chroma"]
    kw["packing"], kw["out_packing"] = in_format, out_format
    return kw


def run(reader, writer, open_stream, out_format=None, log=None, **session_kw) -> int:
    """Every frame of ``reader`` (RawReader) through a session, into ``writer`` (RawWriter); returns the frame count.  ``open_stream`` is
    ``PFNLEngine.open_stream`` or anything with its keywords; ``session_kw`` as ``session_keywords`` takes them.  Frames are written in
    index order as ``push`` and ``end`` return them - with ``interlaced="field"`` (and ``field_order``: a raw pipe has no header to say) two per
    frame read.  ``out_matrix``, ``out_range``, ``primaries``, ``out_primaries`` (and ``scale``, 4 unless given) as pfnl_amd/upscale.py
    ``session_keywords`` takes them: each reaches the session only where it is named.  One line with frames, seconds and fps goes to ``log``."""
    session_kw = dict(session_kw)
    named = {k: session_kw.pop(k, None) for k in ("out_matrix", "out_range", "primaries", "out_primaries")}
    scale = session_kw.pop("scale", 4)
    kw = session_keywords(reader.name, out_format, **session_kw)
    out_size = kw.get("out_size")
    kw.update(_colour.side_keywords(reader.height, out_size[0] if out_size is not None else scale * reader.height, kw.get("matrix", "bt709"), **named))
    batch = kw.pop("batch")
    t0 = time.perf_counter()
    done = 0
    with open_stream(reader.height, reader.width, batch, **kw) as vs:

        def deliver(frames):
            nonlocal done
            for index, frame in frames:
                if index != done:
                    raise RuntimeError(f"frame {index} delivered where {done} was due")
                writer.write_frame(frame)
                done += 1

        for frame in reader:
            deliver(vs.push(frame))
        deliver(vs.end())
    due = reader.frames * (2 if kw.get("interlaced") == "field" else 1)   # (at field rate a woven frame is two)
    if kw.get("telecine") is not None:                                    # (film: every frame, or four in five)
        due = _telecine.deliverable(kw["telecine"], reader.frames, True)
    if done != due:
        raise RuntimeError(f"{reader.frames} frames read, {done} delivered where {due} were due")
    seconds = time.perf_counter() - t0
    print(f"pfnl_amd.rawvideo: {done} frames in {seconds:.2f} s ({done / seconds if seconds > 0 else 0.0:.2f} fps)",
          file=sys.stderr if log is None else log)
    return done


def _size(text):
    try:
        h, w = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"HxW, got {text!r}") from None
    return h, w


def parser() -> argparse.ArgumentParser:
    names = _packed.PACKINGS[1:]
    ap = argparse.ArgumentParser(prog="python -m pfnl_amd.rawvideo", description="Upscale headerless packed frames 4x with PFNL on the GPU.")
    ap.add_argument("input", metavar="IN", help="a file of raw frames, or - for stdin")
    ap.add_argument("output", metavar="OUT", help="the file to write, or - for stdout")
    ap.add_argument("--in-format", choices=names, required=True)
    ap.add_argument("--size", type=_size, required=True, metavar="HxW", help="the input frames' rows x columns")
    ap.add_argument("--out-format", choices=names, default=None, help="default: the input's")
    w = ap.add_mutually_exclusive_group(required=True)
    w.add_argument("--checkpoint", metavar="DIR", help="the directory of a trained checkpoint")
    w.add_argument("--synthetic-weights", metavar="SEED", type=int, help="seeded random weights (for trying the pipeline)")
    ap.add_argument("--num-block", type=int, default=20)
    ap.add_argument("--matrix", choices=("bt601", "bt709"), default="bt709")
    ap.add_argument("--full-range", action="store_true")
    ap.add_argument("--out-matrix", choices=("auto", "bt601", "bt709"), default=None, help="the output's matrix (default: the input's); auto: bt709 above 576 delivered lines")
    ap.add_argument("--out-range", choices=("limited", "full"), default=None, help="the output's range (default: the input's)")
    ap.add_argument("--primaries", choices=("auto",) + _colour.PRIMARIES, default=None,
                    help="the input's primaries (default: bt709); auto: bt601-525 at 480 / 486 lines, bt601-625 at 576, else bt709")
    ap.add_argument("--out-primaries", choices=("auto",) + _colour.PRIMARIES, default=None,
                    help="the output's primaries (default: the input's), converted on the device; auto: bt709 above 576 delivered lines")
    ap.add_argument("--siting", choices=("left", "center", "topleft"), default="left", help="where the 4:2:2 chroma samples sit, in and out")
    ap.add_argument("--batch", type=int, default=1, help="windows per forward")
    ap.add_argument("--out-size", type=_size, default=None, metavar="HxW")
    ap.add_argument("--interlaced", choices=("frame", "field"), default=None,
                    help="the frames are woven fields: deinterlace on the device, one progressive frame per frame or per field")
    ap.add_argument("--ivtc", choices=("match", "decimate"), default=None,
                    help="the frames are film under 3:2 pulldown: match the fields on the device; decimate also drops the repeat (needs --batch 2 or more)")
    ap.add_argument("--field-order", choices=("tff", "bff"), default="tff", help="which field of a woven frame comes first (a raw pipe has no header)")
    return ap


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    from ._capi import PFNLHipError
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
    eng = None
    try:
        reader = RawReader(fin, a.in_format, *a.size)
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
        woven = {} if a.interlaced is None else {"interlaced": a.interlaced, "field_order": a.field_order}
        if a.ivtc is not None:
            if a.interlaced is not None:
                raise ValueError("--ivtc and --interlaced are exclusive: film carried in fields is matched, video is deinterlaced")
            woven = {"telecine": a.ivtc, "field_order": a.field_order}
        run(reader, RawWriter(fout), eng.open_stream, out_format=a.out_format, batch=a.batch, matrix=a.matrix, full_range=a.full_range,
            chroma_siting=a.siting, out_size=a.out_size, scale=geom.scale, **woven,
            **{k: v for k, v in (("out_matrix", a.out_matrix), ("out_range", a.out_range), ("primaries", a.primaries),
                                 ("out_primaries", a.out_primaries)) if v is not None})
        fout.flush()
    except (ValueError, PFNLHipError) as e:
        print(f"pfnl_amd.rawvideo: {e}", file=sys.stderr)
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
