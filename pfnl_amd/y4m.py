"""YUV4MPEG2 (Y4M) streams, 4:2:0 and - where the caller asks - 4:2:2 / 4:4:4 (numpy only; no device): what ``ffmpeg -f yuv4mpegpipe`` writes and reads.

A stream is one header line and, per frame, a ``FRAME`` line followed by the planes Y [H][W], Cb [H/2][W/2], Cr [H/2][W/2] - exactly the
streaming session's tightly packed ``i420`` frame (pfnl_amd/yuv.py), so ``Y4MReader`` yields ``(H*3//2, W)`` uint8 arrays that
``VideoStream.push`` takes as they are, and ``Y4MWriter`` takes what ``pop`` returns (``i010`` at 10 bits: little-endian uint16 samples).

The header is ``YUV4MPEG2`` and space-separated tokens up to the newline:

* ``W``, ``H``: the raster, required, both even (4:2:0);
* ``F n:d``: the frame rate, kept verbatim; ``X...``: extensions, kept verbatim, ``XCOLORRANGE=FULL|LIMITED`` setting the range;
* ``I``: ``p`` (progressive) and ``?`` (unknown) are accepted; ``t``, ``b``, ``m`` are refused - the network is no deinterlacer;
* ``A n:d``: the sample aspect ratio, ``0:0`` (unknown) or absent = (1, 1);
* ``C``: absent, ``420jpeg`` and bare ``420`` = chroma sited "center"; ``420mpeg2`` = "left"; ``420paldv`` = "topleft" (pfnl_amd/yuv.py
  SITINGS); any other tag (``422``, ``444``, ``mono``, ...) is a ValueError that names it;
* ``C420p10`` (yuv420p10le) is read where the caller asks for it - ``Y4MReader(f, depths=(8, 10))``; by default it is refused like any
  other tag - and gives ``bits=10``, frames as ``(H*3//2, W)`` little-endian uint16 arrays (the session's ``i010``, taken with
  ``in_depth=10``) and ``siting="left"``: Y4M's 10-bit tag carries no siting, and left is what HEVC / AV1 encoders mean unless told otherwise;
* ``C422``, ``C444``, ``C422p10``, ``C444p10`` are opt-in the same way - ``Y4MReader(f, depths=(8, 10), chromas=("420", "422", "444"))`` - and
  give ``chroma`` "422" | "444" (pfnl_amd/yuv.py CHROMAS): the planes Y [H][W], Cb, Cr [H][W/2] or [H][W], the session's ``i420`` layout at
  that subsampling, frames as ``(2*H, W)`` / ``(3*H, W)`` arrays.  ``C422`` is horizontally co-sited: ``siting="left"``; 4:4:4 has no
  siting and says "left" too.  W is even at 4:2:2 and H anything; a ``C444`` stream may have odd W and H.  The writer adds the ``XYSCSS=``
  token ffmpeg writes beside these tags (``422``, ``444``, ``422P10``, ``444P10``).

Out of scope: mono, 4:1:1 and alpha, 12 and 16 bits, interlaced streams, per-frame parameters (they are read and dropped).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import Iterator, Optional, Tuple

import numpy as np

MAGIC = b"YUV4MPEG2"
MAX_LINE = 4096                                                         # a header or frame line longer than this is not Y4M
SITING_OF_TAG = {"420jpeg": "center", "420": "center", "420mpeg2": "left", "420paldv": "topleft"}
TAG_OF_SITING = {"center": "420jpeg", "left": "420mpeg2", "topleft": "420paldv"}
TAG_10BIT = "420p10"
CHROMAS = ("420", "422", "444")                                         # pfnl_amd/yuv.py CHROMAS
CHROMA_TAGS = {"422": ("422", 8), "444": ("444", 8), "422p10": ("422", 10), "444p10": ("444", 10)}   # tag -> (chroma, bits)
RANGE_KEY = "XCOLORRANGE="


def _ratio(text: str, what: str) -> Tuple[int, int]:
    try:
        n, d = (int(v) for v in text.split(":"))
    except ValueError:
        raise ValueError(f"y4m: {what} is n:d, got {text!r}") from None
    if n < 0 or d < 0:
        raise ValueError(f"y4m: {what} is n:d, got {text!r}")
    return n, d


@dataclass(frozen=True)
class Y4MHeader:
    """One stream's parameters.  ``rate`` and ``interlace`` are the ``F`` and ``I`` tokens' values or None where the stream has none;
    ``extensions`` are the ``X`` tokens verbatim, in order, ``XCOLORRANGE`` among them; ``bits`` is 8, or 10 for a stream the writer makes;
    ``chroma`` is "420", or "422" | "444" for a stream read with ``chromas`` or made by the writer."""
    width: int
    height: int
    rate: Optional[str] = None
    interlace: Optional[str] = None
    sar: Tuple[int, int] = (1, 1)
    siting: str = "center"
    extensions: Tuple[str, ...] = ()
    bits: int = 8
    chroma: str = "420"
    interlaced_ok: bool = field(default=False, compare=False, repr=False)   # ``It`` / ``Ib`` pass: the caller deinterlaces (pfnl_amd/deinterlace.py)

    def __post_init__(self):
        if self.chroma not in CHROMAS:
            raise ValueError(f"y4m: chroma: one of {CHROMAS}, got {self.chroma!r}")
        if self.chroma == "420" and (self.width < 2 or self.height < 2 or self.width % 2 or self.height % 2):
            raise ValueError(f"y4m: W and H must be even and at least 2 (4:2:0), got W{self.width} H{self.height}")
        if self.chroma == "422" and (self.width < 2 or self.height < 1 or self.width % 2):
            raise ValueError(f"y4m: W must be even and at least 2 and H at least 1 (4:2:2), got W{self.width} H{self.height}")
        if self.chroma == "444" and (self.width < 1 or self.height < 1):
            raise ValueError(f"y4m: W and H must be at least 1, got W{self.width} H{self.height}")
        if self.interlace not in (None, "p", "?") and not (self.interlaced_ok and self.interlace in ("t", "b")):
            raise ValueError(f"y4m: interlaced streams are not supported (I{self.interlace}); deinterlace first")
        if self.siting not in TAG_OF_SITING:
            raise ValueError(f"y4m: siting: one of {sorted(TAG_OF_SITING)}, got {self.siting!r}")
        if self.bits not in (8, 10):
            raise ValueError(f"y4m: bits: 8 or 10, got {self.bits!r}")

    @property
    def full_range(self) -> bool:
        """True where the last ``XCOLORRANGE`` token says FULL; limited range otherwise."""
        full = False
        for x in self.extensions:
            if x.startswith(RANGE_KEY):
                full = x[len(RANGE_KEY):] == "FULL"
        return full

    @property
    def frame_samples(self) -> int:
        return self.width * self.height * {"420": 3, "422": 4, "444": 6}[self.chroma] // 2

    @property
    def frame_bytes(self) -> int:
        return self.frame_samples * (2 if self.bits == 10 else 1)

    @classmethod
    def parse(cls, line: bytes, depths: Tuple[int, ...] = (8,), chromas: Tuple[str, ...] = ("420",), interlaced: bool = False) -> "Y4MHeader":
        """The header of its line (without or with the newline).  ``depths``: the sample depths the caller takes; with 10 among them
        ``C420p10`` parses to ``bits=10``, ``siting="left"``.  ``chromas``: the subsamplings the caller takes; with "422" / "444" among
        them ``C422`` / ``C444`` (and, with 10 among ``depths``, ``C422p10`` / ``C444p10``) parse to that ``chroma``, ``siting="left"``.  ``interlaced``: ``It`` / ``Ib`` (top / bottom field first) pass, and ``.interlace`` says
        which; ``Im`` (mixed) is refused either way."""
        try:
            tokens = line.rstrip(b"\n").decode("ascii").split(" ")
        except UnicodeDecodeError:
            raise ValueError("y4m: the header is not ASCII") from None
        if tokens[0] != MAGIC.decode():
            raise ValueError(f"y4m: the stream does not start with {MAGIC.decode()}")
        width = height = None
        rate = interlace = None
        sar, siting, ext, bits, chroma = (1, 1), "center", [], 8, "420"
        for t in tokens[1:]:
            if not t:
                continue
            key, value = t[0], t[1:]
            if key in "WH":
                try:
                    v = int(value)
                except ValueError:
                    raise ValueError(f"y4m: {key} is an integer, got {t!r}") from None
                width, height = (v, height) if key == "W" else (width, v)
            elif key == "F":
                _ratio(value, "F")
                rate = value
            elif key == "I":
                interlace = value
            elif key == "A":
                sar = _ratio(value, "A")
                if sar[0] == 0 or sar[1] == 0:
                    sar = (1, 1)
            elif key == "C" and value == TAG_10BIT and 10 in depths and "420" in chromas:
                siting, bits, chroma = "left", 10, "420"
            elif key == "C" and value in CHROMA_TAGS and CHROMA_TAGS[value][0] in chromas and CHROMA_TAGS[value][1] in depths:
                siting, (chroma, bits) = "left", CHROMA_TAGS[value]
            elif key == "C":
                if value not in SITING_OF_TAG or "420" not in chromas:
                    raise ValueError(f"y4m: chroma format C{value} is not supported (8-bit 4:2:0: {', '.join('C' + k for k in SITING_OF_TAG)})")
                siting, bits, chroma = SITING_OF_TAG[value], 8, "420"
            elif key == "X":
                if t.startswith(RANGE_KEY) and t[len(RANGE_KEY):] not in ("FULL", "LIMITED"):
                    raise ValueError(f"y4m: {RANGE_KEY}FULL or {RANGE_KEY}LIMITED, got {t!r}")
                ext.append(t)
            else:
                raise ValueError(f"y4m: unknown header token {t!r}")
        if width is None or height is None:
            raise ValueError("y4m: the header needs W and H")
        return cls(width, height, rate, interlace, sar, siting, tuple(ext), bits, chroma, bool(interlaced))

    def to_bytes(self) -> bytes:
        """The header line, newline included: W H F I A C, then the extensions."""
        t = [MAGIC.decode(), f"W{self.width}", f"H{self.height}"]
        if self.rate is not None:
            t.append("F" + self.rate)
        if self.interlace is not None:
            t.append("I" + self.interlace)
        t.append(f"A{self.sar[0]}:{self.sar[1]}")
        if self.chroma == "420":
            t.append("C" + (TAG_10BIT if self.bits == 10 else TAG_OF_SITING[self.siting]))
        else:
            t.append("C" + self.chroma + ("p10" if self.bits == 10 else ""))
        t += list(self.extensions)
        return (" ".join(t) + "\n").encode("ascii")

    def for_output(self, width: int, height: int, siting: Optional[str] = None, bits: int = 8, sar: Optional[Tuple[int, int]] = None,
                   full_range: Optional[bool] = None, chroma: Optional[str] = None, progressive: bool = False,
                   double_rate: bool = False, film_rate: bool = False) -> "Y4MHeader":
        """The header of the stream made from this one: the new raster, siting, depth and aspect; ``F``, ``I`` and the extensions pass
        through - but ``XYSCSS``, which restates the chroma format and becomes ``XYSCSS=420P10`` at 10 bits (``422`` / ``444`` /
        ``422P10`` / ``444P10`` for those tags), and the range token where ``full_range`` says otherwise than the stream.  ``chroma`` None:
        this stream's.  ``progressive``: the frames have been deinterlaced, ``I`` becomes ``Ip``; ``double_rate``: at field rate, ``F`` doubles
        its numerator; ``film_rate``: one frame in five has been dropped, ``F`` becomes 4 / 5 of its rational in lowest terms (30000:1001 ->
        24000:1001)."""
        chroma = self.chroma if chroma is None else chroma
        rate = self.rate
        if film_rate and rate is not None:
            num, den = _ratio(rate, "F")
            g = math.gcd(4 * num, 5 * den)
            rate = f"{4 * num // g}:{5 * den // g}"
        if double_rate and rate is not None:
            num, den = _ratio(rate, "F")
            rate = f"{2 * num}:{den}"
        ext = [x for x in self.extensions if not x.startswith("XYSCSS=")]
        if full_range is not None and bool(full_range) != self.full_range:
            ext = [x for x in ext if not x.startswith(RANGE_KEY)] + [RANGE_KEY + ("FULL" if full_range else "LIMITED")]
        if bits == 10 or chroma != "420":
            ext.insert(0, f"XYSCSS={chroma}" + ("P10" if bits == 10 else ""))
        return replace(self, rate=rate, interlace="p" if progressive else self.interlace, width=int(width), height=int(height), siting=self.siting if siting is None else siting, bits=bits, chroma=chroma,
                       sar=self.sar if sar is None else tuple(sar), extensions=tuple(ext))


def _read_exact(f, n: int) -> bytes:
    """Up to n bytes, fewer only at the end of the stream: a pipe returns what it has."""
    parts, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return b"".join(parts)


def _read_line(f) -> bytes:
    """One line without its newline; None at the end of the stream; ValueError where the stream ends inside a line."""
    line = bytearray()
    while True:
        b = f.read(1)
        if not b:
            if line:
                raise ValueError("y4m: the stream ends inside a line")
            return None
        if b == b"\n":
            return bytes(line)
        line += b
        if len(line) > MAX_LINE:
            raise ValueError("y4m: a line without an end: not a Y4M stream")


class Y4MReader:
    """``Y4MReader(fileobj)`` reads the header at once (``.header``); iterating yields every frame as a ``(H*3//2, W)`` uint8 array -
    little-endian uint16 for a ``C420p10`` stream, which ``depths=(8, 10)`` lets through; ``(2*H, W)`` / ``(3*H, W)`` for a ``C422`` /
    ``C444`` stream, which ``chromas=("420", "422", "444")`` lets through.  ``interlaced=True`` lets ``It`` / ``Ib`` streams through - their frames are woven, and
    ``header.interlace`` says which field comes first; so are the frames of film under 3:2 pulldown (pfnl_amd/telecine.py)."""

    def __init__(self, fileobj, depths: Tuple[int, ...] = (8,), chromas: Tuple[str, ...] = ("420",), interlaced: bool = False):
        self._f = fileobj
        line = _read_line(fileobj)
        if line is None:
            raise ValueError("y4m: empty stream")
        self.header = Y4MHeader.parse(line, depths, chromas, interlaced)
        self.frames = 0

    def read_frame(self):
        """The next frame, or None at the end of the stream; ValueError for a bad frame line or a truncated frame."""
        line = _read_line(self._f)
        if line is None:
            return None
        if line != b"FRAME" and not line.startswith(b"FRAME "):
            raise ValueError(f"y4m: frame {self.frames}: expected a FRAME line, got {line[:16]!r}")
        h = self.header
        data = _read_exact(self._f, h.frame_bytes)
        if len(data) != h.frame_bytes:
            raise ValueError(f"y4m: frame {self.frames} is truncated: {len(data)} of {h.frame_bytes} bytes")
        self.frames += 1
        return np.frombuffer(data, "<u2" if h.bits == 10 else np.uint8).reshape(h.frame_samples // h.width, h.width)

    def __iter__(self) -> Iterator[np.ndarray]:
        while True:
            frame = self.read_frame()
            if frame is None:
                return
            yield frame


class Y4MWriter:
    """``Y4MWriter(fileobj, header=None)``: ``write_header`` once (at construction where ``header`` is given), then ``write_frame`` per frame:
    ``(H*3//2, W)`` or flat (2 H W / 3 H W samples under a 4:2:2 / 4:4:4 header), uint8 - uint16 values 0 .. 1023 (``i010``) for a 10-bit
    header, written little-endian."""

    def __init__(self, fileobj, header: Optional[Y4MHeader] = None):
        self._f = fileobj
        self.header = None
        self.frames = 0
        if header is not None:
            self.write_header(header)

    def write_header(self, header: Y4MHeader) -> None:
        if self.header is not None:
            raise ValueError("y4m: the header has been written")
        self._f.write(header.to_bytes())
        self.header = header

    def write_frame(self, frame) -> None:
        h = self.header
        if h is None:
            raise ValueError("y4m: write_header first")
        frame = np.asarray(frame)
        dtype = np.uint16 if h.bits == 10 else np.uint8
        if frame.dtype != dtype or frame.size != h.frame_samples:
            raise ValueError(f"y4m: expected {h.frame_samples} {np.dtype(dtype).name} samples, got {frame.dtype} x {frame.size}")
        self._f.write(b"FRAME\n")
        self._f.write(np.ascontiguousarray(frame).astype("<u2" if h.bits == 10 else np.uint8, copy=False).tobytes())
        self.frames += 1
