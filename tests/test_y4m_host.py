"""Y4M streams and the upscale loop, without a device (pfnl_amd/y4m.py, pfnl_amd/upscale.py): headers on literal byte strings, every refusal,
short reads, truncated streams, and ``upscale()`` around a stub session that records its keywords."""
import io

import numpy as np
import pytest

from pfnl_amd import upscale as up
from pfnl_amd import y4m


def _frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)


def _stream(header: bytes, frames, frame_line=b"FRAME\n"):
    return header + b"".join(frame_line + f.tobytes() for f in frames)


# ---- headers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,siting", [(b"", "center"), (b" C420jpeg", "center"), (b" C420", "center"), (b" C420mpeg2", "left"),
                                        (b" C420paldv", "topleft")])
def test_chroma_tags_map_to_sitings(tag, siting):
    h = y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 F30000:1001 Ip A1:1" + tag + b"\n")
    assert (h.width, h.height, h.rate, h.interlace, h.sar, h.siting, h.bits, h.full_range) == (24, 16, "30000:1001", "p", (1, 1), siting, 8, False)
    want = {"center": b"C420jpeg", "left": b"C420mpeg2", "topleft": b"C420paldv"}[siting]
    assert h.to_bytes() == b"YUV4MPEG2 W24 H16 F30000:1001 Ip A1:1 " + want + b"\n"
    assert y4m.Y4MHeader.parse(h.to_bytes()) == h


def test_header_round_trips_on_literal_strings():
    h = y4m.Y4MHeader.parse(b"YUV4MPEG2 W352 H288 F25:1 Ip A0:0 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL XFOO=bar")
    assert h.sar == (1, 1) and h.siting == "left" and h.full_range is True                                  # A0:0 is unknown = square
    assert h.extensions == ("XYSCSS=420MPEG2", "XCOLORRANGE=FULL", "XFOO=bar")                              # verbatim, unknown ones kept
    assert h.to_bytes() == b"YUV4MPEG2 W352 H288 F25:1 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL XFOO=bar\n"
    assert y4m.Y4MHeader.parse(h.to_bytes()) == h
    h = y4m.Y4MHeader.parse(b"YUV4MPEG2 H2 W4\n")                                                          # nothing but the raster, any order
    assert (h.width, h.height, h.rate, h.interlace, h.sar, h.siting, h.extensions) == (4, 2, None, None, (1, 1), "center", ())
    assert h.to_bytes() == b"YUV4MPEG2 W4 H2 A1:1 C420jpeg\n" and h.frame_bytes == 12
    h = y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H576 F25:1 I? A16:15 XCOLORRANGE=LIMITED\n")
    assert h.interlace == "?" and h.sar == (16, 15) and h.full_range is False
    assert h.to_bytes() == b"YUV4MPEG2 W720 H576 F25:1 I? A16:15 C420jpeg XCOLORRANGE=LIMITED\n"


def test_output_headers():
    h = y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 F25:1 Ip A16:15 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED XFOO=1\n")
    assert h.for_output(96, 64).to_bytes() == b"YUV4MPEG2 W96 H64 F25:1 Ip A16:15 C420jpeg XCOLORRANGE=LIMITED XFOO=1\n"
    assert h.for_output(96, 64, siting="topleft", sar=(1, 1)).to_bytes() == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420paldv XCOLORRANGE=LIMITED XFOO=1\n"
    ten = h.for_output(100, 72, bits=10, sar=(1, 1))
    assert ten.to_bytes() == b"YUV4MPEG2 W100 H72 F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED XFOO=1\n"
    assert ten.frame_bytes == 2 * 100 * 72 * 3 // 2
    assert h.for_output(96, 64, full_range=True).to_bytes() == b"YUV4MPEG2 W96 H64 F25:1 Ip A16:15 C420jpeg XFOO=1 XCOLORRANGE=FULL\n"
    assert h.for_output(96, 64, full_range=False).extensions == ("XCOLORRANGE=LIMITED", "XFOO=1")


@pytest.mark.parametrize("line,word", [
    (b"YUV4MPEG W24 H16\n", "YUV4MPEG2"), (b"RIFF W24 H16\n", "YUV4MPEG2"), (b"YUV4MPEG2 W24\n", "W and H"), (b"YUV4MPEG2 H16\n", "W and H"),
    (b"YUV4MPEG2 W23 H16\n", "even"), (b"YUV4MPEG2 W24 H15\n", "even"), (b"YUV4MPEG2 W0 H16\n", "even"), (b"YUV4MPEG2 Wx H16\n", "integer"),
    (b"YUV4MPEG2 W24 H16 It\n", "It"), (b"YUV4MPEG2 W24 H16 Ib\n", "Ib"), (b"YUV4MPEG2 W24 H16 Im\n", "Im"),
    (b"YUV4MPEG2 W24 H16 C422\n", "C422"), (b"YUV4MPEG2 W24 H16 C444\n", "C444"), (b"YUV4MPEG2 W24 H16 Cmono\n", "Cmono"),
    (b"YUV4MPEG2 W24 H16 C420p10\n", "C420p10"), (b"YUV4MPEG2 W24 H16 C411\n", "C411"), (b"YUV4MPEG2 W24 H16 A4-3\n", "A"),
    (b"YUV4MPEG2 W24 H16 F25\n", "F"), (b"YUV4MPEG2 W24 H16 XCOLORRANGE=WIDE\n", "XCOLORRANGE"), (b"YUV4MPEG2 W24 H16 Q7\n", "Q7"),
    (b"YUV4MPEG2 W24 H16 C420jp\xffg\n", "ASCII")])
def test_header_refusals(line, word):
    with pytest.raises(ValueError, match=word):
        y4m.Y4MHeader.parse(line)
    with pytest.raises(ValueError, match=word):
        y4m.Y4MReader(io.BytesIO(line))


def test_stream_refusals():
    with pytest.raises(ValueError, match="empty"):
        y4m.Y4MReader(io.BytesIO(b""))
    with pytest.raises(ValueError, match="inside a line"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W24 H16"))                     # no newline
    with pytest.raises(ValueError, match="without an end"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 " + b"X" * 10000))
    head = b"YUV4MPEG2 W4 H2\n"
    f = _frame(2, 4, 0)
    for bad in (b"FRAMES\n", b"frame\n", b"\n", b"FRAMEx\n"):
        r = y4m.Y4MReader(io.BytesIO(_stream(head, [f]) + bad + f.tobytes()))
        assert np.array_equal(r.read_frame(), f)
        with pytest.raises(ValueError, match="FRAME"):
            r.read_frame()
    for cut in (1, 5, 6, 7, 17):                                             # inside the FRAME line, at its end, inside the planes
        r = y4m.Y4MReader(io.BytesIO(_stream(head, [f, f])[:len(head) + 18 + cut]))
        assert np.array_equal(r.read_frame(), f)
        with pytest.raises(ValueError, match="truncated|inside a line"):
            r.read_frame()
    r = y4m.Y4MReader(io.BytesIO(_stream(head, [f, f], b"FRAME Ip X1\n")))    # frame parameters are read and dropped
    assert len(list(r)) == 2 and r.frames == 2 and r.read_frame() is None
    w = y4m.Y4MWriter(io.BytesIO())
    with pytest.raises(ValueError, match="write_header"):
        w.write_frame(f)
    w.write_header(r.header)
    with pytest.raises(ValueError, match="written"):
        w.write_header(r.header)
    for bad in (f[:-1], f.astype(np.uint16), np.zeros((3, 5), np.uint8)):
        with pytest.raises(ValueError, match="expected"):
            w.write_frame(bad)


class _OneByte:
    """a pipe at its worst: every read returns one byte at the most"""

    def __init__(self, data):
        self._f = io.BytesIO(data)
        self.reads = 0

    def read(self, n=-1):
        self.reads += 1
        return self._f.read(min(n, 1) if n > 0 else 1)


def test_short_reads_and_the_writer_round_trip():
    H, W = 6, 10
    head = b"YUV4MPEG2 W10 H6 F24:1 Ip A1:1 C420paldv\n"
    frames = [_frame(H, W, k) for k in range(3)]
    data = _stream(head, frames)
    r = y4m.Y4MReader(_OneByte(data))
    got = list(r)
    assert r.header.siting == "topleft" and len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, frames))
    assert all(g.shape == (H * 3 // 2, W) and g.dtype == np.uint8 for g in got)
    out = io.BytesIO()
    w = y4m.Y4MWriter(out, r.header)
    for g in got:
        w.write_frame(g.reshape(-1))                                         # flat frames are frames too
    assert out.getvalue() == data and w.frames == 3
    out = io.BytesIO()                                                       # 10 bits: little-endian samples whatever the array's order
    w = y4m.Y4MWriter(out, r.header.for_output(W, H, bits=10))
    f10 = np.random.default_rng(5).integers(0, 1024, (H * 3 // 2, W)).astype(np.uint16)
    w.write_frame(f10)
    body = out.getvalue().split(b"\n", 1)[1]
    assert body == b"FRAME\n" + f10.astype("<u2").tobytes() and len(body) == 6 + 2 * f10.size


# ---- the loop, around a stub session -------------------------------------------------------------------------------------------------------
class _StubStream:
    """nearest-neighbour 4 x of every plane, delivered ``batch`` frames late; records what open_stream was given"""
    scale = 4

    def __init__(self, log, H, W, batch=1, **kw):
        log.append(dict(kw, H=H, W=W, batch=batch))
        self.H, self.W, self.batch, self.kw = H, W, batch, kw
        self.out_size = tuple(kw["out_size"]) if kw.get("out_size") is not None else None
        self.out_chroma_siting = kw.get("out_chroma_siting") or kw["chroma_siting"]
        self.held, self.pushed, self.tiling, self.closed = [], 0, None, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.closed = True

    def set_tiling(self, *t):
        self.tiling = t

    def _sr(self, frame):
        assert frame.dtype == np.uint8 and frame.shape == (self.H * 3 // 2, self.W)
        H, W = self.H, self.W
        flat = frame.reshape(-1)
        planes = [flat[:H * W].reshape(H, W), flat[H * W:H * W * 5 // 4].reshape(H // 2, W // 2), flat[H * W * 5 // 4:].reshape(H // 2, W // 2)]
        big = np.concatenate([np.repeat(np.repeat(p, 4, 0), 4, 1).reshape(-1) for p in planes]).reshape(4 * H * 3 // 2, 4 * W)
        return big.astype(np.uint16) * 4 if self.kw["out_format"] == "i010" else big

    def push(self, frame):
        self.held.append((self.pushed, self._sr(frame)))
        self.pushed += 1
        due, self.held = self.held[:-self.batch], self.held[-self.batch:]
        return due

    def end(self):
        due, self.held = self.held, []
        return due


def _run(head, frames, **kw):
    log, out, err = [], io.BytesIO(), io.StringIO()
    made = []

    def open_stream(H, W, batch=1, **k):
        made.append(_StubStream(log, H, W, batch, **k))
        return made[-1]

    n = up.upscale(y4m.Y4MReader(io.BytesIO(_stream(head, frames))), y4m.Y4MWriter(out), open_stream, log=err, **kw)
    assert n == len(frames) and made[0].closed
    return log[0], out.getvalue(), err.getvalue(), made[0]


def test_upscale_derives_the_session_from_the_header():
    H, W = 16, 24
    frames = [_frame(H, W, k) for k in range(5)]
    kw, data, err, vs = _run(b"YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL XFOO=1\n", frames, batch=2)
    assert kw == {"H": 16, "W": 24, "batch": 2, "pixel_format": "i420", "out_format": "i420", "chroma_siting": "center", "matrix": "bt601",
                  "full_range": True}                                        # (no sar without fit, nothing that was not asked for)
    head, body = data.split(b"\n", 1)
    assert head == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL XFOO=1"
    want = b"".join(b"FRAME\n" + vs._sr(f).tobytes() for f in frames)       # index order, the session's bytes
    assert body == want and len(body) == 5 * (6 + 96 * 64 * 3 // 2)
    assert err.startswith("pfnl_amd.upscale: 5 frames in ") and err.rstrip().endswith("fps)") and err.count("\n") == 1
    back = y4m.Y4MReader(io.BytesIO(data))                                   # and what was written is a stream again
    assert (back.header.width, back.header.height, back.header.siting) == (96, 64, "center") and len(list(back)) == 5


def test_upscale_keywords_10_bits_fit_siting_and_tiles():
    H, W = 16, 24
    frames = [_frame(H, W, 10 + k) for k in range(3)]
    kw, data, _, vs = _run(b"YUV4MPEG2 W24 H16 F30:1 A16:15 C420mpeg2\n", frames, batch=4, out_format="i010", out_size=(64, 96), fit="contain",
                           out_chroma_siting="topleft", matrix="bt709", scene_cut=12.0, ensemble=2, tile=(16, 16, 6))
    assert kw == {"H": 16, "W": 24, "batch": 4, "pixel_format": "i420", "out_format": "i010", "chroma_siting": "left",
                  "out_chroma_siting": "topleft", "matrix": "bt709", "full_range": False, "out_size": (64, 96), "fit": "contain", "sar": (16, 15),
                  "scene_cut": 12.0, "ensemble": 2}
    assert vs.tiling == (16, 16, 6)
    head, body = data.split(b"\n", 1)
    assert head == b"YUV4MPEG2 W96 H64 F30:1 A1:1 C420p10 XYSCSS=420P10"     # fit resolved the aspect: square pixels out
    assert body == b"".join(b"FRAME\n" + vs._sr(f).astype("<u2").tobytes() for f in frames)
    # the matrix a stream does not name: by its height; --full-range overrides a limited header, never the other way
    assert _run(b"YUV4MPEG2 W24 H16\n", frames)[0]["matrix"] == "bt601" and up.auto_matrix(576) == "bt601" and up.auto_matrix(578) == "bt709"
    assert _run(b"YUV4MPEG2 W24 H16 XCOLORRANGE=LIMITED\n", frames, full_range=True)[0]["full_range"] is True
    assert _run(b"YUV4MPEG2 W24 H16 XCOLORRANGE=LIMITED\n", frames, full_range=True)[1].startswith(b"YUV4MPEG2 W96 H64 A1:1 C420jpeg XCOLORRANGE=FULL\n")
    assert _run(b"YUV4MPEG2 W24 H16 XCOLORRANGE=FULL\n", frames, full_range=False)[0]["full_range"] is True
    assert _run(b"YUV4MPEG2 W24 H16 A16:15\n", frames)[1].startswith(b"YUV4MPEG2 W96 H64 A16:15 C420jpeg\n")   # no fit: the input's aspect
    for bad in ({"out_format": "nv12"}, {"out_format": "rgb24"}, {"pixel_format": "nv12"}, {"chroma_siting": "left"}, {"sar": (1, 1)}):
        with pytest.raises(ValueError):
            _run(b"YUV4MPEG2 W24 H16\n", frames, **bad)


def test_command_line_arguments_and_failures(tmp_path, capsys):
    a = up.parser().parse_args(["in.y4m", "-", "--synthetic-weights", "3", "--num-block", "1", "--bits", "10", "--out-size", "72x100", "--fit",
                                "contain", "--tile", "16,16,6,2", "--scene-cut", "9.5", "--out-siting", "left", "--batch", "2", "--ensemble", "4",
                                "--matrix", "bt601", "--full-range", "--precision", "bf16"])
    assert (a.input, a.output, a.synthetic_weights, a.checkpoint, a.num_block, a.bits, a.out_size, a.fit, a.tile, a.scene_cut, a.out_siting,
            a.batch, a.ensemble, a.matrix, a.full_range, a.precision) == ("in.y4m", "-", 3, None, 1, 10, (72, 100), "contain", (16, 16, 6, 2), 9.5,
                                                                         "left", 2, 4, "bt601", True, "bf16")
    for bad in (["a", "b"], ["a", "b", "--checkpoint", "d", "--synthetic-weights", "0"], ["a", "b", "--synthetic-weights", "0", "--bits", "12"],
                ["a", "b", "--synthetic-weights", "0", "--out-size", "72"], ["a", "b", "--synthetic-weights", "0", "--tile", "16"],
                ["a", "b", "--synthetic-weights", "0", "--out-siting", "centre"], ["a", "b", "--synthetic-weights", "0", "--scene-cut", "manual"]):
        with pytest.raises(SystemExit):
            up.parser().parse_args(bad)
    capsys.readouterr()
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 W24 H16 C422\n")                             # a ValueError ahead of any engine: status 1 and the message
    assert up.main([str(src), str(tmp_path / "out.y4m"), "--synthetic-weights", "0", "--num-block", "1"]) == 1
    assert "C422" in capsys.readouterr().err
