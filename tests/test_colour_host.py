"""The colour rule on the host (pfnl_amd/colour.py), the library's integers against it without a device (pfnl_colour_matrix,
pfnl_colour_tables; pfnl_amd/csrc/colour_geom.h as a plain C++ program, once more under ASan + UBSan), and the keywords and flags that
carry a colour description per side to the session."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi, colour, rawvideo, stream, upscale, y4m

PAIRS = [(s, d) for s in colour.PRIMARIES for d in colour.PRIMARIES if s != d]
TOPS = {8: 255, 10: 1023}


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def test_the_two_matrices_identity_and_row_sums():
    assert colour.PRIMARIES == ("bt709", "bt601-525", "bt601-625")
    assert colour.gamut_matrix("bt601-525", "bt709") == ((15394, 822, 168), (291, 15824, 269), (-27, -72, 16483))
    assert colour.gamut_matrix("bt601-625", "bt709") == ((17106, -722, 0), (0, 16384, 0), (0, 193, 16191))
    positive = 0
    for s in colour.PRIMARIES:
        assert colour.gamut_matrix(s, s) == ((16384, 0, 0), (0, 16384, 0), (0, 0, 16384))
        for d in colour.PRIMARIES:
            m = colour.gamut_matrix(s, d)
            assert [sum(row) for row in m] == [16384] * 3, (s, d)
            positive = max(positive, max(sum(v for v in row if v > 0) for row in m))
    assert positive == 18224 and positive * 65535 + (1 << 13) < 2 ** 31       # the sums of coef * D fit in int32
    with pytest.raises(ValueError):
        colour.gamut_matrix("bt2020", "bt709")


@pytest.mark.parametrize("bits,step", [(8, 57), (10, 14)])
def test_the_tables_invert_each_other_and_are_monotone(bits, step):
    D, E = colour.tables(bits)
    top = TOPS[bits]
    assert D.shape == (top + 1,) and E.shape == (65536,) and D.dtype == E.dtype == np.uint16
    assert np.array_equal(E[D], np.arange(top + 1))
    assert (D[0], D[top], E[0], E[65535]) == (0, 65535, 0, top)
    assert np.diff(D.astype(np.int64)).min() == step                        # D's smallest step
    dE = np.diff(E.astype(np.int64))
    assert dE.min() == 0 and dE.max() == 1                                    # monotone, and no code is skipped
    start, threshold, steps = colour.encode_form(bits)
    assert steps == {8: 2, 10: 5}[bits] and start.shape == (1024,) and threshold.shape == (top + 1,)
    assert np.array_equal(colour.encode_lookup(np.arange(65536), bits), E)    # the device's form of E, over every l


@pytest.mark.parametrize("bits", [8, 10])
def test_convert_keeps_every_grey_and_its_input_where_nothing_changes(bits):
    top = TOPS[bits]
    dtype = np.uint8 if bits == 8 else np.uint16
    grey = np.repeat(np.arange(top + 1, dtype=dtype)[:, None], 3, axis=1)
    for s, d in PAIRS:
        assert np.array_equal(colour.convert(grey, s, d, bits), grey), (s, d)
    x = np.random.default_rng(1).integers(0, top + 1, (5, 7, 3)).astype(dtype)
    assert colour.convert(x, "bt601-625", "bt601-625", bits) is x
    with pytest.raises(ValueError):
        colour.convert(x.astype(np.int32), "bt709", "bt601-525", bits)
    with pytest.raises(ValueError):
        colour.convert(x, "bt709", "bt601-525", 12)


@pytest.mark.parametrize("bits", [8, 10])
def test_convert_against_the_chain_in_double_arithmetic(bits):
    """Under 1 code for all six pairs: half a code of output rounding, under 0.1 code from D's rounding through the matrix, and what E's
    own rounding of l adds where the curve is steep.  Measured: at most 0.56 code at 8 bits and 0.76 at 10."""
    top = TOPS[bits]
    x = np.random.default_rng(2024).integers(0, top + 1, (200_000, 3)).astype(np.uint8 if bits == 8 else np.uint16)
    for s, d in PAIRS:
        got = colour.convert(x, s, d, bits)
        assert got.dtype == x.dtype and got.shape == x.shape and int(got.max()) <= top
        err = float(np.abs(got.astype(np.float64) - colour.convert_reference(x, s, d, bits)).max())
        print(f"{bits} bits {s} -> {d}: max |rule - double| = {err:.3f} code")
        assert err < 1.0, (s, d, err)
    # the saturated primaries move, and a gamut that does not hold a colour clips it
    red = np.array([[top, 0, 0]], x.dtype)
    assert not np.array_equal(colour.convert(red, "bt601-525", "bt709", bits), red)
    assert colour.convert(np.array([[0, top, 0]], x.dtype), "bt709", "bt601-525", bits)[0, 0] == 0


# ---- the library without a device -----------------------------------------------------------------------------------------------------------
def test_the_librarys_integers_are_the_rules():
    lib = _capi.load_library()
    out = (C.c_int32 * 9)()
    for si, s in enumerate(colour.PRIMARIES):
        for di, d in enumerate(colour.PRIMARIES):
            assert lib.pfnl_colour_matrix(si, di, out) == 0
            assert tuple(out) == sum(colour.gamut_matrix(s, d), ()), (s, d)
    for bad in ((-1, 0), (0, 3), (3, 3)):
        assert lib.pfnl_colour_matrix(*bad, out) == -1 and b"primaries" in lib.pfnl_last_error()
    assert lib.pfnl_colour_matrix(0, 1, None) == -1 and b"NULL" in lib.pfnl_last_error()
    for bits in (8, 10):
        dec, enc = (C.c_uint16 * (1 << bits))(), (C.c_uint16 * 65536)()
        assert lib.pfnl_colour_tables(bits, dec, enc) == 0
        D, E = colour.tables(bits)
        assert np.array_equal(np.frombuffer(dec, np.uint16), D) and np.array_equal(np.frombuffer(enc, np.uint16), E)
    dec, enc = (C.c_uint16 * 1024)(), (C.c_uint16 * 65536)()
    for bits in (0, 9, 12, 16):
        assert lib.pfnl_colour_tables(bits, dec, enc) == -1 and b"bits" in lib.pfnl_last_error()
    assert lib.pfnl_colour_tables(8, None, enc) == -1 and lib.pfnl_colour_tables(8, dec, None) == -1
    assert lib.pfnl_version() == 4                                           # additions to version 4


def test_the_hooks_and_the_setter_refuse_before_any_hip_call():
    lib = _capi.load_library()
    d = C.c_void_p(64)                                                       # never dereferenced: the hooks return first
    for hook in (lib.pfnl_op_quantise_colour_u8, lib.pfnl_op_quantise_colour_u10):
        assert hook(None, d, 4, 1, 0, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert hook(d, None, 4, 1, 0, None) == -1 and b"NULL" in lib.pfnl_last_error()
        for pixels in (0, 3, 6, 4 * 257 + 1):
            assert hook(d, d, pixels, 1, 0, None) == -1 and b"multiple of 4" in lib.pfnl_last_error()
        assert hook(C.c_void_p(72), d, 4, 1, 0, None) == -1 and b"aligned" in lib.pfnl_last_error()     # sr: 16 bytes
        assert hook(d, C.c_void_p(68), 4, 1, 0, None) == -1 and b"aligned" in lib.pfnl_last_error()     # out: 8 bytes
        for src, dst in ((3, 0), (0, -1), (7, 7)):
            assert hook(d, d, 4, src, dst, None) == -1 and b"primaries" in lib.pfnl_last_error()
    side = _capi.pfnl_colour(0, 0, 1)
    assert lib.pfnl_stream_colour(None, C.byref(side), C.byref(side)) == -1 and b"NULL" in lib.pfnl_last_error()


DRIVER = r"""
#include <cstdio>
#include "colour_geom.h"

int main() {
    for (int s = -1; s <= 3; ++s)
        for (int d = -1; d <= 3; ++d) {
            pfnl::ColourMatrix m;
            if (!pfnl::colour_matrix(s, d, &m)) {
                std::printf("R %d %d\n", s, d);
                continue;
            }
            std::printf("M %d %d", s, d);
            for (int k = 0; k < 9; ++k) std::printf(" %d", m.m[k]);
            std::printf("\n");
        }
    std::printf("T %d %d\n", (int)pfnl::colour_tables(9, nullptr, nullptr), (int)pfnl::colour_blob(12, nullptr));
    for (int bits : {8, 10}) {
        const int levels = 1 << bits;
        std::vector<uint16_t> D(levels), E(pfnl::COLOUR_LINEAR), blob;
        if (!pfnl::colour_tables(bits, D.data(), E.data()) || !pfnl::colour_blob(bits, &blob)) return 1;
        if ((int)blob.size() != pfnl::colour_blob_words(bits)) return 2;
        std::printf("D %d", bits);
        for (uint16_t v : D) std::printf(" %d", v);
        std::printf("\nE %d", bits);
        for (uint16_t v : E) std::printf(" %d", v);
        std::printf("\nB %d", bits);
        for (uint16_t v : blob) std::printf(" %d", v);
        const uint16_t* const start = blob.data() + levels;
        const uint16_t* const threshold = start + pfnl::COLOUR_BUCKETS;
        long wrong = 0;                                 // the kernel's form of E against E, over every l
        for (int l = 0; l < pfnl::COLOUR_LINEAR; ++l)
            wrong += (bits == 8 ? pfnl::encode_lookup<256>(start, threshold, l) : pfnl::encode_lookup<1024>(start, threshold, l)) != E[l];
        std::printf("\nX %d %ld\n", bits, wrong);
    }
    return 0;
}
"""


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("colour")
    src = tmp / "driver.cpp"
    src.write_text(DRIVER)
    texts = []
    for name, flags in (("driver", []), ("driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp / name                                                     # stand-alone host code: the sanitizers need no preload
        subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
        texts.append(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert texts[0] == texts[1]
    out = {}
    for line in texts[0].strip().split("\n"):
        parts = line.split()
        out.setdefault(parts[0], []).append([int(v) for v in parts[1:]])
    return out


def test_colour_geom_holds_the_rules_integers(geom):
    assert len(geom["M"]) == 9 and len(geom["R"]) == 16 and geom["T"] == [[0, 0]]
    for s, d, *m in geom["M"]:
        assert tuple(m) == sum(colour.gamut_matrix(colour.PRIMARIES[s], colour.PRIMARIES[d]), ()), (s, d)
    assert all(s in (-1, 3) or d in (-1, 3) for s, d in geom["R"])
    for key, which in (("D", 0), ("E", 1)):
        assert [row[0] for row in geom[key]] == [8, 10]
        for bits, *values in geom[key]:
            assert np.array_equal(np.array(values), colour.tables(bits)[which]), (key, bits)
    for bits, *values in geom["B"]:
        start, threshold, _ = colour.encode_form(bits)
        assert np.array_equal(np.array(values), np.concatenate([colour.tables(bits)[0], start, threshold])), bits
    assert geom["X"] == [[8, 0], [10, 0]]                                    # the compare loop lands on E[l] for all 65 536 l, at both depths


# ---- keywords and flags -----------------------------------------------------------------------------------------------------------------------
def test_the_keywords_refuse_what_the_library_refuses():
    assert stream.colour_arguments() is None                                 # all defaults: no call
    assert stream.colour_arguments("bt601", True) is None                    # matrix and range alone are pfnl_stream_format's
    assert stream.colour_arguments("bt601", False, "bt709", None, "bt601-525", "bt709") == ((0, 0, 1), (1, 0, 0))
    assert stream.colour_arguments("bt601", True, None, False, "bt709", None) == ((0, 1, 0), (0, 0, 0))
    assert stream.colour_arguments(primaries="bt601-625") == ((1, 0, 2), (1, 0, 2))
    assert stream.colour_arguments(out_primaries="bt709") == ((1, 0, 0), (1, 0, 0))
    for bad in ({"out_matrix": "bt2020"}, {"out_matrix": 1}, {"primaries": "smpte-c"}, {"primaries": None}, {"out_primaries": "bt601"},
                {"out_primaries": 0}, {"out_full_range": "full"}, {"out_full_range": 2}, {"matrix": "bt2020"}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            stream.colour_arguments(**bad)

    class Unready:                                                           # the check comes before anything touches the engine
        pass
    for bad in ({"out_primaries": "ebu"}, {"primaries": "pal"}, {"out_matrix": "bt470"}, {"out_full_range": "limited"}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            stream.VideoStream(Unready(), 16, 24, 2, **bad)
    import inspect

    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.model import PFNL
    for f in (PFNLEngine.open_stream, PFNL.open_stream, stream.VideoStream.__init__):
        p = inspect.signature(f).parameters
        assert [p[k].default for k in ("out_matrix", "out_full_range", "primaries", "out_primaries")] == [None, None, "bt709", None], f


def test_auto_goes_by_the_lines():
    assert [colour.auto_primaries(h) for h in (480, 486, 576, 720, 1080)] == ["bt601-525", "bt601-525", "bt601-625", "bt709", "bt709"]
    assert colour.auto_primaries(240) == "bt709"
    for h, prim in ((480, "bt601-525"), (486, "bt601-525"), (576, "bt601-625"), (720, "bt709"), (1080, "bt709")):
        big = colour.side_keywords(h, 4 * h, upscale.auto_matrix(h), "auto", None, "auto", "auto")
        assert big == {"primaries": prim, "out_matrix": "bt709", "out_primaries": "bt709"}, h
        same = colour.side_keywords(h, 576 if h <= 576 else h, upscale.auto_matrix(h), "auto", "full", "auto", "auto")
        if h <= 576:                                                         # delivered at up to 576 lines: the input's
            assert same == {"primaries": prim, "out_matrix": "bt601", "out_full_range": True, "out_primaries": prim}, h
        else:
            assert same == {"primaries": "bt709", "out_matrix": "bt709", "out_full_range": True, "out_primaries": "bt709"}, h
    assert colour.side_keywords(480, 1920, "bt601") == {}
    assert colour.side_keywords(480, 1920, "bt601", out_primaries="auto") == {"out_primaries": "bt709"}
    assert colour.side_keywords(480, 480, "bt601", out_primaries="auto") == {"out_primaries": "bt709"}       # (an unnamed input is bt709)
    assert colour.side_keywords(480, 1920, "bt601", out_range="limited") == {"out_full_range": False}
    for bad in ({"out_matrix": "bt2020"}, {"out_range": "tv"}, {"primaries": "ntsc"}, {"out_primaries": "bt601"}):
        with pytest.raises(ValueError):
            colour.side_keywords(480, 1920, "bt601", **bad)


def test_session_keywords_with_and_without_the_flags():
    ntsc = y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H480 F30000:1001 Ip A10:11 C420mpeg2")
    plain = upscale.session_keywords(ntsc, batch=2)
    assert plain == {"batch": 2, "out_format": "i420", "matrix": "bt601", "full_range": False, "pixel_format": "i420", "chroma_siting": "left"}
    kw = upscale.session_keywords(ntsc, batch=2, out_matrix="auto", primaries="auto", out_primaries="auto")
    assert kw == dict(plain, primaries="bt601-525", out_matrix="bt709", out_primaries="bt709")              # 1920 lines out
    kw = upscale.session_keywords(ntsc, batch=2, out_matrix="auto", primaries="auto", out_primaries="auto", out_size=(480, 720))
    assert kw == dict(plain, out_size=(480, 720), primaries="bt601-525", out_matrix="bt601", out_primaries="bt601-525")
    kw = upscale.session_keywords(ntsc, out_matrix="auto", out_primaries="auto", scale=1)                   # 480 lines out
    assert (kw["out_matrix"], kw["out_primaries"]) == ("bt601", "bt709") and "scale" not in kw and "primaries" not in kw
    pal = y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H576 F25:1 Ip")
    kw = upscale.session_keywords(pal, primaries="auto", out_range="full", out_primaries="bt709")
    assert (kw["primaries"], kw["out_full_range"], kw["out_primaries"], kw["full_range"]) == ("bt601-625", True, "bt709", False)
    a = upscale.parser().parse_args(["-", "-", "--synthetic-weights", "0"])
    assert (a.out_matrix, a.out_range, a.primaries, a.out_primaries) == (None, None, None, None)
    a = upscale.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--out-matrix", "auto", "--out-range", "full", "--primaries", "auto",
                                     "--out-primaries", "bt709"])
    assert (a.out_matrix, a.out_range, a.primaries, a.out_primaries) == ("auto", "full", "auto", "bt709")
    a = rawvideo.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--in-format", "uyvy422", "--size", "480x720", "--primaries", "bt601-525",
                                      "--out-primaries", "auto"])
    assert (a.out_matrix, a.out_range, a.primaries, a.out_primaries) == (None, None, "bt601-525", "auto")
    with pytest.raises(SystemExit):
        upscale.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--out-matrix", "bt2020"])


class _Stub:
    """a session that hands back one frame per pushed frame and remembers its keywords"""
    made = []

    def __init__(self, H, W, batch, **kw):
        self.kw, self.H, self.W, self.scale, self.out_size, self.out_chroma_siting = kw, H, W, 4, None, kw.get("out_chroma_siting", "left")
        self.count = self.given = 0
        _Stub.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _frames(self, upto):
        out = []
        while self.given < upto:
            out.append((self.given, np.full(self.out_samples, self.given, np.uint8)))
            self.given += 1
        return out

    def push(self, frame):
        self.count += 1
        return self._frames(self.count - 1)

    def end(self):
        return self._frames(self.count)


def test_the_loops_hand_the_named_keys_on_and_the_header_follows_the_output_range():
    H, W, n = 480, 8, 3
    _Stub.out_samples = 16 * H * W * 3 // 2
    src = io.BytesIO()
    wr = y4m.Y4MWriter(src, y4m.Y4MHeader(W, H, "30000:1001", "p"))
    for i in range(n):
        wr.write_frame(np.full(H * W * 3 // 2, i, np.uint8))
    base = {"out_format", "matrix", "full_range", "pixel_format", "chroma_siting"}
    out, log = io.BytesIO(), io.StringIO()
    assert upscale.upscale(y4m.Y4MReader(io.BytesIO(src.getvalue())), y4m.Y4MWriter(out), _Stub, log=log) == n
    assert set(_Stub.made[-1].kw) == base and not y4m.Y4MReader(io.BytesIO(out.getvalue())).header.full_range
    out = io.BytesIO()
    assert upscale.upscale(y4m.Y4MReader(io.BytesIO(src.getvalue())), y4m.Y4MWriter(out), _Stub, log=log, out_matrix="auto", out_range="full",
                           primaries="auto", out_primaries="auto") == n
    kw = _Stub.made[-1].kw
    assert set(kw) == base | {"out_matrix", "out_full_range", "primaries", "out_primaries"}
    assert (kw["matrix"], kw["out_matrix"], kw["full_range"], kw["out_full_range"], kw["primaries"], kw["out_primaries"]) == \
        ("bt601", "bt709", False, True, "bt601-525", "bt709")
    assert y4m.Y4MReader(io.BytesIO(out.getvalue())).header.full_range        # XCOLORRANGE follows the output
    from pfnl_amd import packed as P
    _Stub.out_samples = P.frame_bytes("uyvy422", 4 * H, 4 * W)
    for named in ({}, {"primaries": "auto", "out_matrix": "auto", "out_primaries": "auto"}):
        raw = rawvideo.RawReader(io.BytesIO(bytes(n * P.frame_bytes("uyvy422", H, W))), "uyvy422", H, W)
        assert rawvideo.run(raw, rawvideo.RawWriter(io.BytesIO()), _Stub, matrix="bt601", log=log, **named) == n
        kw = _Stub.made[-1].kw
        assert {k: kw[k] for k in ("primaries", "out_matrix", "out_primaries") if k in kw} == \
            ({"primaries": "bt601-525", "out_matrix": "bt709", "out_primaries": "bt709"} if named else {})
