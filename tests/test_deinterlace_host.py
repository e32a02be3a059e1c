"""Interlaced input, the host side (pfnl_amd/deinterlace.py; pfnl_amd/csrc/field_geom.h): known answers of the rule, the index replacement,
the rule against a per-sample loop, decode_fields against the decoders the project pins, the generator of the GPU tests, field_geom.h as
a plain C++ program (and once more under AddressSanitizer and UBSan) against the Python rule and a Python model of the session's bound,
the Y4M header, the two command-line loops around a stub session, and the op hooks' refusals without a device."""
import ctypes as C
import io
import os
import shutil
import subprocess
from collections import deque

import numpy as np
import pytest

import deint_gen
from conftest import ROOT
from pfnl_amd import _capi, deinterlace as D, depth10, rawvideo, stream, surface, upscale, y4m, yuv
from pfnl_amd import packed as P


def _col(*v):
    return np.array(v, np.int32).reshape(-1, 1, 1)


# ---- known answers --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("rate", D.RATES)
@pytest.mark.parametrize("order", D.FIELD_ORDERS)
def test_a_static_sequence_is_its_weave(n, rate, order):
    frame = np.random.default_rng(3).integers(0, 256, (8, 6, 3)).astype(np.uint8)
    out = D.frames([frame] * n, order, rate)
    assert len(out) == (n if rate == "frame" else 2 * n)
    assert all(o.dtype == np.uint8 and np.array_equal(o, frame) for o in out)
    ten = (frame.astype(np.uint16) * 4 + 3)
    assert all(o.dtype == np.uint16 and np.array_equal(o, ten) for o in D.frames([ten] * n, order, rate, 1023))


def test_a_one_frame_sequence_is_its_own_weave():
    frame = deint_gen.woven_rgb(2, 8, 6)[1]                             # the 0 / MAX blocks: nothing static about it
    assert D.neighbours(0, 2) == (0, 1, 1, 0) and D.neighbours(1, 2) == (1, 0, 0, 1)
    for rate in D.RATES:
        assert all(np.array_equal(o, frame) for o in D.frames([frame], "bff", rate))


def test_a_moving_ramp_gives_the_cubic():
    """A vertical ramp of 10 per frame row moving down one frame row per field: field k (parity k & 1, tff) holds 10 (2 i + p - k) + 100.
    At field 2 (top) the missing row 2 j + 1 lies between A[j] = 20 j + 80 and A[j + 1]: the cubic of a ramp is its midpoint, 20 j + 90,
    and the clamp - d = mean of P1[j] = 20 j + 100 and N1[j] = 20 j + 80, diff = 10 from each of the three terms - lets it through."""
    h = 6
    field = lambda k: _col(*[10 * (2 * i + (k & 1) - k) + 100 for i in range(h)])   # noqa: E731
    out = D.interpolate(field(0), field(1), field(2), field(3), field(4), 0)[:, 0, 0]
    assert list(out[0::2]) == [20 * i + 80 for i in range(h)]
    assert list(out[3:8:2]) == [20 * j + 90 for j in (1, 2, 3)]         # inside: c + e = cc + ee = 40 j + 180: (8 (c + e) + 8) >> 4
    # row 1: cc clamps onto A[0]: 80 80 100 120 -> (9 * 180 - 200 + 8) >> 4 = 89; d = (100 + 80 + 1) >> 1 = 90, t0 = 10: [80, 100] holds it
    # row 9: ee clamps onto A[5]: 140 160 180 180 -> (9 * 340 - 320 + 8) >> 4 = 171; d = 170, diff = 10
    # row 11: e and ee clamp: 160 180 180 180 -> (9 * 360 - 340 + 8) >> 4 = 181; d = (200 + 180 + 1) >> 1 = 190, t0 = 10,
    # t1 = (|200 - 180| + |200 - 180| + 1) >> 1 = 20 (P2[u + 1] clamps as well): [170, 210] holds it
    assert (out[1], out[9], out[11]) == (89, 171, 181)
    t = D.branches(field(0), field(1), field(2), field(3), field(4), 0)
    assert t["inside"] == h and t["below"] == t["above"] == 0


def test_the_cubic_clips_and_the_clamp_fires():
    z = _col(0, 0, 0, 0)
    # numerator below 0: A = 255 0 0 255, u = 1: 9 (0 + 0) - 510 + 8 = -502 -> -32 -> 0; nothing else moves: out = d = 0
    a = _col(255, 0, 0, 255)
    assert D.interpolate(a, z, a, z, a, 0)[3, 0, 0] == 0 and D.branches(a, z, a, z, a, 0)["clip_low"] == 1
    # ... and, with room around d (x = 40, y = 0: d = 20, diff = 20), still 0: the clip, not the clamp
    assert D.interpolate(a, _col(0, 40, 0, 0), a, z, a, 0)[3, 0, 0] == 0
    # above MAX: A = 0 255 255 0: 9 * 510 + 8 = 4598 -> 287 -> 255; P1 = N1 = 255 there: out = 255
    b, f = _col(0, 255, 255, 0), _col(0, 255, 0, 0)
    assert D.interpolate(b, f, b, f, b, 0)[3, 0, 0] == 255 and D.branches(b, f, b, f, b, 0)["clip_high"] == 1
    b10, f10 = b * 1023 // 255, f * 1023 // 255
    assert D.interpolate(b10, f10, b10, f10, b10, 0, 1023)[3, 0, 0] == 1023 and D.branches(b10, f10, b10, f10, b10, 0, 1023)["clip_high"] == 1
    # the clamp: A flat 100 (s = 100); x = 10, y = 30: d = 20, t0 = 20 -> diff = 10: s above -> 30; x = 200, y = 220: d = 210 -> 200
    flat = _col(100, 100, 100, 100)
    assert D.interpolate(flat, _col(10, 10, 10, 10), flat, _col(30, 30, 30, 30), flat, 0)[1, 0, 0] == 30
    assert D.interpolate(flat, _col(200, 200, 200, 200), flat, _col(220, 220, 220, 220), flat, 0)[1, 0, 0] == 200
    # a same-parity difference widens it: P2 = 60 (t1 = 40): [20 - 40, 20 + 40] holds... 60 is the bound: out = 60
    assert D.interpolate(_col(60, 60, 60, 60), _col(10, 10, 10, 10), flat, _col(30, 30, 30, 30), flat, 0)[1, 0, 0] == 60
    # at 10 bits a sample above 1023 is 1023
    hot = np.full((2, 1, 1), 65535, np.uint16)
    assert (D.interpolate(hot, hot, hot, hot, hot, 1, 1023) == 1023).all()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_index_replacement_at_both_ends(n):
    nf = 2 * n
    for q in range(-2, nf + 2):
        r = D.replace(q, nf)
        assert 0 <= r < nf and (r - q) % 2 == 0 and abs(r - q) in (0, 2)
        assert r == (q if 0 <= q < nf else (q + 2 if q < 0 else q - 2))
    assert D.neighbours(0, nf)[:2] == (0, 1) and D.neighbours(nf - 1, nf)[2:] == (nf - 2, nf - 1)
    for order, first in (("tff", 0), ("bff", 1)):
        assert D.field_sequence(n, order) == [(k // 2, (k & 1) ^ first) for k in range(nf)]
    with pytest.raises(ValueError):
        D.replace(-3, nf)


def _brute(p2, p1, a, n1, n2, p, maxv):
    h = a.shape[0]
    out = np.zeros((2 * h,) + a.shape[1:], np.int64)
    clamp = lambda i: min(max(i, 0), h - 1)                             # noqa: E731
    v = lambda f, i, idx: min(int(f[(clamp(i),) + idx]), maxv)          # noqa: E731
    for idx in np.ndindex(a.shape[1:]):
        for i in range(h):
            out[(2 * i + p,) + idx] = v(a, i, idx)
        for j in range(h):
            u = j - p
            c, e, cc, ee = v(a, u, idx), v(a, u + 1, idx), v(a, u - 1, idx), v(a, u + 2, idx)
            s = min(max((9 * (c + e) - (cc + ee) + 8) >> 4, 0), maxv)
            x, y = v(p1, j, idx), v(n1, j, idx)
            d = (x + y + 1) >> 1
            t1 = (abs(v(p2, u, idx) - c) + abs(v(p2, u + 1, idx) - e) + 1) >> 1
            t2 = (abs(v(n2, u, idx) - c) + abs(v(n2, u + 1, idx) - e) + 1) >> 1
            diff = max((abs(x - y) + 1) >> 1, t1, t2)
            out[(2 * j + 1 - p,) + idx] = min(max(s, d - diff), d + diff)
    return out


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", deint_gen.SHAPES)
def test_the_rule_equals_a_per_sample_loop(h, w, maxv):
    for order in D.FIELD_ORDERS:
        seq = D.sequence_fields(deint_gen.woven_rgb(4, h, w, maxv), order)
        for k in range(len(seq)):
            nb = D.neighbours(k, len(seq))
            args = (seq[nb[0]][0], seq[nb[1]][0], seq[k][0], seq[nb[2]][0], seq[nb[3]][0], seq[k][1], maxv)
            assert np.array_equal(D.interpolate(*args), _brute(*args)), (h, w, maxv, order, k)


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", deint_gen.SHAPES)
def test_the_generator_reaches_every_case(h, w, maxv):
    frames = deint_gen.woven_rgb(5, h, w, maxv, deint_gen.SEED)
    assert np.array_equal(frames[2], frames[1]) and set(np.unique(frames[-1])) == {0, maxv}
    for order in D.FIELD_ORDERS:
        counts = deint_gen.branch_counts(frames, order, maxv)
        assert set(counts) == set(D.BRANCHES) and all(v > 0 for v in counts.values()), counts


# ---- decoding a pushed frame ----------------------------------------------------------------------------------------------------------------
def _rgb(h, w, maxv=255, seed=5):
    return np.random.default_rng(seed).integers(0, maxv + 1, (h, w, 3)).astype(np.uint8 if maxv == 255 else np.uint16)


def test_decode_fields_equals_decoding_the_woven_frame_where_no_row_is_filtered():
    h, w = 8, 12
    rgb, rgb10 = _rgb(h, w), _rgb(h, w, 1023)
    assert np.array_equal(D.decode_fields(rgb, "rgb24", h, w), rgb)
    hot = rgb10.copy()
    hot[0, 0, 0] = 4000
    assert np.array_equal(D.decode_fields(hot, "rgb24", h, w, in_depth=10), np.minimum(hot, 1023))
    for fmt in yuv.FORMATS:
        for chroma in ("422", "444"):
            for siting in ("left", "center"):
                f = yuv.from_rgb(rgb, fmt, "bt601", True, siting, chroma)
                assert np.array_equal(D.decode_fields(f, fmt, h, w, chroma=chroma, matrix="bt601", full_range=True, siting=siting),
                                      yuv.to_rgb(f, fmt, h, w, "bt601", True, siting, chroma))
                f10 = depth10.from_rgb10(rgb10, "p010" if fmt == "nv12" else "i010", "bt709", False, siting, chroma)
                assert np.array_equal(D.decode_fields(f10, fmt, h, w, in_depth=10, chroma=chroma, siting=siting),
                                      depth10.to_rgb10(f10, "p010" if fmt == "nv12" else "i010", h, w, "bt709", False, siting, chroma))
    for name in P.PACKINGS[1:]:
        src = rgb10 if P.bits(name) == 10 else rgb
        f = P.from_rgb(src, name, "bt709", False, "center")
        kw = {"pixel_format": "nv12" if P.is_yuv(name) else "rgb24", "in_depth": P.bits(name), "chroma": "422" if P.is_yuv(name) else "420"}
        assert np.array_equal(D.decode_fields(f, kw.pop("pixel_format"), h, w, packing=name, siting="center", **kw), P.to_rgb(f, name, h, w, "bt709", False, "center"))


def test_decode_fields_at_420_is_to_rgb_of_each_fields_planes():
    h, w = 8, 12
    rgb = deint_gen.woven_rgb(2, h, w)[0]
    for fmt in yuv.FORMATS:
        for siting in yuv.SITINGS:
            f = yuv.from_rgb(rgb, fmt, "bt709", False, siting)
            Y, Cb, Cr = yuv.planes(f, fmt, h, w)
            got = D.decode_fields(f, fmt, h, w, siting=siting)
            for p in (0, 1):
                field = yuv.pack(Y[p::2], Cb[p::2], Cr[p::2], fmt)
                assert np.array_equal(got[p::2], yuv.to_rgb(field, fmt, h // 2, w, "bt709", False, siting))
            assert not np.array_equal(got, yuv.to_rgb(f, fmt, h, w, "bt709", False, siting))   # (the one input where the fields matter)
    f10 = depth10.from_rgb10(deint_gen.woven_rgb(2, h, w, 1023)[0], "p010")
    Y, Cb, Cr = depth10.planes10(f10, "p010", h, w)
    got = D.decode_fields(f10, "nv12", h, w, in_depth=10)
    for p in (0, 1):
        assert np.array_equal(got[p::2], depth10.to_rgb10(depth10.pack10(Y[p::2], Cb[p::2], Cr[p::2], "p010"), "p010", h // 2, w))
    with pytest.raises(ValueError, match="multiple of 4"):
        D.decode_fields(np.zeros(6 * 4 * 3 // 2, np.uint8), "i420", 6, 4)
    with pytest.raises(ValueError):
        D.decode_fields(np.zeros((5, 4, 3), np.uint8), "rgb24", 5, 4)


def test_the_keywords_of_open_stream():
    assert stream.interlace_arguments() == (0, 0)
    assert stream.interlace_arguments("frame", "tff") == (1, 0) and stream.interlace_arguments("field", "bff") == (2, 1)
    assert stream.interlace_arguments("field", "tff", 18, "i420", "422") == (2, 0)
    assert stream.interlace_arguments("field", "tff", 18, "nv12", "420", "yuyv422") == (2, 0)
    assert stream.interlace_arguments(None, "tff", 18, "i420") == (0, 0)
    for bad in (("both",), (True,), ("frame", "top"), ("frame", "tff", 18, "i420"), ("frame", "tff", 18, "nv12", "420")):
        with pytest.raises(ValueError):
            stream.interlace_arguments(*bad)
    with pytest.raises(ValueError):                                      # checked before the engine is touched: this one has none
        stream.VideoStream(None, 16, 24, 1, interlaced="sometimes")


# ---- field_geom.h as a plain C++ program ----------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <deque>
#include <utility>
#include "field_geom.h"
#include "surface_geom.h"
static unsigned long long lcg = 12345;
static unsigned rnd() { lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(lcg >> 33); }
int main() {
    std::printf("K | %d %d\n", pfnl::DEINT_STRIP_PAIRS, pfnl::DEINT_STRIP_ROWS);
    for (int n = 1; n <= 3; ++n)
        for (long long q = -2; q <= 2 * n + 1; ++q) std::printf("R %d %lld | %lld\n", n, q, pfnl::field_replace(q, 2 * n));
    for (int order = 0; order <= 1; ++order)
        for (long long k = 0; k < 6; ++k) std::printf("F %d %lld | %lld %d\n", order, k, pfnl::field_frame(k), pfnl::field_parity(k, order));
    // field surfaces: every format at every chroma format, every packing, tight and pitched
    const int H = 8, W = 12;
    for (int fmt = 0; fmt <= 5; ++fmt)
        for (int chroma = 0; chroma <= 2; ++chroma)
            for (int pack = 0; pack <= 9; ++pack)
                for (int extra = 0; extra <= 40; extra += 40) {
                    const pfnl::SurfaceGeom g = pfnl::surface_geom(fmt, H, W, chroma, pack);
                    if (!g.planes) continue;
                    pfnl_surface sf{};
                    for (int k = 0; k < g.planes; ++k) sf.plane[k] = reinterpret_cast<void*>((uintptr_t)4096 * (k + 1)), sf.pitch[k] = g.plane[k].row_bytes + extra;
                    for (int p = 0; p <= 1; ++p) {
                        const pfnl_surface f = pfnl::field_surface(sf, g.planes, p);
                        std::printf("S %d %d %d %d %d | %d", fmt, chroma, pack, extra, p, g.planes);
                        for (int k = 0; k < g.planes; ++k)
                            std::printf(" %zu %zu %d %zu", (size_t)(reinterpret_cast<uintptr_t>(f.plane[k]) - (uintptr_t)4096 * (k + 1)), f.pitch[k], g.plane[k].rows / 2,
                                        g.plane[k].row_bytes);
                        std::printf("\n");
                    }
                }
    for (int mode = -1; mode <= 3; ++mode)
        for (int order = -1; order <= 2; ++order)
            for (int h = 16; h <= 18; ++h)
                for (int yuv = 0; yuv <= 1; ++yuv)
                    for (int chroma = 0; chroma <= 2; ++chroma)
                        for (int pack = 0; pack <= 4; pack += 4) {
                            const char* why = pfnl::interlace_refused(mode, order, h, yuv != 0, chroma, pack);
                            std::printf("X %d %d %d %d %d %d | %s\n", mode, order, h, yuv, chroma, pack, why ? why : "ok");
                        }
    // a simulated session: woven pushes, pops and the end, in random order; the bound once per ring frame
    for (int T = 3; T <= 7; T += 4)
        for (int batch = 1; batch <= 3; ++batch)
            for (int mode = 1; mode <= 2; ++mode)
                for (int round = 0; round < 6; ++round) {
                    const int cap = 3 * batch + T - 2;
                    pfnl::RingCounters c{0, 0, 0, 0, 0};
                    long long woven = 0;
                    std::printf("C %d %d %d |", T, batch, mode);
                    const int ops = 20 + (int)(rnd() % 60);
                    for (int i = 0; i < ops; ++i) {
                        if (rnd() % 3) {
                            const bool ok = pfnl::ring_admit_all(T, batch, cap, woven ? pfnl::interlace_yield(mode) : 0, &c);
                            if (ok) ++woven;
                            std::printf(" u%d:%lld:%lld:%lld:%d", (int)ok, c.pushed, c.launched, c.delivered, c.in_flight);
                        } else {
                            const bool got = c.in_flight > 0;
                            if (got && ++c.delivered == c.oldest + batch) {          // the front batch is delivered: its slot is free, pump
                                --c.in_flight;
                                c.oldest += batch;
                                while (c.in_flight < 2 && pfnl::ring_next_batch(T, batch, c.pushed, c.launched)) {
                                    if (!c.in_flight) c.oldest = c.launched;
                                    c.launched += batch;
                                    ++c.in_flight;
                                }
                            }
                            std::printf(" o%d:%lld:%lld:%lld:%d", (int)got, c.pushed, c.launched, c.delivered, c.in_flight);
                        }
                    }
                    const bool ok = pfnl::ring_admit_all(T, batch, cap, woven ? pfnl::interlace_yield(mode) : 0, &c);
                    std::printf(" e%d:%lld:%lld:%lld:%d\n", (int)ok, c.pushed, c.launched, c.delivered, c.in_flight);
                }
    return 0;
}
"""


def _cxx():
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build's own clang++ is the last candidate)"
    return cxx


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deinterlace")
    src = tmp / "driver.cpp"
    src.write_text(DRIVER)
    texts = []
    for name, flags in (("driver", []), ("driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp / name                                                 # stand-alone host code: the sanitizers need no preload
        subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
        texts.append(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert texts[0] == texts[1]
    out = {}
    for line in texts[0].strip().split("\n"):
        head, _, rest = line.partition("|")
        out.setdefault(head[0], []).append((head[1:].split(), rest.split()))
    return out


def test_field_geom_replaces_indices_as_the_rule_does(geom):
    assert geom["K"] == [([], [str(C_STRIP // 2), str(C_STRIP)])]
    seen = 0
    for (n, q), (r,) in geom["R"]:
        assert int(r) == D.replace(int(q), 2 * int(n))
        seen += 1
    assert seen == sum(2 * n + 4 for n in (1, 2, 3))
    for (order, k), (frame, parity) in geom["F"]:
        assert (int(frame), int(parity)) == D.field_sequence(3, D.FIELD_ORDERS[int(order)])[int(k)]


C_STRIP = 4                                                              # ops.DEINTERLACE_STRIP_ROWS, stated again where no torch is needed
FMT_NAMES = ("rgb24", "nv12", "i420", "rgb10", "p010", "i010")


def test_field_surfaces_are_the_rows_of_the_rule(geom):
    """field_surface's (offset, pitch, rows, row bytes) per plane, walked over real pitched buffers, against deinterlace.field_frames"""
    from pfnl_amd import ops
    assert ops.DEINTERLACE_STRIP_ROWS == C_STRIP
    H, W = 8, 12
    rng = np.random.default_rng(9)
    seen = set()
    for (fmt, chroma, pack, extra, p), vals in geom["S"]:
        fmt, chroma, pack, extra, p = int(fmt), yuv.CHROMAS[int(chroma)], P.PACKINGS[int(pack)], int(extra), int(p)
        planes, vals = int(vals[0]), [int(v) for v in vals[1:]]
        name, ten = FMT_NAMES[fmt], fmt >= 3
        layout = {"rgb10": "rgb24", "p010": "nv12", "i010": "i420"}.get(name, name)
        packing = None if pack == "none" else pack
        shapes = surface.plane_shapes(name, H, W, chroma, packing)
        assert planes == len(shapes)
        tight = [rng.integers(0, 256, (rows, n * dt.itemsize)).astype(np.uint8) for rows, n, dt in shapes]
        frame = np.concatenate([t.reshape(-1) for t in tight])
        if packing is not None:                                          # (a tight v210 row is padded: the frame as push takes it)
            frame = np.zeros(P.frame_shape(packing, H, W), np.uint8)
            frame[:, :tight[0].shape[1]] = tight[0]
        want = D.field_frames(frame.view(np.uint16) if ten and packing is None else frame, layout, H, W, 10 if ten else 8, chroma, packing)[p]
        want = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
        got = []
        for k, t in enumerate(tight):
            off, pitch, rows, row_bytes = vals[4 * k:4 * k + 4]
            buf = surface.embed([t], [t.shape[1] + extra], 0xEE)[0].reshape(-1)
            assert (pitch, rows, row_bytes) == (2 * (t.shape[1] + extra), t.shape[0] // 2, t.shape[1])
            got.append(np.stack([buf[off + r * pitch:off + r * pitch + row_bytes] for r in range(rows)]))
        if packing is not None:
            assert np.array_equal(got[0], want.reshape(H // 2, -1)[:, :got[0].shape[1]])
        else:
            assert np.array_equal(np.concatenate([g.reshape(-1) for g in got]), want), (name, chroma, extra, p)
        seen.add((name, chroma, pack))
    assert {("nv12", "420", "none"), ("i420", "444", "none"), ("p010", "422", "none"), ("rgb10", "420", "x2rgb10"), ("i010", "422", "v210")} <= seen
    assert {pk for _, _, pk in seen} == set(P.PACKINGS)


def test_what_a_session_refuses_is_what_the_keywords_refuse(geom):
    for (mode, order, h, is_yuv, chroma, pack), why in geom["X"]:
        mode, order, h, is_yuv, chroma, pack = int(mode), int(order), int(h), int(is_yuv), yuv.CHROMAS[int(chroma)], P.PACKINGS[int(pack)]
        why = " ".join(why)
        if not 0 <= mode <= 2 or order not in (0, 1):
            assert why != "ok"
            continue
        try:
            stream.interlace_arguments(((None,) + D.RATES)[mode], D.FIELD_ORDERS[order], h, "nv12" if is_yuv else "rgb24", chroma, None if pack == "none" else pack)
            ok = True
        except ValueError:
            ok = False
        assert ok == (why == "ok"), (mode, order, h, is_yuv, chroma, pack, why)


class _Model:
    """push_frame's inequality (pfnl_amd/csrc/capi_stream.hip) applied once per admitted ring frame, around a plain model of the session:
    batches of ``batch`` launch when their look-ahead of T // 2 frames is there and one of two output slots is free."""

    def __init__(self, T, batch):
        self.T, self.batch, self.cap = T, batch, 3 * batch + T - 2
        self.pushed = self.launched = self.delivered = 0
        self.q = deque()

    def pump(self):
        while len(self.q) < 2 and self.pushed >= self.launched + self.batch + self.T // 2:
            self.q.append(self.launched)
            self.launched += self.batch

    def push_ok(self):
        count = self.batch if self.pushed + 1 >= self.launched + self.batch + self.T // 2 else 0
        oldest = self.q[0] if self.q else self.launched
        lo = max(oldest - self.T // 2, 0)
        return not ((count and self.launched - self.delivered + count > 2 * self.batch) or self.pushed - lo + 1 > self.cap)

    def admit(self, frames):
        saved = (self.pushed, self.launched, self.delivered, deque(self.q))
        for _ in range(frames):
            if not self.push_ok():
                self.pushed, self.launched, self.delivered, self.q = saved
                return False
            self.pushed += 1
            self.pump()
        return True

    def pop(self):
        if not self.q:
            return False
        self.delivered += 1
        if self.delivered == self.q[0] + self.batch:
            self.q.popleft()
            self.pump()
        return True


def test_the_bound_once_per_ring_frame_over_random_schedules(geom):
    refused = popped = 0
    assert len(geom["C"]) == 2 * 3 * 2 * 6
    for (T, batch, mode), ops_ in geom["C"]:
        m, woven = _Model(int(T), int(batch)), 0
        for op in ops_:
            kind, vals = op[0], [int(v) for v in op[1:].split(":")]
            if kind in "ue":
                ok = m.admit((int(mode) if woven else 0))
                woven += ok and kind == "u"
                refused += not ok
            else:
                ok = m.pop()
                popped += ok
            assert [int(ok), m.pushed, m.launched, m.delivered, len(m.q)] == vals, (T, batch, mode, op)
    assert refused > 20 and popped > 100                                # the schedules reach both


# ---- Y4M, the two loops, the hooks ------------------------------------------------------------------------------------------------------------
def test_y4m_interlace_tags():
    for tag, order in (("t", "tff"), ("b", "bff")):
        line = f"YUV4MPEG2 W720 H576 F25:1 I{tag} A16:15 C420mpeg2\n".encode()
        with pytest.raises(ValueError, match=f"interlaced streams are not supported \\(I{tag}\\); deinterlace first"):
            y4m.Y4MReader(io.BytesIO(line))
        h = y4m.Y4MReader(io.BytesIO(line), interlaced=True).header
        assert h.interlace == tag and h.to_bytes() == line
        out = h.for_output(2880, 2304, progressive=True)
        assert out.to_bytes() == b"YUV4MPEG2 W2880 H2304 F25:1 Ip A16:15 C420mpeg2\n"
        out = h.for_output(2880, 2304, progressive=True, double_rate=True)
        assert out.to_bytes() == b"YUV4MPEG2 W2880 H2304 F50:1 Ip A16:15 C420mpeg2\n"
        kw = upscale.session_keywords(h, deinterlace="field")
        assert (kw["interlaced"], kw["field_order"]) == ("field", order)
        with pytest.raises(ValueError, match=f"I{tag}"):
            upscale.session_keywords(h)
    ntsc = y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H480 F30000:1001 It", interlaced=True)
    assert ntsc.for_output(720, 480, progressive=True, double_rate=True).rate == "60000:1001"
    for flag in (False, True):
        with pytest.raises(ValueError, match="Im"):
            y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H576 Im", interlaced=flag)
    prog = y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H576 F25:1 Ip", interlaced=True)
    assert "interlaced" not in upscale.session_keywords(prog, deinterlace="frame") and prog.for_output(8, 8).to_bytes().count(b"Ip") == 1
    with pytest.raises(ValueError):
        upscale.session_keywords(prog, interlaced="frame")               # comes from the header
    assert upscale.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--deinterlace", "field"]).deinterlace == "field"
    a = rawvideo.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--in-format", "v210", "--size", "1080x1920", "--interlaced", "field",
                                      "--field-order", "bff"])
    assert (a.interlaced, a.field_order) == ("field", "bff") and rawvideo.parser().parse_args(
        ["-", "-", "--synthetic-weights", "0", "--in-format", "v210", "--size", "2x6"]).interlaced is None


class _Stub:
    """a session that delivers one frame per ring frame it would make, a frame late and the rest at the end"""
    made = []

    def __init__(self, H, W, batch, **kw):
        self.kw, self.H, self.W, self.scale, self.out_size, self.out_chroma_siting = kw, H, W, 4, None, kw.get("out_chroma_siting", "left")
        self.per = 2 if kw.get("interlaced") == "field" else 1
        self.count = self.given = 0
        _Stub.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _frames(self, upto):
        out = []
        while self.given < upto:
            out.append((self.given, np.full(self.out_samples, self.given % 251, self.out_dtype)))
            self.given += 1
        return out

    def push(self, frame):
        self.count += 1
        return self._frames((self.count - 1) * self.per if "interlaced" in self.kw else self.count - 1)

    def end(self):
        return self._frames(self.count * self.per)


@pytest.mark.parametrize("rate,frames", [(None, 3), ("frame", 3), ("field", 6)])
def test_upscale_and_rawvideo_count_progressive_frames(rate, frames):
    H, W = 8, 12
    _Stub.out_samples, _Stub.out_dtype = 16 * H * W * 3 // 2, np.uint8
    src = io.BytesIO()
    hdr = y4m.Y4MHeader(W, H, "25:1", "b" if rate else "p", interlaced_ok=True)
    wr = y4m.Y4MWriter(src, hdr)
    for i in range(3):
        wr.write_frame(np.full(H * W * 3 // 2, i, np.uint8))
    out, log = io.BytesIO(), io.StringIO()
    reader = y4m.Y4MReader(io.BytesIO(src.getvalue()), interlaced=rate is not None)
    assert upscale.upscale(reader, y4m.Y4MWriter(out), _Stub, deinterlace=rate, log=log) == frames
    kw = _Stub.made[-1].kw
    assert (kw.get("interlaced"), kw.get("field_order")) == ((rate, "bff") if rate else (None, None))
    back = y4m.Y4MReader(io.BytesIO(out.getvalue()))                     # progressive: the default reader takes it
    assert back.header.interlace == "p" and back.header.rate == ("50:1" if rate == "field" else "25:1")
    assert len(list(back)) == frames and f"{frames} frames" in log.getvalue()
    _Stub.out_samples = P.frame_bytes("uyvy422", 4 * H, 4 * W)
    raw = rawvideo.RawReader(io.BytesIO(bytes(3 * P.frame_bytes("yuyv422", H, W))), "yuyv422", H, W)
    out = io.BytesIO()
    woven = {} if rate is None else {"interlaced": rate, "field_order": "bff"}
    assert rawvideo.run(raw, rawvideo.RawWriter(out), _Stub, out_format="uyvy422", log=log, **woven) == frames
    kw = _Stub.made[-1].kw
    assert (kw.get("interlaced"), kw.get("field_order"), kw["packing"]) == ((rate, "bff", "yuyv422") if rate else (None, None, "yuyv422"))
    assert len(out.getvalue()) == frames * _Stub.out_samples


def test_the_hooks_refuse_before_any_hip_call():
    lib = _capi.load_library()
    d = C.c_void_p(64)                                                   # never dereferenced: the hooks return first
    for hook in (lib.pfnl_op_deinterlace_u8, lib.pfnl_op_deinterlace_u10):
        for at, name in enumerate((b"p2", b"p1", b"cur", b"n1", b"n2")):
            args = [d, d, d, d, d, 4, 2, 0, d, None]
            args[at] = None
            assert hook(*args) == -1 and name + b" is NULL" in lib.pfnl_last_error()
        assert hook(d, d, d, d, d, 4, 2, 0, None, None) == -1 and b"out is NULL" in lib.pfnl_last_error()
        for H in (0, 1, 3, -2):
            assert hook(d, d, d, d, d, H, 2, 0, d, None) == -1 and b"H must be even" in lib.pfnl_last_error()
        assert hook(d, d, d, d, d, 4, 0, 0, d, None) == -1 and b"W must be" in lib.pfnl_last_error()
        for parity in (-1, 2):
            assert hook(d, d, d, d, d, 4, 2, parity, d, None) == -1 and b"parity" in lib.pfnl_last_error()
    assert lib.pfnl_op_deinterlace_u10(d, C.c_void_p(65), d, d, d, 4, 2, 0, d, None) == -1 and b"p1" in lib.pfnl_last_error()
    assert lib.pfnl_stream_interlace(None, 1, 0) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_version() == 4
