"""Letterbox and pillarbox bars without a device: the rule of pfnl_amd/bars.py on literal frames and against brute force, bars_geom.h as a
plain program (and once more under AddressSanitizer and UBSan) against the Python rule, the keyword's and the command line's refusals, and
the upscale loop around a stub session and a stub measurement."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import bars_gen as G
from conftest import ROOT
from pfnl_amd import bars, stream, y4m
from pfnl_amd import upscale as up


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def test_known_answers_on_literal_frames():
    f = np.zeros((6, 8, 3), np.uint8)
    f[2:4, 1:7] = 255                                                    # white: luma 219
    rows, cols = bars.line_sums(f)
    assert rows.tolist() == [0, 0, 6 * 219, 6 * 219, 0, 0] and cols.tolist() == [0] + [2 * 219] * 6 + [0]
    assert bars.box(rows, cols, 6, 8, 8) == (2, 1, 2, 6) == bars.frame_box(f)
    f10 = np.zeros((6, 8, 3), np.uint16)
    f10[1:5, 0:8] = 1023                                                 # white at 10 bits: luma 220; a sample above 1023 counts as 1023
    f10[1, 0] = 4000
    assert bars.line_sums(f10, 10)[0].tolist() == [0, 8 * 220, 8 * 220, 8 * 220, 8 * 220, 0]
    assert bars.frame_box(f10, depth=10) == (1, 0, 4, 8)
    f[2:4, 1:7] = 0                                                      # a dark row inside the picture does not split it
    f[0, 3], f[5, 3] = 255, 255
    assert bars.frame_box(f, limit=0) == (0, 3, 6, 1)
    assert bars.frame_box(np.zeros((4, 4, 3), np.uint8)) == (0, 0, 0, 0) == bars.frame_box(np.zeros((4, 4, 3), np.uint8), limit=0)
    assert bars.LIMIT == 8 and bars.frame_box(G.boxed(12, 20, (3, 4, 6, 10))) == (3, 4, 6, 10)
    for bad in (-1, 220, 8.5, "8", None, True):
        with pytest.raises(ValueError):
            bars.box([0], [0], 1, 1, bad)
    with pytest.raises(ValueError):
        bars.box([0, 0], [0], 1, 1)
    with pytest.raises(ValueError):
        bars.line_sums(f, depth=12)
    with pytest.raises(ValueError):
        bars.line_sums(f.astype(np.uint16))                              # (depth 8 takes uint8)


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("limit", [1, 8, 100])
def test_a_sum_at_the_threshold_is_no_picture_and_one_above_is(limit, maxv):
    H, W, depth = 6, 9, 10 if maxv == 1023 else 8
    assert bars.frame_box(G.at_threshold(H, W, limit, maxv), limit, depth) == (0, 0, 0, 0)
    assert bars.frame_box(G.at_threshold(H, W, limit, maxv, over=True), limit, depth) == (H // 2, W // 3, 1, 1)
    rows, cols = [limit * W] * H, [limit * H] * W                        # and on the sums themselves, rows and columns apart
    assert bars.box(rows, cols, H, W, limit) == (0, 0, 0, 0)
    rows[4] += 1
    assert bars.box(rows, cols, H, W, limit) == (0, 0, 0, 0)             # a picture row alone, no picture column: empty
    cols[2] += 1
    assert bars.box(rows, cols, H, W, limit) == (4, 2, 1, 1)
    rows[4] -= 1
    assert bars.box(rows, cols, H, W, limit) == (0, 0, 0, 0)


def test_a_lone_bright_pixel_in_a_bar_does_not_lift_its_row():
    H, W = 32, 48                                                        # 219 <= 8 * 32: one white pixel stays under both thresholds
    f = G.boxed(H, W, (8, 0, 16, W))
    f[2, 5] = 255
    f[30, 40] = 255
    assert bars.frame_box(f) == (8, 0, 16, W)
    assert bars.frame_box(f, limit=0)[0] == 2                            # (it is seen where the limit says so)


def test_box_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    for case in range(200):
        H, W, limit = int(rng.integers(1, 12)), int(rng.integers(1, 12)), int(rng.integers(0, 220))
        rows = rng.integers(max(limit * W - 3, 0), limit * W + 4, H)
        cols = rng.integers(max(limit * H - 3, 0), limit * H + 4, W)
        top = bottom = left = right = None
        for y in range(H):
            if rows[y] > limit * W:
                top = y if top is None else top
                bottom = y
        for x in range(W):
            if cols[x] > limit * H:
                left = x if left is None else left
                right = x
        want = (0, 0, 0, 0) if top is None or left is None else (top, left, bottom - top + 1, right - left + 1)
        assert bars.box(rows, cols, H, W, limit) == want, case


def test_union_snap_and_decide():
    assert bars.union([]) == (0, 0, 0, 0) == bars.union([(0, 0, 0, 0), (3, 3, 0, 5), (3, 3, 5, 0)])
    assert bars.union([(2, 3, 4, 5)]) == (2, 3, 4, 5) == bars.union([(0, 0, 0, 0), (2, 3, 4, 5)])
    assert bars.union([(2, 3, 4, 5), (1, 6, 2, 10), (0, 0, 0, 0)]) == (1, 3, 5, 13)
    assert bars.snap((3, 5, 10, 11), 4, 2) == (4, 6, 8, 10) and bars.snap((4, 6, 8, 10), 4, 2) == (4, 6, 8, 10)
    assert bars.snap((1, 0, 3, 8), 4, 2) == (0, 0, 0, 0) == bars.snap((0, 1, 8, 1), 2, 2) == bars.snap((0, 0, 0, 0), 2, 2)
    assert bars.align("420", True) == (4, 2) and bars.align("420", False) == (2, 2) == bars.align("422", True) == bars.align(None, True)
    rng = np.random.default_rng(5)
    for case in range(300):
        H, W = int(rng.integers(2, 40)), int(rng.integers(2, 40))
        ay, ax = (int(rng.choice([1, 2, 4])), int(rng.choice([1, 2])))
        boxes = []
        for _ in range(int(rng.integers(0, 4))):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            boxes.append((y0, x0, int(rng.integers(0, H - y0 + 1)), int(rng.integers(0, W - x0 + 1))))
        u = bars.union(boxes)
        for b in boxes:                                                  # the union holds every non-empty box
            if b[2] and b[3]:
                assert u[0] <= b[0] and u[1] <= b[1] and u[0] + u[2] >= b[0] + b[2] and u[1] + u[3] >= b[1] + b[3]
        s = bars.snap(u, ay, ax)
        if s != (0, 0, 0, 0):                                            # inside the union, on the grid, and no grid line further out fits
            assert s[0] >= u[0] and s[1] >= u[1] and s[0] + s[2] <= u[0] + u[2] and s[1] + s[3] <= u[1] + u[3]
            assert s[0] % ay == s[2] % ay == s[1] % ax == s[3] % ax == 0
            assert s[0] - ay < u[0] and s[1] - ax < u[1] and s[0] + s[2] + ay > u[0] + u[2] and s[1] + s[3] + ax > u[1] + u[3]
        d = bars.decide(boxes, H, W, ay, ax)
        keeps = s != (0, 0, 0, 0) and 3 * s[2] >= H and 3 * s[3] >= W
        assert d == (s if keeps else (0, 0, H, W)), case
    assert bars.decide([], 32, 48, 2, 2) == (0, 0, 32, 48) == bars.decide([(0, 0, 0, 0)] * 3, 32, 48, 2, 2)
    assert bars.decide([(12, 0, 10, 48)], 32, 48, 2, 2) == (0, 0, 32, 48)   # a fade-in's sliver: less than a third of the rows
    assert bars.decide([(12, 0, 10, 48)], 32, 48, 2, 2, min_keep=(1, 4)) == (12, 0, 10, 48)
    assert bars.decide([(10, 0, 11, 48)], 32, 48, 2, 2) == (0, 0, 32, 48) and bars.decide([(10, 0, 12, 48)], 32, 48, 2, 2) == (10, 0, 12, 48)
    assert bars.decide([(8, 0, 16, 48), (9, 2, 3, 3)], 32, 48, 4, 2) == (8, 0, 16, 48)
    with pytest.raises(ValueError):
        bars.decide([], 4, 4, 2, 2, min_keep=(2, 1))
    with pytest.raises(ValueError):
        bars.snap((0, 0, 4, 4), 0, 2)


# ---- bars_geom.h as a plain program ---------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <vector>
#include "bars_geom.h"

// every line of stdin is one case; the answer goes to stdout in the same order
int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'B') {                                              // H W limit rows.. cols.. -> the box, scanned whole and by three strided scans
            int H, W, limit;
            if (std::scanf("%d %d %d", &H, &W, &limit) != 3) return 2;
            std::vector<unsigned> rows(H), cols(W);
            for (auto& v : rows) if (std::scanf("%u", &v) != 1) return 2;
            for (auto& v : cols) if (std::scanf("%u", &v) != 1) return 2;
            int32_t whole[4], merged[4];
            int rf, rl, cf, cl;
            pfnl::bars_scan([&](int i) { return rows[i]; }, H, pfnl::bars_threshold(limit, W), 0, 1, &rf, &rl);
            pfnl::bars_scan([&](int i) { return cols[i]; }, W, pfnl::bars_threshold(limit, H), 0, 1, &cf, &cl);
            pfnl::bars_box(rf, rl, cf, cl, whole);
            int span[4] = {H, -1, W, -1};
            for (int t = 0; t < 3; ++t) {
                pfnl::bars_scan([&](int i) { return rows[i]; }, H, pfnl::bars_threshold(limit, W), t, 3, &rf, &rl);
                pfnl::bars_scan([&](int i) { return cols[i]; }, W, pfnl::bars_threshold(limit, H), t, 3, &cf, &cl);
                span[0] = rf < span[0] ? rf : span[0], span[1] = rl > span[1] ? rl : span[1];
                span[2] = cf < span[2] ? cf : span[2], span[3] = cl > span[3] ? cl : span[3];
            }
            pfnl::bars_box(span[0], span[1], span[2], span[3], merged);
            std::printf("B %d %d %d %d | %d %d %d %d | %d\n", whole[0], whole[1], whole[2], whole[3], merged[0], merged[1], merged[2], merged[3],
                        (int)pfnl::bars_args_ok(H, W, limit));
        } else if (kind == 'D') {                                       // H W ay ax p q n boxes.. -> union, its snap, the decision
            int H, W, ay, ax, p, q, n;
            if (std::scanf("%d %d %d %d %d %d %d", &H, &W, &ay, &ax, &p, &q, &n) != 7) return 2;
            int32_t u[4] = {0, 0, 0, 0}, s[4], d[4];
            for (int k = 0; k < n; ++k) {
                int32_t b[4];
                if (std::scanf("%d %d %d %d", &b[0], &b[1], &b[2], &b[3]) != 4) return 2;
                pfnl::bars_union(u, b);
            }
            for (int k = 0; k < 4; ++k) s[k] = u[k];
            pfnl::bars_snap(s, ay, ax);
            pfnl::bars_decide(u, H, W, ay, ax, p, q, d);
            std::printf("D %d %d %d %d | %d %d %d %d | %d %d %d %d\n", u[0], u[1], u[2], u[3], s[0], s[1], s[2], s[3], d[0], d[1], d[2], d[3]);
        } else if (kind == 'A') {                                       // planes_420 woven -> the grid
            int c, w, ay, ax;
            if (std::scanf("%d %d", &c, &w) != 2) return 2;
            pfnl::bars_align(c != 0, w != 0, &ay, &ax);
            std::printf("A %d %d\n", ay, ax);
        } else {
            return 2;
        }
    }
    std::printf("K %d %d\n", pfnl::BARS_LIMIT_MAX, pfnl::BARS_MAX_SIDE);
    return 0;
}
"""


def _cxx():
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build's own clang++ is the last candidate)"
    return cxx


def _cases():
    rng = np.random.default_rng(3)
    lines, want = [], []
    for _ in range(300):
        H, W, limit = int(rng.integers(1, 14)), int(rng.integers(1, 14)), int(rng.integers(0, 220))
        rows = rng.integers(max(limit * W - 2, 0), limit * W + 3, H)
        cols = rng.integers(max(limit * H - 2, 0), limit * H + 3, W)
        lines.append(f"B {H} {W} {limit} " + " ".join(str(v) for v in rows) + " " + " ".join(str(v) for v in cols))
        b = bars.box(rows, cols, H, W, limit)
        want.append("B %d %d %d %d | %d %d %d %d | 1" % (*b, *b))
    H, W = bars.MAX_SIDE, 1                                              # the largest sums there are: 220 * 16384 a line, against the largest limit
    rows, cols = [220] * H, [220 * H]
    lines.append(f"B {H} {W} 219 " + " ".join(str(v) for v in rows) + " " + " ".join(str(v) for v in cols))
    want.append("B 0 0 %d 1 | 0 0 %d 1 | 1" % (H, H))
    for _ in range(300):
        H, W = int(rng.integers(2, 60)), int(rng.integers(2, 60))
        ay, ax, q = int(rng.choice([1, 2, 4])), int(rng.choice([1, 2])), int(rng.integers(1, 6))
        p = int(rng.integers(0, q + 1))
        boxes = []
        for _ in range(int(rng.integers(0, 5))):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            boxes.append((y0, x0, int(rng.integers(0, H - y0 + 1)), int(rng.integers(0, W - x0 + 1))))
        lines.append(f"D {H} {W} {ay} {ax} {p} {q} {len(boxes)} " + " ".join(" ".join(str(v) for v in b) for b in boxes))
        u = bars.union(boxes)
        want.append("D %d %d %d %d | %d %d %d %d | %d %d %d %d" % (*u, *bars.snap(u, ay, ax), *bars.decide(boxes, H, W, ay, ax, (p, q))))
    for c in (0, 1):
        for w in (0, 1):
            lines.append(f"A {c} {w}")
            want.append("A %d %d" % bars.align("420" if c else "444", bool(w)))
    want.append(f"K {bars.LIMIT_MAX} {bars.MAX_SIDE}")
    return "\n".join(lines) + "\n", want


def test_bars_geom_walks_the_rule(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    text, want = _cases()
    for name, flags in (("driver", []), ("driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name                                            # stand-alone host code: the sanitizers need no preload
        subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
        got = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.strip().split("\n")
        assert len(got) == len(want) == 606
        for k, (a, b) in enumerate(zip(got, want)):
            assert a == b, (name, k, text.split("\n")[k] if k < 605 else "K")


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_the_keyword_refuses_what_the_library_refuses():
    assert stream.bars_argument(None) is None and stream.bars_argument(8, 16, 24) == 8
    assert stream.bars_argument(0) == 0 and stream.bars_argument(np.int64(219)) == 219
    for bad in (-1, 220, 8.0, "8", True, (8,)):
        with pytest.raises(ValueError, match="limit"):
            stream.bars_argument(bad, 16, 24)
    with pytest.raises(ValueError, match="16384"):
        stream.bars_argument(8, 16386, 24)
    info = stream.PopInfo(3, 99, (1, 2, 3, 4))                           # last_info with bars: the tuple it always was, and the box
    assert info == (3, 99) and tuple(info) == (3, 99) and info[0] == 3 and info[1] == 99 and len(info) == 2
    assert info["box"] == (1, 2, 3, 4) == info.box and info["scene_first"] == 3 and info["sad"] == 99
    with pytest.raises(KeyError):
        info["boxes"]


def test_the_crop_parser_and_the_grid():
    base = ["in.y4m", "-", "--synthetic-weights", "0"]
    a = up.parser().parse_args(base)
    assert (a.crop, a.crop_limit, a.crop_probe) == (None, 8, 120)
    a = up.parser().parse_args(base + ["--crop", "auto", "--crop-limit", "12", "--crop-probe", "30"])
    assert (a.crop, a.crop_limit, a.crop_probe) == ("auto", 12, 30)
    assert up.parser().parse_args(base + ["--crop", "60,0,360,720"]).crop == (60, 0, 360, 720)
    for bad in ("60,0,360", "60,0,360,720,1", "a,b,c,d", "Auto", "", "60 0 360 720"):
        with pytest.raises(SystemExit):
            up.parser().parse_args(base + ["--crop", bad])
    assert bars.check_crop((60, 0, 360, 720), 480, 720, 4, 2) == (60, 0, 360, 720)
    for box, word in (((62, 0, 360, 720), "grid"), ((60, 1, 360, 718), "grid"), ((60, 0, 358, 720), "grid"), ((60, 0, 360, 722), "outside"),
                      ((-4, 0, 360, 720), "outside"), ((124, 0, 360, 720), "outside"), ((60, 0, 0, 720), "outside")):
        with pytest.raises(ValueError, match=word):
            bars.check_crop(box, 480, 720, 4, 2)
    assert bars.check_crop((62, 0, 360, 720), 480, 720, 2, 2) == (62, 0, 360, 720)   # (progressive: rows in twos)


# ---- the loop, around a stub session and a stub measure -------------------------------------------------------------------------------------
class _Stub:
    """delivers ``batch`` frames late, as zeros of the session's output size; records every push"""
    scale = 4

    def __init__(self, log, H, W, batch=1, **kw):
        self.H, self.W, self.batch, self.kw = H, W, batch, kw
        self.out_size, self.out_chroma_siting = None, kw["chroma_siting"]
        self.log, self.held, self.pushed = log, [], 0
        log.append(("open", H, W, batch, dict(kw)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.log.append(("close",))

    def _take(self, what, payload):
        self.log.append((what, payload))
        self.held.append((self.pushed, np.zeros((4 * self.H * 3 // 2, 4 * self.W), np.uint8)))
        self.pushed += 1
        due, self.held = self.held[:-self.batch], self.held[-self.batch:]
        return due

    def push(self, frame):
        return self._take("push", frame)

    def push_planes(self, *planes):
        assert [p.shape for p in planes] == [(self.H, self.W), (self.H // 2, self.W // 2), (self.H // 2, self.W // 2)]
        return self._take("planes", planes)

    def end(self):
        due, self.held = self.held, []
        return due


UH, UW = 32, 48


def _tagged_stream(n, head=b"YUV4MPEG2 W48 H32 F25:1 Ip C420jpeg\n"):
    """n frames whose every sample says where it is: plane, row, column and frame can be read off a window"""
    frames = []
    for k in range(n):
        y = (np.arange(UH)[:, None] * 7 + np.arange(UW)[None, :] * 3 + k) % 251
        cb = (np.arange(UH // 2)[:, None] * 5 + np.arange(UW // 2)[None, :] * 11 + k + 100) % 251
        cr = (np.arange(UH // 2)[:, None] * 13 + np.arange(UW // 2)[None, :] * 2 + k + 200) % 251
        frames.append(np.concatenate([p.reshape(-1) for p in (y, cb, cr)]).astype(np.uint8).reshape(UH * 3 // 2, UW))
    return head + b"".join(b"FRAME\n" + f.tobytes() for f in frames), frames


def _run(data, interlaced=False, **kw):
    log, out, err = [], io.BytesIO(), io.StringIO()
    n = up.upscale(y4m.Y4MReader(io.BytesIO(data), interlaced=interlaced), y4m.Y4MWriter(out), lambda H, W, batch=1, **k: _Stub(log, H, W, batch, **k),
                   log=err, **kw)
    return n, log, out.getvalue(), err.getvalue()


def test_upscale_pushes_windows_of_the_decided_rectangle():
    data, frames = _tagged_stream(7)
    seen = []

    def measure(fs, header, limit):
        seen.append((len(fs), header.height, header.width, limit))
        assert all(np.array_equal(a, b) for a, b in zip(fs, frames))     # the frames read ahead, as the reader gives them
        return [(9, 0, 3, 48), (8, 2, 16, 44), (0, 0, 0, 0)]             # union (8, 0, 16, 48)

    n, log, out, err = _run(data, batch=2, crop="auto", crop_limit=11, crop_probe=3, measure=measure)
    assert n == 7 and seen == [(3, UH, UW, 11)]
    assert err.split("\n")[0] == "crop 8,0,16,48 (from 3 frames)"
    assert log[0][:4] == ("open", 16, 48, 2) and "crop" not in log[0][4] and "bars" not in log[0][4] and log[-1] == ("close",)
    pushes = log[1:-1]
    assert [p[0] for p in pushes] == ["planes"] * 7                      # the buffered frames first, then the rest, in order
    for k, (_, (y, cb, cr)) in enumerate(pushes):
        full = frames[k].reshape(-1)
        Y, Cb, Cr = full[:UH * UW].reshape(UH, UW), full[UH * UW:UH * UW * 5 // 4].reshape(UH // 2, UW // 2), full[UH * UW * 5 // 4:].reshape(UH // 2, UW // 2)
        assert np.array_equal(y, Y[8:24]) and np.array_equal(cb, Cb[4:12]) and np.array_equal(cr, Cr[4:12])
        assert np.shares_memory(y, frames[k]) or y.base is not None      # a view: nothing was copied
    assert out.startswith(b"YUV4MPEG2 W192 H64 F25:1 Ip")                # the output header is the cropped session's

    # a rectangle named by the caller: no measurement, no line on stderr, windows with both offsets
    n, log, out, err = _run(data, batch=1, crop=(4, 6, 20, 30), measure=lambda *a: pytest.fail("measured"))
    assert n == 7 and "crop" not in err and log[0][:4] == ("open", 20, 30, 1)
    y, cb, cr = log[3][1]
    Y = frames[2].reshape(-1)[:UH * UW].reshape(UH, UW)
    assert np.array_equal(y, Y[4:24, 6:36]) and cb.shape == (10, 15) and cb.strides == (UW // 2, 1)


def test_a_full_frame_decision_and_no_crop_take_todays_path():
    data, frames = _tagged_stream(4)
    plain = _run(data, batch=2)
    assert [p[0] for p in plain[1][1:-1]] == ["push"] * 4 and plain[1][0][:4] == ("open", UH, UW, 2)
    for boxes in ([(0, 0, UH, UW)], [(0, 0, 0, 0)] * 3, [(14, 0, 4, UW)], []):   # the whole frame, black, a sliver (min_keep), nothing
        n, log, out, err = _run(data, batch=2, crop="auto", crop_probe=3, measure=lambda fs, h, lim, b=boxes: b)
        assert err.split("\n")[0] == f"crop 0,0,{UH},{UW} (from 3 frames)"
        assert log[0] == plain[1][0] and [p[0] for p in log[1:-1]] == ["push"] * 4 and out == plain[2]
        for (_, a), b in zip(log[1:-1], frames):
            assert np.array_equal(a, b)
    n, log, _, _ = _run(data, batch=2, crop=(0, 0, UH, UW))             # named, and the whole frame
    assert log[0] == plain[1][0] and [p[0] for p in log[1:-1]] == ["push"] * 4
    n, log, _, err = _run(data, batch=2, crop="auto", crop_probe=50, measure=lambda fs, h, lim: [(8, 0, 16, 48)] * len(fs))
    assert n == 4 and err.startswith("crop 8,0,16,48 (from 4 frames)") and [p[0] for p in log[1:-1]] == ["planes"] * 4   # a probe longer than the stream


def test_the_grid_follows_the_stream_and_bad_rectangles_are_named():
    data, _ = _tagged_stream(3)
    woven, _ = _tagged_stream(3, b"YUV4MPEG2 W48 H32 F25:1 It C420jpeg\n")
    with pytest.raises(ValueError, match="grid"):
        _run(woven, interlaced=True, deinterlace="frame", crop=(6, 0, 16, 48))    # woven 4:2:0: rows in fours
    assert _run(data, crop=(6, 0, 16, 48))[1][0][:3] == ("open", 16, 48)
    n, log, _, err = _run(woven, interlaced=True, deinterlace="frame", crop="auto", measure=lambda fs, h, lim: [(6, 0, 20, 48)] * len(fs))
    assert err.startswith("crop 8,0,16,48 (from 3 frames)") and log[0][4]["interlaced"] == "frame"
    for box, word in (((8, 0, 16, 50), "outside"), ((8, 1, 16, 46), "grid"), ((40, 0, 16, 48), "outside")):
        with pytest.raises(ValueError, match=word):
            _run(data, crop=box)
    for bad in ({"crop_limit": 220}, {"crop_probe": 0}):
        with pytest.raises(ValueError):
            _run(data, crop="auto", measure=lambda fs, h, lim: [], **bad)


def test_the_command_line_names_a_bad_rectangle(tmp_path, capsys):
    src = tmp_path / "in.y4m"
    src.write_bytes(_tagged_stream(1)[0])
    for crop, word in (("8,0,16,50", "outside"), ("8,1,16,46", "grid")):   # checked against the header, ahead of any engine: status 1 and the reason
        status = up.main([str(src), str(tmp_path / "out.y4m"), "--synthetic-weights", "0", "--num-block", "1", "--crop", crop])
        err = capsys.readouterr().err
        assert status == 1 and err.startswith("pfnl_amd.upscale: crop ") and word in err
