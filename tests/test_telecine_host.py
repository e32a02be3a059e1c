"""Inverse telecine, the host side (pfnl_amd/telecine.py; pfnl_amd/csrc/telecine_geom.h): known answers of the comb count, pulldown material
in every phase and both field orders given back as the film, the video insert, marks, an incomplete cycle, telecine_geom.h as a plain C++
program (and once more under AddressSanitizer and UBSan) against the Python rule, the library's refusals and pfnl_telecine_deliverable
without a device, the Y4M header, and the two command-line loops around a stub session."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import telecine_gen as G
from conftest import ROOT
from pfnl_amd import _capi, deinterlace as D, rawvideo, stream, telecine as TC, upscale, y4m
from pfnl_amd import packed as P


def _col(*v):
    return np.array(v, np.int64).reshape(-1, 1, 1)


# ---- known answers --------------------------------------------------------------------------------------------------------------------------
def test_comb_count_known_answers():
    # h = 1: both neighbours clamp onto A[0]: a = b = X - A, combed iff (X - A)^2 > T^2
    assert TC.comb_count(_col(100), _col(111), 0) == 1 and TC.comb_count(_col(100), _col(110), 0) == 0     # 11 * 11 > 100; 10 * 10 is not
    assert TC.comb_count(_col(100), _col(89), 1) == 1 and TC.comb_count(_col(100), _col(90), 1) == 0
    # parity 0: the missing row j lies between A[j] and A[j + 1] (the last one clamps); parity 1: between A[j - 1] (the first clamps) and A[j]
    A = _col(100, 200, 100)
    X = _col(150, 150, 150)                                              # between its neighbours everywhere they differ: a b < 0
    assert TC.comb_count(A, X, 0) == 1                                   # rows 0, 1: 50 * -50, -50 * 50; row 2: A[2], A[2] clamped: 50 * 50
    assert TC.comb_count(A, X, 1) == 1                                   # row 0: A[0], A[0]: 50 * 50; rows 1, 2 between
    X = _col(250, 50, 120)
    # parity 0: (150, 50) combed; (-150, -50) combed; (20, 20) 400 > 100 combed.  parity 1: (150, 150); (-50, -150); (-80, 20) not
    assert TC.comb_count(A, X, 0) == 3 and TC.comb_count(A, X, 1) == 2
    # a b exactly T^2 is not combed; one above is: a = 5, b = 20 -> 100; a = 5, b = 21 -> 105
    assert TC.comb_count(_col(100, 85, 85), _col(105, 85, 85), 0, 10) == 0
    assert TC.comb_count(_col(100, 84, 84), _col(105, 84, 84), 0, 10) == 1
    assert TC.comb_count(_col(100, 84, 84), _col(105, 84, 84), 0, 11) == 0
    # one sign is needed: -5 * -21; and a product of two signs is never combed however large
    assert TC.comb_count(_col(105, 121, 121), _col(100, 121, 121), 0, 10) == 1 and TC.comb_count(_col(0, 255, 255), _col(128, 255, 255), 0, 1) == 0
    # 10 bits: T = 4 threshold; samples above 1023 are 1023 first
    assert TC.comb_count(_col(400), _col(441), 0, 10, 1023) == 1 and TC.comb_count(_col(400), _col(440), 0, 10, 1023) == 0
    assert TC.comb_count(_col(1023), _col(65535), 0, 10, 1023) == 0 and TC.comb_count(_col(2000), _col(982), 0, 10, 1023) == 1
    assert TC.comb_count(_col(2000), _col(983), 0, 10, 1023) == 0
    # every sample alone, no horizontal term: a [2, 3, 3] field counts its 18 samples one by one
    A = np.zeros((2, 3, 3), np.uint8)
    X = np.zeros((2, 3, 3), np.uint8)
    X[0, 1, 2] = X[1, 0, 0] = 50
    assert TC.comb_count(A, X, 0) == 2 and TC.comb_count(A, X, 0) <= 2 * 3 * 3
    assert TC.match(A, X, A, 0) == ("p", 2, 0) and TC.match(A, X, X, 1) == ("c", 2, 2)       # the smaller count; c on a tie
    with pytest.raises(ValueError):
        TC.comb_count(A, X, 2)
    with pytest.raises(ValueError):
        TC.comb_count(A, X[:1], 0)


def test_the_defaults_and_the_ids():
    assert (TC.THRESHOLD, TC.POST, TC.CYCLE) == (10, True, 5) and TC.comb_limit_default(540, 1920) == (540 * 3 * 1920) >> 8
    assert TC.params(4, 12) == (10, 1, 0) and TC.params(8, 20, 3, False, 7) == (3, 0, 7)
    assert [TC.mode_id(m) for m in (None, "match", "decimate")] == [0, 1, 2]
    for bad in ("both", 1, "frame"):
        with pytest.raises(ValueError):
            TC.mode_id(bad)
    for bad in ({"threshold": 0}, {"threshold": 256}, {"comb_limit": -1}):
        with pytest.raises(ValueError):
            TC.params(4, 12, **bad)
    assert TC.match_fields(0, 3) == (0, 1, 1) and TC.match_fields(2, 3) == (4, 5, 3)


# ---- pulldown and back ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", G.SHAPES)
@pytest.mark.parametrize("maxv", [255, 1023])
def test_the_content_separates_right_from_wrong(H, W, maxv):
    """what the GPU tests rely on: every film frame differs from its predecessor, no sample of a true frame is combed, and wherever one
    candidate belongs to another film frame its count exceeds the right one's - and the default limit"""
    film = G.film(G.N_FILM, H, W, maxv)
    assert all(not np.array_equal(a, b) for a, b in zip(film, film[1:]))
    limit = TC.comb_limit_default(H // 2, W)
    for order in D.FIELD_ORDERS:
        for phase in range(5):
            pushed = TC.pulldown(film, phase, order)
            under = TC.pulldown_fields(G.N_FILM, phase)
            _, dec = TC.matched_frames(pushed, order, maxv=maxv)
            for n, d in enumerate(dec):
                a, c, p = TC.match_fields(n, len(pushed))
                for count, k in ((d["count_c"], c), (d["count_p"], p)):
                    if under[k] == under[a]:
                        assert count == 0
                    else:
                        assert count > limit and count > min(d["count_c"], d["count_p"]) == 0
                assert d["post"] == 0


@pytest.mark.parametrize("order", D.FIELD_ORDERS)
@pytest.mark.parametrize("phase", range(5))
@pytest.mark.parametrize("maxv", [255, 1023])
def test_decimate_gives_the_film_back_and_match_every_frame_its_film_frame(phase, order, maxv):
    H, W = G.SHAPES[phase % 2]
    film = G.film(G.N_FILM, H, W, maxv)
    pushed = TC.pulldown(film, phase, order)
    assert len(pushed) == G.N_PUSHED and all(f.shape == (H, W, 3) and f.dtype == film[0].dtype for f in pushed)
    out = TC.frames(pushed, "decimate", order, maxv=maxv)
    assert len(out) == G.N_FILM and all(np.array_equal(a, b) for a, b in zip(out, film))
    matched = TC.frames(pushed, "match", order, maxv=maxv)
    under = TC.pulldown_fields(G.N_FILM, phase)
    assert len(matched) == G.N_PUSHED and all(np.array_equal(m, film[under[2 * n]]) for n, m in enumerate(matched))
    assert TC.stats(pushed, "decimate", order, maxv=maxv)[2:] == (0, 2, G.N_FILM)
    c, p, flagged, dropped, delivered = TC.stats(pushed, "match", order, maxv=maxv)
    assert (c + p, flagged, dropped, delivered) == (G.N_PUSHED, 0, 0, G.N_PUSHED) and p >= 2          # frames woven from two film frames match p


def test_pulldown_cadences():
    assert TC.pulldown_fields(8, 0) == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 5, 5, 6, 6, 6, 7, 7]
    assert TC.pulldown_fields(8, 1)[:8] == [0, 0, 0, 1, 1, 1, 2, 2]       # a lone first field and the two behind it: 1 + 2 -> 3
    assert TC.pulldown_fields(8, 2)[:8] == [0, 0, 1, 1, 2, 2, 3, 3]       # ... and the three behind it: 1 + 3 -> 2 + 2
    assert TC.pulldown_fields(8, 3)[:7] == [0, 0, 1, 1, 2, 2, 2] and TC.pulldown_fields(8, 4)[:7] == [0, 0, 1, 1, 1, 2, 2]
    for phase in range(5):
        f = TC.pulldown_fields(8, phase)
        assert len(f) == 20 and f[0] == 0 and f[-1] == 7 and all(0 <= b - a <= 1 for a, b in zip(f, f[1:]))
        assert all(f.count(i) in (2, 3, 4) for i in range(8))
    assert len(TC.pulldown_fields(3, 0)) == 8 and len(TC.pulldown_fields(8, 0, 4)) == 8
    with pytest.raises(ValueError):
        TC.pulldown_fields(8, 5)


@pytest.mark.parametrize("maxv", [255, 1023])
def test_a_video_insert(maxv):
    """two frames woven from four different instants, behind a whole film frame and ahead of one: with post they are flagged and are the
    deinterlacer's frames; without, the c-weave - the frames as pushed"""
    H, W = G.SHAPES[1]
    pushed = TC.pulldown(G.film(G.N_FILM, H, W, maxv), 0, "tff")
    pushed[6:8] = G.video(2, H, W, maxv)
    video = D.frames(pushed, "tff", "frame", maxv)
    m, dec = TC.matched_frames(pushed, "tff", maxv=maxv)
    assert [d["post"] for d in dec] == [0, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    assert all(np.array_equal(m[n], video[n]) for n in (6, 7)) and not any(np.array_equal(m[n], video[n]) for n in (1, 2, 5, 8))
    m, dec = TC.matched_frames(pushed, "tff", post=False, maxv=maxv)
    assert not any(d["post"] for d in dec) and all(dec[n]["match"] == 0 and np.array_equal(m[n], pushed[n]) for n in (6, 7))
    assert min(dec[6]["count_c"], dec[7]["count_c"]) > TC.comb_limit_default(H // 2, W)
    m, dec = TC.matched_frames(pushed, "tff", comb_limit=10 ** 6, maxv=maxv)         # a limit nothing exceeds flags nothing
    assert not any(d["post"] for d in dec)


def test_mark_placement_for_every_frame_and_drop():
    for j in range(5):
        for d in list(range(5)) + [None]:
            marks = [i == j for i in range(5)]
            out, carry = TC.place_marks(marks, d)
            kept = [i for i in range(5) if i != d]
            assert len(out) == len(kept) and sum(out) + carry == 1
            if j != d:
                assert out[kept.index(j)]                                # on the frame made from it
            elif j < 4:
                assert out[kept.index(j + 1)]                            # dropped: on the next delivered one
            else:
                assert carry and not any(out)                            # the cycle's last frame dropped: the next cycle's first
            out2, carry2 = TC.place_marks([False] * 5, d, carry)
            assert out2[0] == carry and not carry2 and sum(out2) == int(carry)
    frames = [np.full((2, 1, 3), v, np.uint8) for v in (0, 9, 9, 30, 60, 90, 120, 120, 150, 151, 200, 230)]
    out, dropped, marks = TC.decimate(frames, [n in (2, 7, 11) for n in range(12)])
    assert dropped == [2, 7] and [int(f[0, 0, 0]) for f in out] == [0, 9, 30, 60, 90, 120, 150, 151, 200, 230]
    assert [i for i, m in enumerate(marks) if m] == [2, 6, 9]             # (12 frames: two whole cycles and two frames delivered whole)


def test_decimation_ties_the_first_frame_and_an_incomplete_cycle():
    same = [np.zeros((2, 1, 3), np.uint8)] * 7
    assert TC.distances(same) == [TC.D_FIRST] + [0] * 6
    out, dropped, _ = TC.decimate(same)
    assert dropped == [1] and len(out) == 6                             # D_0 is never the smallest; a tie drops the lowest index; 5, 6 whole
    assert TC.drop_index([5, 5, 5, 5, 5]) == 0 and TC.drop_index([9, 3, 7, 3, 8]) == 1
    for n in range(13):
        frames = [np.full((2, 1, 3), 10 * i, np.uint8) for i in range(n)]
        for ended in (False, True):
            made = n if ended else max(n - 1, 0)
            assert TC.deliverable("match", n, ended) == made
            assert TC.deliverable("decimate", n, ended) == 4 * (made // 5) + (made % 5 if ended else 0)
        if n:
            assert len(TC.decimate(frames)[0]) == TC.deliverable("decimate", n, True) == len(TC.frames(frames, "decimate"))


# ---- telecine_geom.h as a plain program -----------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <initializer_list>
#include "telecine_geom.h"

int main() {
    std::printf("K %d\n", pfnl::TC_CYCLE);
    for (long long n_frames = 1; n_frames <= 3; ++n_frames)
        for (long long n = 0; n < n_frames; ++n) {
            const pfnl::MatchFields f = pfnl::telecine_match_fields(n, 2 * n_frames);
            std::printf("F %lld %lld | %lld %lld %lld\n", n_frames, n, f.a, f.c, f.p);
        }
    for (int mode = 1; mode <= 2; ++mode)
        for (long long pushed = 0; pushed <= 12; ++pushed) {
            long long made = 0;                                        // pushes one by one, then the end: the yields add up
            for (long long k = 0; k < pushed; ++k) made += pfnl::telecine_push_yield(mode, k);
            const long long matched = pushed > 0 ? pushed - 1 : 0;
            std::printf("Y %d %lld | %lld %lld %lld %lld %lld\n", mode, pushed, made, made + pfnl::telecine_end_yield(mode, pushed, matched),
                        pfnl::telecine_deliverable(mode, pushed, 0), pfnl::telecine_deliverable(mode, pushed, 1), pfnl::telecine_cycle(pushed));
        }
    for (int j = 0; j < pfnl::TC_CYCLE; ++j)
        for (int d = -1; d < pfnl::TC_CYCLE; ++d)
            for (int carry0 = 0; carry0 < 2; ++carry0) {
                bool marks[pfnl::TC_CYCLE] = {false, false, false, false, false}, out[pfnl::TC_CYCLE], carry = carry0 != 0;
                marks[j] = true;
                const int made = pfnl::telecine_place_marks(marks, pfnl::TC_CYCLE, d, &carry, out);
                std::printf("M %d %d %d | %d %d", j, d, carry0, made, (int)carry);
                for (int i = 0; i < made; ++i) std::printf(" %d", (int)out[i]);
                std::printf("\n");
            }
    const unsigned long long ds[4][5] = {{5, 5, 5, 5, 5}, {9, 3, 7, 3, 8}, {pfnl::TC_D_FIRST, 4, 4, 2, 9}, {7, 6, 5, 4, 3}};
    for (const auto& d : ds) std::printf("D %llu %llu %llu %llu %llu | %d\n", d[0], d[1], d[2], d[3], d[4], pfnl::telecine_drop_index(d));
    // telecine_ring_fits against a walk of the bound itself: cycles of four frames from an empty ring, everything deliverable popped
    // where a cycle is refused (the pop as field_geom.h's own test program states it); a cycle refused with nothing left to pop never fits
    for (int T : {1, 3, 5, 7})
        for (int batch = 1; batch <= 5; ++batch) {
            const int cap = 3 * batch + T - 2;
            pfnl::RingCounters c{0, 0, 0, 0, 0};
            bool fits = true;
            const auto pop = [&] {
                if (!c.in_flight) return false;
                if (++c.delivered == c.oldest + batch) {
                    --c.in_flight;
                    c.oldest += batch;
                    while (c.in_flight < 2 && pfnl::ring_next_batch(T, batch, c.pushed, c.launched)) {
                        if (!c.in_flight) c.oldest = c.launched;
                        c.launched += batch;
                        ++c.in_flight;
                    }
                }
                return true;
            };
            for (int q = 0; q < 40 && fits; ++q) {
                if (pfnl::ring_admit_all(T, batch, cap, pfnl::TC_CYCLE - 1, &c)) continue;
                while (pop()) {}
                fits = pfnl::ring_admit_all(T, batch, cap, pfnl::TC_CYCLE - 1, &c);
            }
            std::printf("R %d %d | %d %d\n", T, batch, (int)pfnl::telecine_ring_fits(batch), (int)fits);
        }
    const int hs[4] = {8, 9, 18, 0};
    for (int mode = -1; mode <= 3; ++mode)
        for (int order = 0; order <= 2; order += 2 - (mode == 1))
            for (int h : hs)
                for (int yuv = 0; yuv < 2; ++yuv)
                    for (int batch = 1; batch <= 2; ++batch) {
                        const char* why = pfnl::telecine_refused(mode, order, h, yuv != 0, PFNL_CHROMA_420, PFNL_PACK_NONE, batch);
                        std::printf("X %d %d %d %d %d | %s\n", mode, order, h, yuv, batch, why ? why : "ok");
                    }
    const pfnl_telecine_params given[4] = {{10, 1, -1}, {0, 1, 5}, {255, 0, 0}, {10, 2, 1}};
    for (const auto& g : given) {
        pfnl_telecine_params q;
        const char* why = pfnl::telecine_params_refused(&g, 540, 1920, &q);
        std::printf("P %d %d %lld | %d %d %lld %s\n", g.threshold, g.post, g.comb_limit, q.threshold, q.post, q.comb_limit, why ? "refused" : "ok");
    }
    pfnl_telecine_params q;
    const char* why = pfnl::telecine_params_refused(nullptr, 4, 12, &q);
    std::printf("P - - - | %d %d %lld %s\n", q.threshold, q.post, q.comb_limit, why ? "refused" : "ok");
    return 0;
}
"""


def _cxx():
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build's own clang++ is the last candidate)"
    return cxx


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("telecine")
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


def test_telecine_geom_walks_the_rule(geom):
    from pfnl_amd import ops  # noqa: F401  (the package imports without a device)
    assert geom["K"] == [([str(TC.CYCLE)], [])]
    for (n_frames, n), fields in geom["F"]:
        assert tuple(int(v) for v in fields) == TC.match_fields(int(n), int(n_frames))
    assert len(geom["Y"]) == 2 * 13
    for (mode, pushed), (made, with_end, open_, ended, cycle) in geom["Y"]:
        name, pushed = TC.MODES[int(mode) - 1], int(pushed)
        assert int(made) == int(open_) == TC.deliverable(name, pushed, False)
        assert int(with_end) == int(ended) == TC.deliverable(name, pushed, True)
        assert int(cycle) == pushed // TC.CYCLE
    assert len(geom["M"]) == 5 * 6 * 2
    for (j, d, carry0), vals in geom["M"]:
        want, carry = TC.place_marks([i == int(j) for i in range(5)], None if int(d) < 0 else int(d), bool(int(carry0)))
        assert [int(v) for v in vals] == [len(want), int(carry)] + [int(m) for m in want]
    for d, (at,) in geom["D"]:
        assert int(at) == TC.drop_index([int(v) for v in d])
    assert len(geom["R"]) == 4 * 5
    for (T, b), (rule, walked) in geom["R"]:                             # the closed condition is what walking the bound finds
        assert rule == walked == str(int(int(b) >= 2)), (T, b)
    seen = set()
    for (mode, order, h, is_yuv, batch), why in geom["X"]:
        mode, order, h, is_yuv, batch = int(mode), int(order), int(h), int(is_yuv), int(batch)
        why = " ".join(why)
        seen.add(why)
        if not 0 <= mode <= 2 or order not in (0, 1):
            assert why != "ok"
            continue
        try:
            stream.telecine_arguments(((None,) + TC.MODES)[mode], D.FIELD_ORDERS[order], None, h, 12,
                                      "i420" if is_yuv else "rgb24")
            ok = not (mode == 2 and batch == 1)                          # (the keywords do not know the batch: the library refuses it)
        except ValueError:
            ok = False
        assert ok == (why == "ok"), (mode, order, h, is_yuv, batch, why)
    assert any("multiple of 4" in w for w in seen) and any("larger batch" in w for w in seen) and "ok" in seen
    got = [(" ".join(a), " ".join(b)) for a, b in geom["P"]]
    assert got == [("10 1 -1", f"10 1 {(540 * 3 * 1920) >> 8} ok"), ("0 1 5", "0 1 5 refused"), ("255 0 0", "255 0 0 ok"), ("10 2 1", "10 2 1 refused"),
                   ("- - -", "10 1 0 ok")]
    assert TC.params(540, 1920) == (10, 1, (540 * 3 * 1920) >> 8) and TC.params(4, 12) == (10, 1, 0)


# ---- the library without a device -----------------------------------------------------------------------------------------------------------
def test_deliverable_is_the_rule():
    lib = _capi.load_library()
    n = C.c_longlong(-1)
    for mode, name in ((1, "match"), (2, "decimate")):
        for pushed in range(13):
            for ended in (0, 1):
                assert lib.pfnl_telecine_deliverable(mode, pushed, ended, C.byref(n)) == 0
                assert n.value == TC.deliverable(name, pushed, bool(ended)), (name, pushed, ended)
    assert lib.pfnl_telecine_deliverable(0, 5, 0, C.byref(n)) == -1 and lib.pfnl_telecine_deliverable(3, 5, 0, C.byref(n)) == -1
    assert lib.pfnl_telecine_deliverable(1, -1, 0, C.byref(n)) == -1 and lib.pfnl_telecine_deliverable(1, 5, 0, None) == -1


def test_the_hooks_refuse_before_any_hip_call():
    lib = _capi.load_library()
    d = C.c_void_p(64)                                                   # never dereferenced: the hooks return first
    for hook in (lib.pfnl_op_fieldmatch_u8, lib.pfnl_op_fieldmatch_u10):
        for at, name in enumerate((b"A", b"Xc", b"Xp")):
            args = [d, d, d, 2, 2, 0, 10, d, None]
            args[at] = None
            assert hook(*args) == -1 and name + b" is NULL" in lib.pfnl_last_error()
        assert hook(d, d, d, 2, 2, 0, 10, None, None) == -1 and b"is NULL" in lib.pfnl_last_error()
        assert hook(d, d, d, 0, 2, 0, 10, d, None) == -1 and b"h must be" in lib.pfnl_last_error()
        assert hook(d, d, d, 2, 0, 0, 10, d, None) == -1 and b"W must be" in lib.pfnl_last_error()
        assert hook(d, d, d, 1 << 30, 1 << 30, 0, 10, d, None) == -1 and b"2^32" in lib.pfnl_last_error()
        for parity in (-1, 2):
            assert hook(d, d, d, 2, 2, parity, 10, d, None) == -1 and b"parity" in lib.pfnl_last_error()
        for thr in (0, 256):
            assert hook(d, d, d, 2, 2, 0, thr, d, None) == -1 and b"threshold" in lib.pfnl_last_error()
        assert hook(d, d, d, 2, 2, 0, 10, C.c_void_p(68), None) == -1 and b"8-byte" in lib.pfnl_last_error()
    assert lib.pfnl_op_fieldmatch_u10(d, C.c_void_p(65), d, 2, 2, 0, 10, d, None) == -1 and b"Xc" in lib.pfnl_last_error()
    bad = _capi.pfnl_telecine_params(10, 2, -1)
    for hook in (lib.pfnl_op_telecine_frame_u8, lib.pfnl_op_telecine_frame_u10):
        assert hook(d, d, d, 2, 2, 0, None, None, d, None) == -1 and b"out is NULL" in lib.pfnl_last_error()
        assert hook(d, d, d, 2, 2, 0, None, d, None, None) == -1 and b"is NULL" in lib.pfnl_last_error()
        assert hook(d, d, d, 2, 2, 0, C.byref(bad), d, d, None) == -1 and b"post" in lib.pfnl_last_error()
        # out [2 h][W][3] = 24 samples touches a field of 12: its head inside A, its tail inside Xc
        assert hook(C.c_void_p(64), C.c_void_p(512), C.c_void_p(1024), 2, 2, 0, None, C.c_void_p(64 + 10), C.c_void_p(2048), None) == -1
        assert b"overlaps" in lib.pfnl_last_error()
        assert hook(C.c_void_p(512), C.c_void_p(64), C.c_void_p(1024), 2, 2, 0, None, C.c_void_p(64 - 20), C.c_void_p(2048), None) == -1
        assert b"overlaps" in lib.pfnl_last_error()
    assert lib.pfnl_stream_telecine(None, 1, 0, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_telecine_stats(None, (C.c_longlong * 5)()) == -1
    assert lib.pfnl_version() == 4                                       # additions to version 4


def test_the_keywords_refuse_what_the_library_refuses():
    assert stream.telecine_arguments() == (0, 0, (10, 1, 0))
    assert stream.telecine_arguments("decimate", "bff", {"threshold": 12, "post": False}, 16, 20) == (2, 1, (12, 0, (8 * 60) >> 8))
    for bad in ({"telecine": "both"}, {"telecine": "match", "field_order": "top"}, {"telecine": "match", "H": 9},
                {"telecine": "decimate", "H": 18, "pixel_format": "i420"}, {"telecine": "match", "interlaced": "field"},
                {"telecine": "match", "telecine_params": {"threshold": 0}}, {"telecine": "match", "telecine_params": {"limit": 1}}):
        with pytest.raises(ValueError):
            stream.telecine_arguments(**bad)
    assert stream.telecine_arguments("decimate", H=18, pixel_format="i420", chroma="422")[0] == 2      # only 4:2:0 splits chroma rows
    assert stream.telecine_arguments(None, interlaced="field")[0] == 0


# ---- Y4M and the two loops --------------------------------------------------------------------------------------------------------------------
def test_y4m_film_rate_and_the_keywords():
    ntsc = y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H480 F30000:1001 It A10:11 C420mpeg2", interlaced=True)
    out = ntsc.for_output(2880, 1920, progressive=True, film_rate=True)
    assert out.to_bytes() == b"YUV4MPEG2 W2880 H1920 F24000:1001 Ip A10:11 C420mpeg2\n"
    assert ntsc.for_output(2880, 1920, progressive=True).rate == "30000:1001"
    assert y4m.Y4MHeader.parse(b"YUV4MPEG2 W8 H8 F30:1 Ib", interlaced=True).for_output(8, 8, film_rate=True).rate == "24:1"
    assert y4m.Y4MHeader.parse(b"YUV4MPEG2 W8 H8 F25:1 Ib", interlaced=True).for_output(8, 8, film_rate=True).rate == "20:1"
    for tag, order in (("t", "tff"), ("b", "bff")):
        h = y4m.Y4MHeader.parse(f"YUV4MPEG2 W720 H480 F30000:1001 I{tag}".encode(), interlaced=True)
        kw = upscale.session_keywords(h, ivtc="decimate")
        assert (kw["telecine"], kw["field_order"]) == ("decimate", order) and "interlaced" not in kw
        assert upscale.session_keywords(h, ivtc="match")["telecine"] == "match"
        with pytest.raises(ValueError, match="exclusive"):
            upscale.session_keywords(h, ivtc="match", deinterlace="frame")
        with pytest.raises(ValueError, match=f"I{tag}"):
            upscale.session_keywords(h)
        with pytest.raises(ValueError):
            upscale.session_keywords(h, telecine="match")                # comes from the header and --ivtc
    prog = y4m.Y4MHeader.parse(b"YUV4MPEG2 W720 H480 F24000:1001 Ip", interlaced=True)
    assert "telecine" not in upscale.session_keywords(prog, ivtc="decimate")                 # a progressive stream ignores it
    a = upscale.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--ivtc", "--no-decimate", "--batch", "2"])
    assert a.ivtc and a.no_decimate and not upscale.parser().parse_args(["-", "-", "--synthetic-weights", "0"]).ivtc
    a = rawvideo.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--in-format", "v210", "--size", "1080x1920", "--ivtc", "decimate",
                                      "--field-order", "bff"])
    assert (a.ivtc, a.field_order) == ("decimate", "bff")


class _Stub:
    """a session that delivers what pfnl_telecine_deliverable says it has made, a cycle at a time"""
    made = []

    def __init__(self, H, W, batch, **kw):
        self.kw, self.H, self.W, self.scale, self.out_size, self.out_chroma_siting = kw, H, W, 4, None, kw.get("out_chroma_siting", "left")
        self.count = self.given = 0
        _Stub.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _frames(self, ended):
        upto = TC.deliverable(self.kw["telecine"], self.count, ended) if "telecine" in self.kw else (self.count if ended else self.count - 1)
        out = []
        while self.given < upto:
            out.append((self.given, np.full(self.out_samples, self.given % 251, self.out_dtype)))
            self.given += 1
        return out

    def push(self, frame):
        self.count += 1
        return self._frames(False)

    def end(self):
        return self._frames(True)


@pytest.mark.parametrize("mode,pushed,frames", [(None, 7, 7), ("match", 7, 7), ("decimate", 7, 6), ("decimate", 10, 8), ("decimate", 4, 4)])
def test_upscale_and_rawvideo_count_film_frames(mode, pushed, frames):
    H, W = 8, 12
    _Stub.out_samples, _Stub.out_dtype = 16 * H * W * 3 // 2, np.uint8
    src = io.BytesIO()
    wr = y4m.Y4MWriter(src, y4m.Y4MHeader(W, H, "30000:1001", "t" if mode else "p", interlaced_ok=True))
    for i in range(pushed):
        wr.write_frame(np.full(H * W * 3 // 2, i, np.uint8))
    out, log = io.BytesIO(), io.StringIO()
    reader = y4m.Y4MReader(io.BytesIO(src.getvalue()), interlaced=mode is not None)
    assert upscale.upscale(reader, y4m.Y4MWriter(out), _Stub, ivtc=mode, batch=2, log=log) == frames
    kw = _Stub.made[-1].kw
    assert (kw.get("telecine"), kw.get("field_order")) == ((mode, "tff") if mode else (None, None)) and "interlaced" not in kw
    back = y4m.Y4MReader(io.BytesIO(out.getvalue()))                     # progressive: the default reader takes it
    assert back.header.interlace == "p" and back.header.rate == ("24000:1001" if mode == "decimate" else "30000:1001")
    assert len(list(back)) == frames and f"{frames} frames" in log.getvalue()
    _Stub.out_samples = P.frame_bytes("uyvy422", 4 * H, 4 * W)
    raw = rawvideo.RawReader(io.BytesIO(bytes(pushed * P.frame_bytes("yuyv422", H, W))), "yuyv422", H, W)
    out = io.BytesIO()
    film = {} if mode is None else {"telecine": mode, "field_order": "bff"}
    assert rawvideo.run(raw, rawvideo.RawWriter(out), _Stub, out_format="uyvy422", batch=2, log=log, **film) == frames
    kw = _Stub.made[-1].kw
    assert (kw.get("telecine"), kw.get("field_order"), kw["packing"]) == ((mode, "bff", "yuyv422") if mode else (None, None, "yuyv422"))
    assert len(out.getvalue()) == frames * _Stub.out_samples
