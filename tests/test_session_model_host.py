"""tests/session_model.py checked where it can be, without a device: the pairwise array covers every legal pair within its row cap and is
the same on every call, ``legal`` refuses what include/pfnl_hip.h says is refused, ``expected`` gives frames of the right layout for every
row and no factor outside ``base`` is vacuous in it, and three faults seeded in the MODEL - the wrong field order, a siting on the wrong
side, placement taps clamped at the frame instead of at the source rectangle - each change its bytes on some row."""
import itertools

import numpy as np
import pytest

import session_model as M
from pfnl_amd import fit, packed, resize, stream

ROWS = M.covering_rows()


# ---- the array ------------------------------------------------------------------------------------------------------------------------------
def _exists(i, a, j, b):
    """is there a legal row with VALUES[i] = a and VALUES[j] = b?  The defaults first, then every input side, output side and size"""
    for k in itertools.product(M.IN_VALUES, M.OUT_VALUES, M.SIZES):
        row = list(M.with_(M.DEFAULT, in_=k[0], out=k[1], size=k[2]))
        row[i], row[j] = a, b
        if M.legal(M.Row(*row)):
            return True
    return False


def test_every_row_is_legal_and_every_legal_pair_is_covered():
    assert all(M.legal(r) for r in ROWS)
    for r in ROWS:
        M.arguments(r)                                                   # (the validators themselves, past the cache of ``legal``)
    n = len(M.FACTORS)
    held = {(i, j): {(r[i], r[j]) for r in ROWS} for i, j in itertools.combinations(range(n), 2)}
    pairs, missing = 0, []
    for (i, j), got in held.items():
        for a, b in itertools.product(M.VALUES[M.FACTORS[i]], M.VALUES[M.FACTORS[j]]):
            row = list(M.DEFAULT)
            row[i], row[j] = a, b
            if M.legal(M.Row(*row)) or ({i, j} <= {0, 1, 8} and _exists(i, a, j, b)):   # (in, out and size alone constrain each other)
                pairs += 1
                if (a, b) not in got:
                    missing.append((M.FACTORS[i], a, M.FACTORS[j], b))
            else:
                assert (a, b) not in got
    assert not missing, missing[:5]
    assert pairs == len(M.legal_pairs()) == 3288
    in_out = sum(1 for a, b in itertools.product(M.IN_VALUES, M.OUT_VALUES) if M.legal(M.with_(M.DEFAULT, in_=a, out=b)))
    assert in_out == 23 * 23 - 16 * 3 == 481                             # the 16 YUV inputs against the three rgb10-family outputs
    assert len(M.VALUES["in"]) == len(M.VALUES["out"]) == 23 == max(len(v) for v in M.VALUES.values())
    assert len(ROWS) <= 1.1 * in_out, len(ROWS)
    print(f"{len(ROWS)} rows, {pairs} legal pairs, {in_out} of them in x out")


def test_two_calls_return_the_same_rows():
    make = M.covering_rows.__wrapped__                                   # (past the cache)
    assert make() == make() == ROWS


def test_the_walks_keys_partition_the_rows():
    keys = M.walk_keys(ROWS)
    assert sorted(keys) == [(f, b) for f in (False, True) for b in (1, 2, 3)]
    assert sum(len(v) for v in keys.values()) == len(ROWS) and all(len(v) >= 16 for v in keys.values())


# ---- legal ----------------------------------------------------------------------------------------------------------------------------------
def _why(row, h=M.H):
    with pytest.raises(ValueError) as e:
        M.arguments(row, h)
    assert not M.legal(row) or h != M.H
    return str(e.value)


def test_legal_refuses_by_name():
    D = M.DEFAULT
    for in_ in M.IN_VALUES:
        for out in (("rgb10", "420", None), ("rgb10", "420", "x2rgb10"), ("rgb10", "420", "x2bgr10")):
            assert M.legal(M.with_(D, in_=in_, out=out)) == (in_[0] == "rgb24")
    assert "goes with pixel_format 'rgb24'" in _why(M.with_(D, in_=("nv12", 8, "420", None), out=("rgb10", "420", None)))
    for out in M.OUT_VALUES:                                             # odd sizes into subsampled outputs
        yuv_out = out[0] in ("nv12", "i420", "p010", "i010")
        assert M.legal(M.with_(D, out=out, size="odd")) == (not yuv_out or (out[1] == "444" and out[2] is None)), out
    assert "even sizes" in _why(M.with_(D, out=("nv12", "420", None), size="odd"))
    assert "even width" in _why(M.with_(D, out=("i010", "422", None), size="odd"))
    # each packing on a wrong family, depth or chroma
    for name, (is_yuv, bits, _, _, _) in packed.TABLE.items():
        good = ("nv12", bits, "422", name) if is_yuv else ("rgb24", bits, "420", name)
        assert M.legal(M.with_(D, in_=good))
        assert "family" in _why(M.with_(D, in_=("rgb24" if is_yuv else "nv12", bits, "422", name)))
        assert "depth" in _why(M.with_(D, in_=(good[0], 18 - bits, good[2], name)))
        fmt = ("nv12" if bits == 8 else "p010") if is_yuv else ("rgb24" if bits == 8 else "rgb10")
        assert M.legal(M.with_(D, out=(fmt, "422", name)))
        assert "family" in _why(M.with_(D, out=(("rgb24" if bits == 8 else "rgb10") if is_yuv else ("nv12" if bits == 8 else "p010"), "422", name)))
        assert "depth" in _why(M.with_(D, out=({"nv12": "p010", "p010": "nv12", "rgb24": "rgb10", "rgb10": "rgb24"}[fmt], "422", name)))
        if is_yuv:
            assert "PFNL_CHROMA_422" in _why(M.with_(D, in_=("nv12", bits, "420", name)))
            assert "PFNL_CHROMA_422" in _why(M.with_(D, out=(fmt, "444", name)))
    with pytest.raises(ValueError, match="multiple of 6"):               # v210 on a width that 6 does not divide
        stream.packing_arguments(None, "v210", "rgb24", "p010", 8, "420", "422", M.W, 100)
    with pytest.raises(ValueError, match="multiple of 6"):
        M.arguments(M.with_(D, in_=("nv12", 10, "422", "v210")), M.H, 20)
    for size in M.SIZES:                                                 # every width but the odd one keeps v210 out legal
        assert M.legal(M.with_(D, out=("p010", "422", "v210"), size=size)) == (size != "odd")
    assert "multiple of 4" in _why(M.with_(D, in_=("i420", 8, "420", None), interlace=("frame", "tff")), 18)
    M.arguments(M.with_(D, in_=("i420", 8, "422", None), interlace=("frame", "tff")), 18)
    for bad in (M.with_(D, ensemble=3), M.with_(D, tiling=(11, 16, 2, 0)), M.with_(D, pop="file"), M.with_(D, batch=4)):
        assert not M.legal(bad)


# ---- expected -------------------------------------------------------------------------------------------------------------------------------
def _expected(row):
    return M.expected(row, M.pushed_frames(row), M.standin_base)


def test_expected_has_the_rows_layout_for_every_row():
    for row in ROWS:
        got = _expected(row)
        n = 2 * M.F if row.interlace and row.interlace[0] == "field" else M.F
        assert [i for i, _ in got] == list(range(n)), row
        oH, oW = M.arguments(row)["canvas"]
        of, out_chroma, out_pack = row.out
        if out_pack is not None:
            shape, dtype = packed.frame_shape(out_pack, oH, oW), np.uint8
        else:
            shape, dtype = stream.frame_shapes(of, oH, oW, out_chroma)[0], stream.frame_dtype(of)
        assert all(f.shape == shape and f.dtype == dtype for _, f in got), (row, got[0][1].shape, shape)
        pushed = M.pushed_frames(row)
        pf, depth, chroma, pack = row.in_
        for f in pushed:                                                 # ... and what is pushed is what push takes
            if pack is not None:
                stream.packed_frame_argument(f, pack, M.H, M.W)
            else:
                stream.frame_argument(f, pf, M.H, M.W, depth, chroma)
        assert [p.shape[1] * p.dtype.itemsize for p in M.in_planes(row, pushed[0])] == [n for _, n in _in_plane_bytes(row)]


def _in_plane_bytes(row):
    from pfnl_amd import surface
    pf, depth, chroma, pack = row.in_
    return [(r, n * dt.itemsize) for r, n, dt in surface.plane_shapes(stream.pushed_format(pf, depth), M.H, M.W, chroma, pack)]


def _differs(a, b):
    return len(a) != len(b) or any(x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y) for (_, x), (_, y) in zip(a, b))


@pytest.mark.parametrize("factor", M.OUTSIDE_BASE)
def test_no_factor_outside_base_is_vacuous(factor):
    name = "in_" if factor == "in" else factor
    for row in ROWS:
        for v in M.VALUES[factor]:
            other = M.with_(row, **{name: v})
            if v == row.get(factor) or not M.legal(other):
                continue
            if _differs(_expected(row), _expected(other)):              # (the same picture, pushed the other row's way)
                return
    raise AssertionError(f"no row's expected bytes change with {factor} alone")


def test_matrix_range_and_siting_act_on_the_bytes_that_are_pushed():
    """the decode of the SAME pushed bytes changes with each input-side setting (above, a row's own encoding may undo its own decode)"""
    row = M.with_(M.DEFAULT, in_=("i420", 8, "420", None))
    pushed = M.pushed_frames(row)
    for change in ({"matrix": "bt601"}, {"full_range": True}, {"chroma_siting": "center"}, {"chroma_siting": "topleft"},
                   {"interlace": ("frame", "tff")}, {"interlace": ("field", "bff")}):
        a, b = M.ring_frames(row, pushed), M.ring_frames(M.with_(row, **change), pushed)
        assert len(a) != len(b) or any(not np.array_equal(x, y) for x, y in zip(a, b)), change


# ---- seeded faults in the model -------------------------------------------------------------------------------------------------------------
def _caught(monkeypatch, patch, rows):
    """does the unmodified model tell itself from the model with ``patch`` applied, on at least one of ``rows``?"""
    plain = [_expected(r) for r in rows]
    patch(monkeypatch)
    return sum(_differs(a, _expected(r)) for a, r in zip(plain, rows))


def test_the_wrong_field_order_is_caught(monkeypatch):
    rows = [r for r in ROWS if r.interlace][:12]
    frames = M.deinterlace.frames

    def patch(mp):
        mp.setattr(M.deinterlace, "frames", lambda woven, order="tff", *rest: frames(woven, "bff" if order == "tff" else "tff", *rest))
    assert _caught(monkeypatch, patch, rows) == len(rows)


def test_a_siting_on_the_wrong_side_is_caught(monkeypatch):
    rows = [r for r in ROWS if r.in_[0] != "rgb24" and r.in_[2] != "444" and r.interlace is None
            and yuv_axes(r.chroma_siting, r.in_[2]) != yuv_axes(r.out_chroma_siting, r.in_[2])][:12]
    assert len(rows) >= 4
    ring = M.ring_frames

    def patch(mp):                                                       # the decode reads the OUTPUT side's siting
        mp.setattr(M, "ring_frames", lambda row, pushed, h=M.H: ring(M.with_(row, chroma_siting=row.out_chroma_siting), pushed, h))
    assert _caught(monkeypatch, patch, rows) == len(rows)


def yuv_axes(siting, chroma):
    """what of a siting a chroma format reads: (vertical, horizontal) at 4:2:0, the horizontal half at 4:2:2"""
    from pfnl_amd import yuv
    v, h = yuv.AXES[siting]
    return (v, h) if chroma == "420" else (h,)


def _axis_at_frame(n_in, n_out, offset, n_frame):
    """resize._row's taps of a source of n_in samples that begins at ``offset`` of a line of n_frame - with every tap's index clamped at
    the LINE's ends, not at the source's: [(indices, coefficients)] per output sample"""
    d = 2 * max(n_in, n_out)
    out = []
    for o in range(n_out):
        centre = n_in * (2 * o + 1)
        j = (centre - 2 * d - n_out) // (2 * n_out)
        at, w = [], []
        while True:
            j += 1
            n = n_out * (2 * j + 1) - centre
            if n >= 2 * d:
                break
            if n <= -2 * d:
                continue
            at.append(min(max(offset + j, 0), n_frame - 1))
            w.append(resize._weight(abs(n), d))
        s = sum(w)
        c = [(2 * x * resize.ONE + s) // (2 * s) for x in w]
        c[c.index(max(c))] += resize.ONE - sum(c)
        out.append((np.array(at), np.array(c, np.int64)))
    return out


def _place_clamped_at_the_frame(frame, out_h, out_w, src=None, dst=None, fill=(0, 0, 0)):
    frame = np.asarray(frame)
    Hf, Wf = frame.shape[:2]
    (sy, sx, sh, sw), (dy, dx, dh, dw) = fit.as_rect(src, "src", Hf, Wf), fit.as_rect(dst, "dst", out_h, out_w)
    x = frame.astype(np.int64)
    h = np.stack([(x[:, at] * c[None, :, None]).sum(axis=1) for at, c in _axis_at_frame(sw, dw, sx, Wf)], axis=1)
    h = (h + (1 << 7)) >> 8
    v = np.stack([(h[at] * c[:, None, None]).sum(axis=0) for at, c in _axis_at_frame(sh, dh, sy, Hf)], axis=0)
    canvas = np.empty((out_h, out_w, 3), np.uint8)
    canvas[:] = np.asarray(fill, np.uint8)
    canvas[dy:dy + dh, dx:dx + dw] = np.clip((v + (1 << 19)) >> 20, 0, 255).astype(np.uint8)
    return canvas


def test_the_mutant_placement_is_the_rule_where_the_source_is_the_frame():
    """the seeded fault is that and no other: with src the whole frame the two clamps are one"""
    f = np.random.default_rng(3).integers(0, 256, (20, 30, 3), dtype=np.uint8)
    for args in ((25, 36, None, None), (31, 40, None, (3, 2, 24, 30)), (12, 18, None, (1, 1, 10, 16))):
        assert np.array_equal(_place_clamped_at_the_frame(f, *args, (9, 8, 7)), fit.place(f, *args, (9, 8, 7)))
    assert not np.array_equal(_place_clamped_at_the_frame(f, 20, 30, (4, 6, 12, 18)), fit.place(f, 20, 30, (4, 6, 12, 18)))


def test_placement_taps_clamped_at_the_frame_are_caught(monkeypatch):
    rows = [r for r in ROWS if r.size == "place" and M.out_depth(r) == 8][:12]   # ("crop" alone is delivered 1 : 1: one tap, no clamp)
    assert len(rows) >= 4

    def patch(mp):
        mp.setattr(M.fit, "place", _place_clamped_at_the_frame)
    assert _caught(monkeypatch, patch, rows) == len(rows)
