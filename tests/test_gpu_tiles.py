"""The tiled forward on a real MI355X (include/pfnl_hip.h TILES; pfnl_amd/csrc/tiles.hip): the two kernels and pfnl_forward_tiled against
the host rule pfnl_amd/tiles.py, byte for byte - a tiled forward is defined by the existing forward and that rule, so the composition of
plain forwards on the same engine is the reference; the oracle bounds the whole once, with the margin the trunk needs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_ensemble as TE  # noqa: E402   (_Arena, _engine, _dev, _same, _bits, SENTINEL)
import test_gpu_forward as TF  # noqa: E402   (ABS_TOL)
from oracle import pfnl_fast  # noqa: E402
from pfnl_amd import _capi, ops, scene, synth, tiles  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

NB = TE.NB
SPECIALS = np.array([0.0, -0.0, 1e-42, np.inf, -np.inf], np.float32)             # bits a copy must keep: the sign of zero, a denormal, inf

# (B,T,H,W), tile: 16-byte words, a shifted last tile on both axes, B > 1 | origins 34 and 8 pixels: 8-byte words | one tile, narrower than a wave
KERNEL_CASES = [((2, 7, 20, 36), (12, 16, 2)), ((1, 5, 34, 66), (14, 32, 4)), ((1, 7, 6, 10), (0, 0, 0))]


def _values(shape, seed):
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    flat = x.ravel()
    flat[::97] = np.resize(SPECIALS, flat[::97].shape)                           # in every tile and every run
    return x


def _runs_to_try(total):
    """all tiles at once; of the runs of 5, a middle one and the short last one"""
    rs = tiles.runs(total, 5)
    return [(0, total)] + ([rs[1], rs[-1]] if len(rs) > 2 else [])


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])             # shifted: dst one float off 16 bytes - the 4-byte words
@pytest.mark.parametrize("shape,tile", KERNEL_CASES)
def test_tile_gather_equals_the_host_rule(shape, tile, shift):
    x = _values(shape + (3,), sum(shape))
    stack = tiles.split(x, tile)
    if shape[0] == 2:
        assert _runs_to_try(len(stack)) == [(0, 12), (5, 5), (10, 2)]
    for first, count in _runs_to_try(len(stack)):
        want = stack[first:first + count]
        a = TE._Arena(x, want.shape, shift=shift)
        out = ops.tile_gather(a.src, tile, first, count, out=a.dst)
        assert out.data_ptr() == a.dst.data_ptr()
        got = a.check().reshape(want.shape)
        assert TE._same(got, want), (first, count, int((TE._bits(got) != TE._bits(want)).sum()))
    if shift == 0:
        assert TE._same(ops.tile_gather(TE._dev(x), tile).cpu().numpy(), stack)  # a tensor of its own, every tile
        off = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")[1:].view(x.shape).copy_(TE._dev(x))   # the source one float off instead
        assert TE._same(ops.tile_gather(off, tile).cpu().numpy(), stack)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("shape,tile", KERNEL_CASES)
def test_tile_scatter_equals_the_host_rule(shape, tile, scale, shift):
    B, _, H, W = shape
    th, tw, rows, cols = tiles.grid(H, W, tile)
    total = B * len(rows) * len(cols)
    y = _values((total, scale * th, scale * tw, 3), sum(shape) + scale)
    full = tiles.assemble(y, B, H, W, scale, tile)
    owner = tiles.assemble(np.broadcast_to(np.arange(total, dtype=np.int64)[:, None, None, None], y.shape[:-1] + (1,)), B, H, W, scale, tile)
    assert full.shape == (B, scale * H, scale * W, 3) and set(owner.ravel()) == set(range(total))
    for first, count in _runs_to_try(total):
        mine = (owner >= first) & (owner < first + count)
        want = np.where(mine, full, TE.SENTINEL)                                 # what other tiles own stays as it was
        a = TE._Arena(y[first:first + count], full.shape, shift=shift)
        out = ops.tile_scatter(a.src, a.dst, tile, scale, first)
        assert out.data_ptr() == a.dst.data_ptr()
        got = a.check().reshape(full.shape)
        assert TE._same(got, want), (first, count, int((TE._bits(got) != TE._bits(want)).sum()))


def test_ops_refuse_bad_arguments():
    x = torch.zeros((2, 7, 20, 36, 3), device="cuda")
    with pytest.raises(ValueError):
        ops.tile_gather(x, (12, 16, 6))
    with pytest.raises(ValueError):
        ops.tile_gather(x, (12, 16, 2), first=10, count=3)                       # 12 tiles
    with pytest.raises(ValueError):
        ops.tile_gather(x, (12, 16, 2), out=torch.zeros((12, 7, 12, 12, 3), device="cuda"))
    with pytest.raises(ValueError):
        ops.tile_gather(x[0], (12, 16, 2))
    out = torch.zeros((2, 80, 144, 3), device="cuda")
    with pytest.raises(ValueError):
        ops.tile_scatter(torch.zeros((2, 48, 48, 3), device="cuda"), out, (12, 16, 2), 4)
    with pytest.raises(ValueError):
        ops.tile_scatter(torch.zeros((13, 48, 64, 3), device="cuda"), out, (12, 16, 2), 4)
    assert ops.tile_scatter(torch.zeros((2, 1, 48, 64, 3), device="cuda"), out.view(2, 1, 80, 144, 3), (12, 16, 2), 4, first=10).shape == (2, 1, 80, 144, 3)


# ---- the forward ---------------------------------------------------------------------------------------------------------------------
def _plain(eng, n=1):
    """the forward of `eng` on device tensors, numpy in and out: the f of the composition"""
    return lambda a: eng.forward(TE._dev(a), ensemble=n).cpu().numpy()


CASES = {"T7": (PFNLGeometry(num_block=NB), "fp32", (2, 7, 20, 36), (12, 16, 2), (0, 4, 5)),      # 12 tiles: whole runs, a short last run
         "T5x2": (PFNLGeometry(num_frames=5, scale=2, num_block=NB), "fp32", (1, 5, 12, 20), (8, 12, 2), (0, 3)),
         "bf16": (PFNLGeometry(num_block=NB), "bf16", (2, 7, 20, 36), (12, 16, 2), (5,))}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_tiled_is_the_composition_of_forwards(case):
    geom, precision, (B, T, H, W), tile, batches = CASES[case]
    eng = TE._engine(geom, precision)
    x = synth.uniform_clips(B, T, H, W, seed=41)
    xd = TE._dev(x)
    whole = eng.forward(xd).cpu().numpy()
    for batch in batches:
        t = tile + (batch,)
        want = tiles.forward_tiled(_plain(eng), x, t)
        got = eng.forward(xd, tile=t)
        assert torch.is_tensor(got) and got.is_cuda
        got = got.cpu().numpy()
        assert got.shape == whole.shape and np.isfinite(got).all()
        assert TE._same(got, want), (case, batch, int((TE._bits(got) != TE._bits(want)).sum()), float(np.abs(got - want).max()))
        assert not TE._same(got, whole)                                          # the non-local block saw its tile
        print(f"\n[tiles] {case} batch={batch}: max |tiled - whole| {np.abs(got - whole).max():.3g}", end="")
    t = tile + (batches[-1],)
    want = tiles.forward_tiled(_plain(eng), x, t)
    eng.tile = t                                                                 # the engine's default tiling
    assert TE._same(eng.forward(xd).cpu().numpy(), want)
    out = torch.empty(eng.out_shape(B, H, W), dtype=torch.float32, device="cuda")
    eng.forward_device(xd.data_ptr(), out.data_ptr(), B, H, W)                   # ... which forward_device does not read
    assert TE._same(out.cpu().numpy(), whole)
    eng.forward_device(xd.data_ptr(), out.data_ptr(), B, H, W, tile=t)
    assert TE._same(out.cpu().numpy(), want)
    eng.tile = None
    eng.sync()                                                                   # no run left a range flag
    with pytest.raises(ValueError):
        eng.forward(xd, tile=tile[:2] + (tile[0] // 2,))
    eng.close()


def test_forward_tiled_with_an_ensemble_and_host_pointers():
    eng = TE._engine()
    x = synth.uniform_clips(2, 7, 20, 36, seed=42)
    t = (12, 16, 2, 5)
    want2 = tiles.forward_tiled(_plain(eng, 2), x, t)                            # every run a pfnl_forward_ensemble of 2
    assert TE._same(eng.forward(TE._dev(x), ensemble=2, tile=t).cpu().numpy(), want2)
    assert not TE._same(want2, tiles.forward_tiled(_plain(eng), x, t))
    # numpy in, numpy out (staging inside the call) against the composition of host-pointer forwards; a torch CPU tensor likewise
    want = tiles.forward_tiled(lambda a: eng.forward(a), x, t)
    got = eng.forward(x, tile=t)
    assert isinstance(got, np.ndarray) and TE._same(got, want)
    got = eng.forward(torch.from_numpy(x), tile=t)
    assert torch.is_tensor(got) and not got.is_cuda and TE._same(got.numpy(), want)
    assert TE._same(eng.forward(x, ensemble=2, tile=t), tiles.forward_tiled(lambda a: eng.forward(a, ensemble=2), x, t))
    assert eng.range_reruns() == 0
    eng.close()


def test_the_degenerate_tiling_is_the_forward():
    eng = TE._engine()
    x = synth.uniform_clips(2, 7, 20, 36, seed=43)
    xd = TE._dev(x)
    whole = eng.forward(xd).cpu().numpy()
    for t in ((0, 0), (0, 0, 0, 0), (20, 36, 9), (40, 64, 50, 2), (0, 0, 0, 7)):  # one tile per clip, one run
        assert TE._same(eng.forward(xd, tile=t).cpu().numpy(), whole), t
    assert TE._same(eng.forward(x, tile=(0, 0)), eng.forward(x))
    assert TE._same(eng.forward(xd, ensemble=2, tile=(0, 0)).cpu().numpy(), eng.forward(xd, ensemble=2).cpu().numpy())
    # one tile per clip, a clip per run: the general path, whose gather and scatter are plain copies
    assert TE._same(eng.forward(xd, tile=(0, 0, 0, 1)).cpu().numpy(), tiles.forward_tiled(_plain(eng), x, (0, 0, 0, 1)))
    eng.close()


def test_with_the_margin_only_the_nonlocal_block_differs():
    """The non-local block's output projection zeroed: the block is the identity, the network its convolutions, and pad = 4 + 2 num_block
    covers their receptive field - tiled and whole-frame forward agree within the forward bound, and the tiled result meets the oracle's."""
    geom = PFNLGeometry(num_block=NB)
    w = dict(synth.synthetic_weights(geom, seed=0))
    for leaf in ("kernel", "bias"):
        w[f"nlvsr/nlblock_0/w/w/{leaf}"] = np.zeros_like(w[f"nlvsr/nlblock_0/w/w/{leaf}"])
    eng = TE.PFNLEngine(geom, device=0)
    eng.load_weights(w)
    pad = 4 + 2 * NB
    x = synth.uniform_clips(1, 7, 24, 40, seed=44)
    t = (20, 24, pad, 4)                                                         # 2 x 3 tiles, runs of 4 and 2
    assert len(tiles.axis(24, 20, pad)) == 2 and len(tiles.axis(40, 24, pad)) == 3
    whole = eng.forward(TE._dev(x)).cpu().numpy()
    got = eng.forward(TE._dev(x), tile=t).cpu().numpy()
    err = float(np.abs(got - whole).max())
    fo = pfnl_fast.FastOracle(w, num_block=NB)
    ref = tiles.forward_tiled(lambda a: fo.forward(np.ascontiguousarray(a)), x, t)
    err_ref = float(np.abs(got - ref).max())
    bare = float(np.abs(eng.forward(TE._dev(x), tile=(20, 24, 0, 4)).cpu().numpy() - whole).max())
    print(f"\n[tiles] projection zeroed: max |tiled - whole| pad {pad}: {err:.3g}, pad 0: {bare:.3g}; max |tiled - oracle tiled| {err_ref:.3g}", end="")
    assert err < TF.ABS_TOL, err
    assert err_ref < TF.ABS_TOL, err_ref
    assert not bare < TF.ABS_TOL, bare                                           # the margin is what does it
    eng.close()


def test_plain_forward_around_a_tiled_call_is_bit_identical():
    eng = TE._engine()
    x = synth.uniform_clips(2, 7, 20, 36, seed=45)
    xd = TE._dev(x)
    y0 = eng.forward(xd).cpu().numpy()
    yt = eng.forward(xd, ensemble=8, tile=(12, 16, 2, 5)).cpu().numpy()          # the handle runs 12 x 16 and 16 x 12 at 5 and 2 clips in between
    y1 = eng.forward(xd).cpu().numpy()
    assert TE._same(y0, y1) and not TE._same(y0, yt)
    assert TE._same(eng.forward(xd, ensemble=8, tile=(12, 16, 2, 5)).cpu().numpy(), yt)
    assert TE._same(yt, tiles.forward_tiled(_plain(eng, 8), x, (12, 16, 2, 5)))
    eng.close()


# ---- range ---------------------------------------------------------------------------------------------------------------------------
def test_host_pointer_tiled_call_reruns_once_on_the_strict_kernels():
    """x 600 as in test_split16_domain_nonlocal_input_scale (600 * 2^7 > 65504 in the f16 non-local kernel, which runs from 1024 keys on:
    tiles of 64 x 64), in columns that only the second of two tiles holds: that tile alone raises the call's flag; the call reads it once
    behind the last run, redoes BOTH tiles on the f32-MFMA kernels and counts one rerun."""
    eng = TE._engine()
    t = (64, 64, 4, 1)
    assert tiles.axis(120, 64, 4) == [(0, 0, 60), (56, 60, 120)]
    x = synth.uniform_clips(1, 7, 64, 120, seed=5)
    x[..., 64:, :] *= np.float32(600.0)                                          # columns 64 .. 119: in tile 1 (56 .. 119) only
    stack = tiles.split(x, t)
    r0 = eng.range_reruns()
    eng.forward(stack[0:1])
    assert eng.range_reruns() == r0                                              # tile 0 stays inside the range ...
    eng.forward(stack[1:2])
    assert eng.range_reruns() == r0 + 1                                          # ... tile 1 leaves it
    got = eng.forward(x, tile=t)
    assert eng.range_reruns() == r0 + 2 and np.isfinite(got).all()               # one count for the whole call
    strict = TE._engine()
    strict.set_option("strict_fp32", "on")
    want = tiles.forward_tiled(lambda a: strict.forward(a), x, t)
    assert strict.range_reruns() == 0
    assert TE._same(got, want), int((TE._bits(got) != TE._bits(want)).sum())
    eng.sync()                                                                   # nothing left for the asynchronous side
    eng.close()
    strict.close()


# ---- the session ---------------------------------------------------------------------------------------------------------------------
def _stream_all(vs, frames, marks=()):
    got = []
    for k, f in enumerate(frames):
        if k in marks:
            vs.mark_cut()
        got += vs.push(f)
        got += vs.pop_ready()
    got += vs.end()
    assert [i for i, _ in got] == list(range(len(frames)))
    return np.stack([f for _, f in got])


def _explicit(eng, frames_u8, idx, batch, tile):
    """host-built windows through the (tiled) forward and ops.quantise_u8 on the session's batch partition: [F,sH,sW,3] uint8"""
    win = (frames_u8 / 255.).astype(np.float32)[idx]
    outs = []
    for first in range(0, len(idx), batch):
        outs.append(ops.quantise_u8(eng.forward(TE._dev(win[first:first + batch]), tile=tile))[:, 0].cpu().numpy())
    return np.concatenate(outs)


def test_session_runs_every_batch_tiled():
    eng = TE._engine()
    F, H, W, batch, T = 9, 20, 36, 2, 7
    t = (12, 16, 2, 2)
    frames = np.random.default_rng(46).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    cut = 5
    sf = np.array([0] * cut + [cut] * (F - cut), np.int64)                       # one scene cut
    idx_cut, idx_one = scene.scene_windows_index(sf, T), scene.scene_windows_index(np.zeros(F, np.int64), T)
    want_cut, want_one = _explicit(eng, frames, idx_cut, batch, t), _explicit(eng, frames, idx_one, batch, t)
    plain = _explicit(eng, frames, idx_one, batch, None)
    assert not np.array_equal(want_cut, want_one) and not np.array_equal(want_one, plain)
    options = {k: eng.get_option(k) for k in eng.OPTION_KEYS}
    with eng.open_stream(H, W, batch=batch, scene_cut="manual") as vs:
        assert vs.tiling is None
        vs.set_tiling(*t)
        assert vs.tiling == t
        assert vs.push(frames[0]) == []
        assert vs._lib.pfnl_stream_tile(vs._s, C.byref(_capi.pfnl_tiling(12, 16, 2, 0))) == -2      # PFNL_ERR_STATE behind the first push
        assert vs._lib.pfnl_stream_tile(vs._s, None) == -2
        assert vs._lib.pfnl_stream_tile(vs._s, C.byref(_capi.pfnl_tiling(12, 16, 6, 0))) == -1
        with pytest.raises(_capi.PFNLHipError):
            vs.set_tiling(12, 16)
        assert vs.tiling == t
        vs.reset()                                                               # the setting survives
        assert np.array_equal(_stream_all(vs, frames, marks={cut}), want_cut)
        vs.reset()
        assert np.array_equal(_stream_all(vs, frames), want_one)
        vs.reset()
        vs.set_tiling(None, None)                                                # off again: whole frames
        assert vs.tiling is None
        assert np.array_equal(_stream_all(vs, frames), plain)
    with eng.open_stream(H, W, batch=batch, ensemble=2) as vs:                   # with the session's ensemble
        vs.set_tiling(12, 16, pad=2)
        assert vs.tiling == (12, 16, 2, 0)
        want = np.concatenate([ops.quantise_u8(eng.forward(TE._dev((frames / 255.).astype(np.float32)[idx_one][a:a + batch]), ensemble=2, tile=(12, 16, 2)))[:, 0]
                               .cpu().numpy() for a in range(0, F, batch)])
        assert np.array_equal(_stream_all(vs, frames), want)
    with eng.open_stream(H, W, batch=batch) as vs:                               # a session that never calls it
        assert vs.tiling is None
        assert np.array_equal(_stream_all(vs, frames), plain)
        with pytest.raises(ValueError):
            vs.set_tiling(11, 16)
    assert {k: eng.get_option(k) for k in eng.OPTION_KEYS} == options
    eng.close()


# ---- the harness ---------------------------------------------------------------------------------------------------------------------
def test_harness_runs_tiled(tmp_path):
    from PIL import Image
    from model.pfnl import PFNL
    from pfnl_amd import model as M
    F, H, W = 5, 20, 36
    lr_u8 = np.random.default_rng(47).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    seq = tmp_path / "seq"
    (seq / "blur4").mkdir(parents=True)
    for i, im in enumerate(lr_u8):
        Image.fromarray(im).save(seq / "blur4" / f"{i:04d}.png")
    m = PFNL()
    assert m.tile is None
    m.num_block = NB
    m.save_dir = str(tmp_path / "none")
    m.set_weights(synth.synthetic_weights(PFNLGeometry(num_block=NB), seed=0))
    win = np.ascontiguousarray(M.sliding_windows((lr_u8 / 255.).astype(np.float32), 7))
    decoded = {}
    for t in ((12, 16, 2, 5), None):
        m.tile = t
        m.test_video_lr(str(seq), name=f"out{t is None}", part=2)               # 5 frames, part 2 -> batches of 3 and 2
        decoded[t] = np.stack([np.asarray(Image.open(p)) for p in sorted((seq / f"out{t is None}").glob("*.png"))])
    eng = m._get_engine()
    assert eng.tile is None
    for t in decoded:
        f = _plain(eng) if t is None else (lambda a: tiles.forward_tiled(_plain(eng), a, t))   # noqa: B023
        want = np.concatenate([M.quantise(f(win[a:b])[:, 0]) for a, b in ((0, 3), (3, 5))])
        assert decoded[t].shape == want.shape == (F, 4 * H, 4 * W, 3)
        assert np.array_equal(decoded[t], want), t
    assert not np.array_equal(decoded[None], decoded[(12, 16, 2, 5)])
    m.tile = (12, 16, 6)
    with pytest.raises(ValueError):
        m.test_video_lr(str(seq), name="bad", part=2)
