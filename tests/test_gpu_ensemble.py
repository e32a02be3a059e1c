"""Self-ensemble on a real MI355X (include/pfnl_hip.h SELF-ENSEMBLE; pfnl_amd/csrc/dihedral.hip): the two kernels and
pfnl_forward_ensemble against the host rule pfnl_amd/ensemble.py, byte for byte - the ensemble is defined by the existing forward and that
rule, so the composition of plain forwards on the same engine is the reference, and the oracle bounds the whole once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_forward as TF  # noqa: E402   (ABS_TOL)
from oracle import pfnl_fast  # noqa: E402
from pfnl_amd import ensemble, ops, synth, yuv  # noqa: E402
from pfnl_amd import model as M  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

NB = 2
SENTINEL = np.float32(-7.25e9)                    # no operand below comes near it
GAP = 64                                          # floats around every operand of an arena (256 bytes: the operands stay 16-byte aligned)

# [3,6,10,3]: a lane per pixel, H != W, smaller than a tile; [2,34,66,3]: crosses a tile edge on both axes, W % 4 != 0;
# [1,64,128,3]: 16-byte accesses, whole tiles
SHAPES = [(3, 6, 10), (2, 34, 66), (1, 64, 128)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _engine(geom=None, precision="fp32"):
    geom = geom or PFNLGeometry(num_block=NB)
    e = PFNLEngine(geom, device=0)
    e.load_weights(synth.synthetic_weights(geom, seed=0))
    if precision != "fp32":
        e.set_option("precision", precision)
    return e


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _plain(eng):
    """the plain forward of `eng` on device tensors, numpy in and out: the f of the composition"""
    return lambda a: eng.forward(_dev(a), ensemble=1).cpu().numpy()


class _Arena:
    """Operands inside one allocation filled with a sentinel: [GAP | src | GAP (+ shift) | dst | GAP]"""

    def __init__(self, src, dst_shape, dst_init=None, shift=0):
        n_src, n_dst = int(np.prod(src.shape)), int(np.prod(dst_shape))
        self.o_src, self.o_dst = GAP, 2 * GAP + n_src + shift
        self.n_src, self.n_dst = n_src, n_dst
        host = np.full(self.o_dst + n_dst + GAP, SENTINEL, np.float32)
        host[self.o_src:self.o_src + n_src] = src.ravel()
        if dst_init is not None:
            host[self.o_dst:self.o_dst + n_dst] = dst_init.ravel()
        self.host = host
        self.buf = torch.from_numpy(host.copy()).cuda()
        self.src = self.buf[self.o_src:self.o_src + n_src].view(src.shape)
        self.dst = self.buf[self.o_dst:self.o_dst + n_dst].view(dst_shape)

    def check(self):
        """everything but the destination holds the bytes it held; returns the destination"""
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        keep = np.ones(got.size, bool)
        keep[self.o_dst:self.o_dst + self.n_dst] = False
        assert np.array_equal(_bits(got[keep]), _bits(self.host[keep])), "bytes outside the destination changed"
        return got[self.o_dst:self.o_dst + self.n_dst]


# ---- 1, 2. the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])    # shifted: dst one float off 16 bytes - the 4-pixel form must not be taken
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_dihedral_equals_the_host_rule(n, H, W, shift):
    rng = np.random.default_rng(n * 1000 + H + W)
    x = rng.standard_normal((n, H, W, 3)).astype(np.float32)
    x.ravel()[:4] = [0.0, -0.0, np.float32(1e-42), np.inf]                       # bits that a multiply by 1 could touch
    for k in range(8):
        want = ensemble.transform(x, k)
        a = _Arena(x, want.shape, shift=shift)
        out = ops.dihedral(a.src, k, out=a.dst)
        assert out.data_ptr() == a.dst.data_ptr()
        got = a.check().reshape(want.shape)
        assert _same(got, want), (k, int((_bits(got) != _bits(want)).sum()))
        if shift == 0:
            assert _same(ops.dihedral(_dev(x), k).cpu().numpy(), want), k        # a tensor of its own
    tail = x[:, 1:]                                                              # (without the special values of row 0)
    half = ops.dihedral(_dev(tail), 5, scale=0.5).cpu().numpy()                  # the scale, once (a power of two: exact)
    assert _same(half, ensemble.transform(tail, 5) * np.float32(0.5))


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_dihedral_accum_equals_the_host_rule(n, H, W, shift):
    H, W = 4 * H, 4 * W                                                          # the HR sizes of those LR shapes
    rng = np.random.default_rng(n * 2000 + H + W)
    acc0 = rng.standard_normal((n, H, W, 3)).astype(np.float32)
    for k in range(8):
        y = rng.standard_normal((n, W, H, 3) if k & 4 else (n, H, W, 3)).astype(np.float32)
        for scale in (1.0, 0.125):                                               # add; add, then scale (the last member of 8)
            want = acc0 + ensemble.inverse(y, k)                                 # float32: one rounding
            if scale != 1.0:
                want = want * np.float32(scale)
            a = _Arena(y, acc0.shape, dst_init=acc0, shift=shift)
            ops.dihedral_accum(a.dst, a.src, k, scale)
            got = a.check().reshape(want.shape)
            assert _same(got, want), (k, scale, int((_bits(got) != _bits(want)).sum()))


def test_ops_refuse_bad_arguments():
    x = torch.zeros((1, 6, 10, 3), device="cuda")
    with pytest.raises(ValueError):
        ops.dihedral(x, 8)
    with pytest.raises(ValueError):
        ops.dihedral(x, 4, out=torch.zeros((1, 6, 10, 3), device="cuda"))        # k >= 4 swaps the shape
    with pytest.raises(ValueError):
        ops.dihedral_accum(x, torch.zeros((1, 10, 6, 3), device="cuda"), 1)
    with pytest.raises(ValueError):
        ops.dihedral(torch.zeros((6, 10, 4), device="cuda"), 0)


# ---- 3. the forward ------------------------------------------------------------------------------------------------------------------
CASES = {"T7": (PFNLGeometry(num_block=NB), "fp32", (2, 7, 16, 24)),
         "T5x2": (PFNLGeometry(num_frames=5, scale=2, num_block=NB), "fp32", (1, 5, 12, 20)),
         "bf16": (PFNLGeometry(num_block=NB), "bf16", (2, 7, 16, 24))}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_ensemble_is_the_composition_of_forwards(case):
    geom, precision, (B, T, H, W) = CASES[case]
    eng = _engine(geom, precision)
    x = synth.uniform_clips(B, T, H, W, seed=21)
    xd = _dev(x)
    y1 = eng.forward(xd).cpu().numpy()
    assert y1.shape == (B, 1, geom.scale * H, geom.scale * W, 3) and np.isfinite(y1).all()
    assert _same(eng.forward(xd, ensemble=1).cpu().numpy(), y1)
    for n in (2, 4, 8):
        want = ensemble.combine(_plain(eng), x, n)
        got = eng.forward(xd, ensemble=n)
        assert torch.is_tensor(got) and got.is_cuda
        got = got.cpu().numpy()
        assert _same(got, want), (case, n, int((_bits(got) != _bits(want)).sum()), float(np.abs(got - want).max()))
        assert not _same(got, y1), (case, n)                                     # no member is a no-op
        print(f"\n[ensemble] {case} n={n}: max |ensemble - plain| {np.abs(got - y1).max():.3g}", end="")
    eng.ensemble = 4                                                             # the engine's default member count
    assert _same(eng.forward(xd).cpu().numpy(), ensemble.combine(_plain(eng), x, 4))
    out = torch.empty(eng.out_shape(B, H, W), dtype=torch.float32, device="cuda")
    eng.forward_device(xd.data_ptr(), out.data_ptr(), B, H, W)                   # ... which forward_device does not read
    assert _same(out.cpu().numpy(), y1)
    eng.forward_device(xd.data_ptr(), out.data_ptr(), B, H, W, ensemble=2)
    assert _same(out.cpu().numpy(), ensemble.combine(_plain(eng), x, 2))
    eng.sync()                                                                   # no member left a range flag
    with pytest.raises(ValueError):
        eng.forward(xd, ensemble=3)
    eng.close()


def test_forward_ensemble_host_pointers():
    """numpy in, numpy out (staging inside the call) against the composition of host-pointer forwards; a torch CPU tensor likewise."""
    eng = _engine()
    x = synth.uniform_clips(2, 7, 16, 24, seed=22)
    for n in (2, 4, 8):
        want = ensemble.combine(lambda a: eng.forward(a), x, n)
        got = eng.forward(x, ensemble=n)
        assert isinstance(got, np.ndarray) and _same(got, want), n
    got = eng.forward(torch.from_numpy(x), ensemble=8)
    assert torch.is_tensor(got) and not got.is_cuda and _same(got.numpy(), want)
    assert eng.range_reruns() == 0
    eng.close()


# ---- 4. the oracle -------------------------------------------------------------------------------------------------------------------
def test_forward_ensemble_against_the_oracle():
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=0)
    x = synth.uniform_clips(1, 7, 12, 20, seed=23)
    fo = pfnl_fast.FastOracle(w, num_block=1)
    ref = ensemble.combine(lambda a: fo.forward(np.ascontiguousarray(a)), x, 8)
    eng = _engine(geom)
    y = eng.forward(_dev(x), ensemble=8).cpu().numpy()
    err = float(np.abs(y - ref).max())
    print(f"\n[ensemble] oracle: max |hip - oracle| {err:.3g}", end="")
    assert y.shape == ref.shape and err < TF.ABS_TOL, err
    eng.close()


# ---- 5. history ----------------------------------------------------------------------------------------------------------------------
def test_plain_forward_around_an_ensemble_is_bit_identical():
    eng = _engine()
    x = synth.uniform_clips(2, 7, 16, 24, seed=24)
    xd = _dev(x)
    y0 = eng.forward(xd).cpu().numpy()
    y8 = eng.forward(xd, ensemble=8).cpu().numpy()                               # the handle runs 24 x 16 in between (members 4 .. 7)
    y1 = eng.forward(xd).cpu().numpy()
    assert _same(y0, y1) and not _same(y0, y8)
    assert _same(eng.forward(xd, ensemble=8).cpu().numpy(), y8)
    eng.close()


# ---- 6. range ------------------------------------------------------------------------------------------------------------------------
def test_host_pointer_ensemble_reruns_once_on_the_strict_kernels():
    """x 600 as in test_split16_domain_nonlocal_input_scale (600 * 2^7 > 65504 in the f16 non-local kernel, 1024 keys): every member
    raises the call's flag; the call reads it once, redoes the whole ensemble strict and counts one rerun.  Each plain host-pointer
    forward of the composition reruns strict by itself: same bytes."""
    eng = _engine()
    x = (synth.uniform_clips(1, 7, 64, 64, seed=5) * 600.0).astype(np.float32)
    r0 = eng.range_reruns()
    got = eng.forward(x, ensemble=4)
    r1 = eng.range_reruns()
    assert r1 == r0 + 1 and np.isfinite(got).all()
    want = ensemble.combine(lambda a: eng.forward(a), x, 4)
    assert eng.range_reruns() == r1 + 4                                          # the composition's four forwards, one rerun each
    assert _same(got, want), int((_bits(got) != _bits(want)).sum())
    eng.sync()                                                                   # nothing left for the asynchronous side
    eng.close()


# ---- 7. the session ------------------------------------------------------------------------------------------------------------------
def _stream_all(vs, frames):
    got = []
    for f in frames:
        got += vs.push(f)
        got += vs.pop_ready()
    got += vs.end()
    return got


def test_session_runs_the_ensemble_per_batch():
    eng = _engine()
    F, H, W, batch, T = 9, 16, 24, 2, 7
    frames = np.random.default_rng(25).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    dev = _dev((frames / 255.).astype(np.float32))
    want, plain = [], []
    for first in range(0, F, batch):                                             # stream.next_batch's batches: [k * batch, min((k + 1) * batch, F))
        win = ops.gather_windows(dev, first, min(batch, F - first), T)
        want.append(ops.quantise_u8(eng.forward(win, ensemble=8))[:, 0].cpu().numpy())
        plain.append(ops.quantise_u8(eng.forward(win))[:, 0].cpu().numpy())
    want, plain = np.concatenate(want), np.concatenate(plain)
    assert not np.array_equal(want, plain)
    with eng.open_stream(H, W, batch=batch, ensemble=8) as vs:
        assert vs.ensemble == 8
        got = vs.push(frames[0])
        assert got == [] and vs._lib.pfnl_stream_ensemble(vs._s, 4) == -2        # PFNL_ERR_STATE behind the first push
        assert vs._lib.pfnl_stream_ensemble(vs._s, 3) == -1
        got = _stream_all(vs, frames[1:])
        assert [i for i, _ in got] == list(range(F))
        assert np.array_equal(np.stack([f for _, f in got]), want)
        vs.reset()                                                               # the setting survives
        got = _stream_all(vs, frames)
        assert np.array_equal(np.stack([f for _, f in got]), want)
    with eng.open_stream(H, W, batch=batch, ensemble=8, out_format="nv12") as vs:
        got = _stream_all(vs, frames)
        assert np.array_equal(np.stack([f for _, f in got]), np.stack([yuv.from_rgb(f, "nv12") for f in want]))
    with eng.open_stream(H, W, batch=batch, ensemble=1) as vs:
        one = np.stack([f for _, f in _stream_all(vs, frames)])
    with eng.open_stream(H, W, batch=batch) as vs:
        assert vs.ensemble == 1
        none = np.stack([f for _, f in _stream_all(vs, frames)])
    assert np.array_equal(one, none) and np.array_equal(none, plain)
    with pytest.raises(ValueError):
        eng.open_stream(H, W, batch=batch, ensemble=3)
    eng.close()


# ---- 8. the harness ------------------------------------------------------------------------------------------------------------------
def test_harness_runs_the_ensemble(tmp_path):
    from PIL import Image
    from model.pfnl import PFNL
    F, H, W = 5, 16, 24
    lr_u8 = np.random.default_rng(26).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    seq = tmp_path / "seq"
    (seq / "blur4").mkdir(parents=True)
    for i, im in enumerate(lr_u8):
        Image.fromarray(im).save(seq / "blur4" / f"{i:04d}.png")
    m = PFNL()
    assert m.self_ensemble == 1
    m.num_block = NB
    m.save_dir = str(tmp_path / "none")
    m.set_weights(synth.synthetic_weights(PFNLGeometry(num_block=NB), seed=0))
    win = np.ascontiguousarray(M.sliding_windows((lr_u8 / 255.).astype(np.float32), 7))
    decoded = {}
    for n in (8, 1):
        m.self_ensemble = n
        m.test_video_lr(str(seq), name=f"out{n}", part=2)                        # 5 frames, part 2 -> batches of 3 and 2
        decoded[n] = np.stack([np.asarray(Image.open(p)) for p in sorted((seq / f"out{n}").glob("*.png"))])
    eng = m._get_engine()
    for n in (8, 1):
        want = np.concatenate([M.quantise(ensemble.combine(_plain(eng), win[a:b], n)[:, 0]) for a, b in ((0, 3), (3, 5))])
        assert decoded[n].shape == want.shape == (F, 4 * H, 4 * W, 3)
        assert np.array_equal(decoded[n], want), n
    assert not np.array_equal(decoded[8], decoded[1])
    m.self_ensemble = 3
    with pytest.raises(ValueError):
        m.test_video_lr(str(seq), name="bad", part=2)
