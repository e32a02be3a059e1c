"""Host-side logic (no GPU): drop-in class surface, harness helpers, checkpoint layout."""
import inspect
import os

import numpy as np
import pytest

from conftest import load_golden
from pfnl_amd import checkpoint, synth, tfbundle
from pfnl_amd import model as M
from pfnl_amd.spec import PFNLGeometry, check_weights


def test_class_surface_matches_reference():
    from model.pfnl import PFNL          # the import the reference's main.py:8 performs
    from model.base_model import VSR
    m = PFNL()
    assert isinstance(m, VSR)
    # reference model/pfnl.py:21-37
    want = dict(num_frames=7, scale=4, in_size=32, gt_size=128, eval_in_size=[128, 240], batch_size=16,
                eval_basz=4, learning_rate=1e-3, end_lr=1e-4, reload=True, max_step=int(1.5e5 + 1),
                decay_step=1.2e5, train_dir='./data/filelist_train.txt', eval_dir='./data/filelist_val.txt',
                save_dir='./checkpoint/pfnl', log_dir='./pfnl.txt')
    for k, v in want.items():
        assert getattr(m, k) == v, k
    sig = lambda f: list(inspect.signature(f).parameters.items())
    assert [(k, p.default) for k, p in sig(m.test_video_truth)] == [('path', inspect._empty), ('name', 'result'),
                                                                    ('reuse', False), ('part', 50)]
    assert [(k, p.default) for k, p in sig(m.test_video_lr)] == [('path', inspect._empty), ('name', 'result'),
                                                                 ('reuse', False), ('part', 50)]
    assert [(k, p.default) for k, p in sig(m.testvideos)][1:] == [('start', 0), ('name', 'pfnl')]
    assert [k for k, _ in sig(m.load)] == ['sess', 'checkpoint_dir', 'step']
    assert [k for k, _ in sig(m.save)] == ['sess', 'checkpoint_dir', 'step']
    for fn in (m.train, m.build):
        with pytest.raises(NotImplementedError):
            fn()
    assert [k for k, _ in sig(m.eval)] == []                     # eval() takes no arguments (model/pfnl.py:94)
    assert PFNL.testvideo is PFNL.test_video_lr


def test_windows_and_quantise_match_golden():
    gd = load_golden("harness_5x16x24_nb1")
    lrs = (gd["lr_u8"] / 255.).astype(np.float32)
    win = M.sliding_windows(lrs, 7)
    assert win.shape == (5, 7, 16, 24, 3)
    for i in range(5):
        for k in range(7):
            assert np.array_equal(win[i, k], lrs[min(max(i + k - 3, 0), 4)])
    assert np.array_equal(M.quantise(gd["sr"][:, 0]), gd["sr_u8"])
    assert M.sliding_windows(np.zeros((0, 4, 4, 3), np.float32), 7).shape == (0, 7, 4, 4, 3)
    assert M.sliding_windows(lrs[:1], 7).shape == (1, 7, 16, 24, 3)


def test_blur_decimate_matches_scipy_definition():
    import scipy.ndimage
    delta = np.zeros((13, 13))
    delta[6, 6] = 1
    blur = scipy.ndimage.gaussian_filter(delta, 1.6)          # reference utils.py:95-105
    k = synth.gaussian_kernel_1d()
    assert np.allclose(blur, np.outer(k, k), atol=1e-15)
    rng = np.random.default_rng(0)
    hr = rng.random((2, 24, 32, 3))
    lr = synth.blur_decimate(hr, 4)
    assert lr.shape == (2, 6, 8, 3)
    hp = np.pad(hr, ((0, 0), (6, 6), (6, 6), (0, 0)), mode="reflect")
    ref = np.einsum("ij,bijc->bc", blur, hp[:, 4:17, 8:21])   # output (1,2): rows 4.., cols 8..
    assert np.allclose(lr[:, 1, 2], ref, atol=1e-6)


def test_load_returns_false_without_checkpoint(tmp_path, capsys):
    m = M.PFNL()
    assert m.load(None, str(tmp_path / "nope")) is False
    assert m.load(None, str(tmp_path)) is False
    assert "ERROR" in capsys.readouterr().out


def test_checkpoint_roundtrip_tf_layout(tmp_path):
    g = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(g)
    m = M.PFNL()
    m.num_block = 1
    m.set_weights(w)
    m.save(None, str(tmp_path), 500)
    files = set(os.listdir(tmp_path))
    assert {"checkpoint", "VSR-500.index", "VSR-500.data-00000-of-00001", "VSR-500.npz"} <= files
    assert checkpoint.read_state_file(str(tmp_path)) == "VSR-500"
    os.remove(tmp_path / "VSR-500.npz")                        # force the TF bundle reader
    m2 = M.PFNL()
    m2.num_block = 1
    assert m2.load(None, str(tmp_path)) is True
    check_weights(g, m2._weights)
    for k in w:
        assert np.array_equal(m2._weights[k], w[k]), k
    # optimizer slots / global_step in a training checkpoint are ignored; outer scope may differ
    extra = {("model/" + k): v for k, v in w.items()}
    extra["beta1_power"] = np.float32(0.9)
    extra["Variable"] = np.int64(1500)
    extra["model/nlvsr/conv0/kernel/Adam"] = np.zeros_like(w["nlvsr/conv0/kernel"])
    tfbundle.write_bundle(str(tmp_path / "VSR-1500"), {k: np.asarray(v) for k, v in extra.items()})
    got = checkpoint.load_checkpoint(str(tmp_path), g, step=1500)
    assert got is not None and np.array_equal(got[1]["nlvsr/conv0/kernel"], w["nlvsr/conv0/kernel"])


def test_tfbundle_known_answers(tmp_path):
    assert tfbundle.crc32c(b"123456789") == 0xE3069283        # CRC-32C check value
    assert tfbundle.crc32c(b"\x00" * 32) == 0x8A9136AA        # RFC 3720 B.4
    assert tfbundle.crc32c(b"\xff" * 32) == 0x62A8AB43
    assert tfbundle.unmask_crc(tfbundle.mask_crc(0x12345678)) == 0x12345678
    t = {"a/b": np.arange(6, dtype=np.float32).reshape(2, 3), "a/c": np.array(7, np.int64),
         "z": np.zeros((0, 4), np.float32)}
    tfbundle.write_bundle(str(tmp_path / "x"), t)
    idx = tfbundle.read_index(str(tmp_path / "x"))
    assert idx["a/b"]["shape"] == (2, 3) and idx["a/b"]["dtype"] == tfbundle.DT_FLOAT
    back = tfbundle.read_bundle(str(tmp_path / "x"), verify_data=True)
    for k in t:
        assert np.array_equal(back[k], t[k]) and back[k].shape == t[k].shape
    raw = bytearray(open(tmp_path / "x.index", "rb").read())
    raw[5] ^= 0xFF
    open(tmp_path / "x.index", "wb").write(bytes(raw))
    with pytest.raises(ValueError):
        tfbundle.read_index(str(tmp_path / "x"))


def test_many_tensor_bundle_spans_several_blocks(tmp_path):
    rng = np.random.default_rng(1)
    t = {f"scope/layer_{i:03d}/kernel": rng.random((3, 3, 2, 2)).astype(np.float32) for i in range(300)}
    tfbundle.write_bundle(str(tmp_path / "big"), t, block_size=512)
    back = tfbundle.read_bundle(str(tmp_path / "big"))
    assert set(back) == set(t) and all(np.array_equal(back[k], t[k]) for k in t)


def test_metrics_known_answers():
    from pfnl_amd import metrics as mt
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, size=(24, 32, 3)).astype(np.float64)
    assert mt.psnr_y(a, a) == float("inf") and abs(mt.ssim(a[..., 0], a[..., 0]) - 1.0) < 1e-12
    # BT.601 studio swing: black -> Y 16, white -> Y 235, grey keeps Cb = Cr = 128
    assert np.allclose(mt.rgb2ycbcr(np.zeros(3)), [16, 128, 128])
    assert np.allclose(mt.rgb2ycbcr(np.full(3, 255.0)), [235, 128, 128], atol=1e-9)
    # constant offset d on all channels -> Y offset d*(sum of the Y row) = d*219/255
    b = a + 3.0
    assert abs(mt.psnr_y(a, b) - 20 * np.log10(255.0 / (3.0 * 219.0 / 255.0))) < 1e-9
    assert abs(mt.psnr_rgb(a / 255, b / 255) - 10 * np.log10(1.0 / (3.0 / 255) ** 2)) < 1e-9
    # AVG_PSNR protocol: borders are excluded, frames are rounded to uint8 first
    vt = rng.random((6, 40, 48, 3))
    vp = vt.copy()
    vp[:, :8] += 0.5
    vp[:2] += 0.5                                   # spatial / temporal borders only
    assert mt.avg_psnr(vt, np.clip(vp, 0, 2)) == float("inf") or mt.avg_psnr(vt, np.clip(vp, 0, 2)) > 100
    assert mt.ssim(a[..., 0], 255 - a[..., 0]) < 0.1


# ---- round 2 -------------------------------------------------------------------------------------------------------

def test_ssim_matches_the_reference_implementation():
    """metrics.ssim against outputs of the REFERENCE's own modules/SSIM_Index.compute_ssim, generated in the build
    container by tools/make_metric_golden.py (the one piece of the reference that imports without TF1)."""
    from conftest import load_golden
    from pfnl_amd import metrics
    gd = load_golden("ssim_ref")
    for a, b, (h, w, s255, s1) in zip(gd["a"], gd["b"], gd["hw_ssim255_ssim1"]):
        h, w = int(h), int(w)
        assert abs(metrics.ssim(a[:h, :w], b[:h, :w]) - s255) < 1e-12
        assert abs(metrics.ssim(a[:h, :w] / 255.0, b[:h, :w] / 255.0, L=1.0) - s1) < 1e-12
    assert gd["hw_ssim255_ssim1"][0, 2] == 1.0                      # identical images


def _crc32c_bitwise(data: bytes) -> int:                            # independent of tfbundle's table-driven version
    c = 0xFFFFFFFF
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
    return c ^ 0xFFFFFFFF


def test_tfbundle_reader_on_a_hand_assembled_bundle(tmp_path):
    """The reader against bytes assembled HERE from the published layouts (LevelDB table_format: prefix-compressed
    entries, restart arrays, block trailers with masked crc32c, index block of separator keys, 48-byte footer;
    tensor_bundle.proto: BundleHeaderProto / BundleEntryProto) - nothing of write_bundle is involved.  Two data blocks,
    restart interval 2, optimizer slots and scalars mixed in, as tf.train.Saver writes a training checkpoint."""
    import struct

    def varint(n):
        out = b""
        while n >= 0x80:
            out += bytes([(n & 0x7f) | 0x80])
            n >>= 7
        return out + bytes([n])

    def mask(c):
        return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xa282ead8) & 0xFFFFFFFF

    def entry(dtype, shape, offset, size, crc):
        dims = b"".join(b"\x12" + varint(len(b"\x08" + varint(d))) + b"\x08" + varint(d) for d in shape)
        msg = b"\x08" + varint(dtype)                               # dtype = 1
        if dims:
            msg += b"\x12" + varint(len(dims)) + dims               # shape = 2 { dim = 2 { size = 1 } }
        if offset:
            msg += b"\x20" + varint(offset)                         # offset = 4 (shard_id = 3 omitted: 0)
        return msg + b"\x28" + varint(size) + b"\x35" + struct.pack("<I", crc)   # size = 5, crc32c = 6 (fixed32)

    def block(items, interval):
        out, restarts, prev = b"", [], b""
        for i, (k, v) in enumerate(items):
            shared = 0
            if i % interval == 0:
                restarts.append(len(out))
            else:
                while shared < min(len(prev), len(k)) and prev[shared] == k[shared]:
                    shared += 1
            out += varint(shared) + varint(len(k) - shared) + varint(len(v)) + k[shared:] + v
            prev = k
        restarts = restarts or [0]
        return out + b"".join(struct.pack("<I", r) for r in restarts) + struct.pack("<I", len(restarts))

    def with_trailer(b):
        return b + b"\x00" + struct.pack("<I", mask(_crc32c_bitwise(b + b"\x00")))

    g = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(g, seed=4)
    tensors = dict(w)
    tensors["nlvsr/conv0/kernel/Adam"] = np.ones((5, 5, 3, 64), np.float32)
    tensors["nlvsr/conv0/kernel/Adam_1"] = np.full((5, 5, 3, 64), 2, np.float32)
    tensors["Variable"] = np.array(1500, dtype=np.int64)           # global_step (model/pfnl.py:153)
    tensors["beta1_power"] = np.array(0.9, dtype=np.float32)
    codes = {np.dtype("float32"): 1, np.dtype("int64"): 9}
    data, items = b"", [(b"", b"\x08\x01\x1a\x02\x08\x01")]         # header: num_shards = 1, version { producer = 1 }
    for name in sorted(tensors):
        raw = tensors[name].tobytes()
        items.append((name.encode(), entry(codes[tensors[name].dtype], tensors[name].shape, len(data), len(raw),
                                           mask(_crc32c_bitwise(raw) if len(raw) < 65536 else tfbundle.crc32c(raw)))))   # (big tensors: the table-driven crc, itself pinned by known answers)
        data += raw
    split = len(items) // 2
    f, handles = b"", []
    for chunk in (items[:split], items[split:]):
        b = block(chunk, 2)
        handles.append(varint(len(f)) + varint(len(b)))
        f += with_trailer(b)
    meta = block([], 1)
    mh = varint(len(f)) + varint(len(meta))
    f += with_trailer(meta)
    idx = block([(items[split - 1][0] + b"\x00", handles[0]), (items[-1][0] + b"\xff", handles[1])], 1)   # separators >= last key
    ih = varint(len(f)) + varint(len(idx))
    f += with_trailer(idx)
    foot = mh + ih
    f += foot + b"\x00" * (40 - len(foot)) + struct.pack("<Q", 0xdb4775248b80fb57)
    (tmp_path / "VSR-1500.index").write_bytes(f)
    (tmp_path / "VSR-1500.data-00000-of-00001").write_bytes(data)
    (tmp_path / "checkpoint").write_text('model_checkpoint_path: "VSR-1500"\nall_model_checkpoint_paths: "VSR-1500"\n')
    got = tfbundle.read_bundle(str(tmp_path / "VSR-1500"), verify_data=True)
    assert set(got) == set(tensors)
    assert all(np.array_equal(got[k], tensors[k]) for k in tensors)
    m = M.PFNL()
    m.num_block = 1
    assert m.load(None, str(tmp_path)) is True and m.loaded_step == 1500
    assert all(np.array_equal(m._weights[k], w[k]) for k in w)
    bad = bytearray(f)
    bad[10] ^= 0x40                                                  # a flipped bit inside the first data block
    (tmp_path / "VSR-1500.index").write_bytes(bytes(bad))
    with pytest.raises(ValueError):
        tfbundle.read_index(str(tmp_path / "VSR-1500"))
    with pytest.raises(ValueError):                                  # present but unreadable: raises, never "random weights"
        M.PFNL().load(None, str(tmp_path))


def test_checkpoint_format_preference_and_mismatch(tmp_path):
    g = PFNLGeometry(num_block=1)
    w_old, w_new = synth.synthetic_weights(g, seed=1), synth.synthetic_weights(g, seed=2)
    checkpoint.save_checkpoint(str(tmp_path), w_old, 10, fmt="npz")
    import time
    tfbundle.write_bundle(str(tmp_path / "VSR-10"), w_new)          # a (re)downloaded TF checkpoint next to a stale cache ...
    os.utime(tmp_path / "VSR-10.index", (time.time() - 500, time.time() - 500))   # ... with an OLD mtime (tar / rsync -t keep them)
    got = checkpoint.load_checkpoint(str(tmp_path), g, step=10)
    assert np.array_equal(got[1]["nlvsr/conv0/kernel"], w_new["nlvsr/conv0/kernel"])   # the cache does not carry this bundle's signature
    checkpoint.save_checkpoint(str(tmp_path), w_old, 9, fmt="npz")   # (the state file now names step 9)
    before = {f.name: f.stat().st_mtime_ns for f in tmp_path.iterdir()}
    with pytest.raises(FileExistsError):                             # no implicit deletion of a reference-format checkpoint ...
        checkpoint.save_checkpoint(str(tmp_path), w_old, 10, fmt="npz")
    assert {f.name: f.stat().st_mtime_ns for f in tmp_path.iterdir()} == before   # ... and no side effect before the raise
    assert checkpoint.read_state_file(str(tmp_path)) == "VSR-9"
    checkpoint.save_checkpoint(str(tmp_path), w_old, 10, fmt="both")  # rewrites the bundle, stamps the cache with its signature
    got = checkpoint.load_checkpoint(str(tmp_path), g, step=10)
    assert np.array_equal(got[1]["nlvsr/conv0/kernel"], w_old["nlvsr/conv0/kernel"])
    with np.load(tmp_path / "VSR-10.npz") as z:
        assert str(z[checkpoint._SIG_KEY]) == checkpoint.index_signature(str(tmp_path / "VSR-10"))
    os.remove(tmp_path / "VSR-10.npz")                               # "both" once, "npz" afterwards (a training loop): the bundle holds
    checkpoint.save_checkpoint(str(tmp_path), w_old, 10, fmt="npz")  # these very weights, so the cache is rewritten as its mirror
    with np.load(tmp_path / "VSR-10.npz") as z:
        assert str(z[checkpoint._SIG_KEY]) == checkpoint.index_signature(str(tmp_path / "VSR-10"))
    wt = dict(w_old)                                                 # theta / phi travel with the checkpoint: all four or an error
    for n, shp in g.optional_weight_shapes():
        wt[n] = np.full(shp, 0.01, np.float32)
    checkpoint.save_checkpoint(str(tmp_path), wt, 11, fmt="both")
    got = checkpoint.load_checkpoint(str(tmp_path), g, step=11)
    assert all(n in got[1] for n, _ in g.optional_weight_shapes())
    del wt[g.optional_weight_shapes()[0][0]]
    checkpoint.save_checkpoint(str(tmp_path), wt, 12, fmt="both")
    with pytest.raises(KeyError, match="theta"):
        checkpoint.load_checkpoint(str(tmp_path), g, step=12)
    m = M.PFNL()                                                     # default geometry (20 blocks) vs a 1-block checkpoint
    with pytest.raises(KeyError):
        m.load(None, str(tmp_path), step=10)
    m1 = M.PFNL()
    m1.save_dir = str(tmp_path / "empty")
    with pytest.raises(RuntimeError, match="no checkpoint"):
        m1._ensure_loaded(False)


def test_optional_theta_phi_layout():
    g = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(g)
    names = [n for n, _ in g.optional_weight_shapes()]
    assert names == ["nlvsr/nlblock_0/theta/theta/kernel", "nlvsr/nlblock_0/theta/theta/bias",
                     "nlvsr/nlblock_0/phi/phi/kernel", "nlvsr/nlblock_0/phi/phi/bias"]
    check_weights(g, w)
    w[names[0]] = np.zeros((1, 1, 84, 84), np.float32)
    with pytest.raises(KeyError):
        check_weights(g, w)


def test_bench_power_sampler_parses_rocm_smi(tmp_path, monkeypatch):
    """bench.py's best-effort power sampler: the socket power and the shader clock out of rocm-smi's report (not its cap line), the
    idle sample in front of the run dropped; no rocm-smi -> nothing reported."""
    import importlib.util
    import stat
    import time
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    fake = tmp_path / "rocm-smi"
    cnt = tmp_path / "n"
    fake.write_text("""#!/bin/sh
n=$(cat %s 2>/dev/null || echo 0); n=$((n+1)); echo $n > %s
if [ $n -le 1 ]; then p=250.0; c=157; else p=1370.0; c=1830; fi
echo "GPU[0]		: sclk clock level: 1: (${c}Mhz)"
echo "GPU[0]		: Current Socket Graphics Package Power (W): $p"
echo "GPU[0]		: Max Graphics Package Power (W): 1400.0"
""" % (cnt, cnt))
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", str(tmp_path) + os.pathsep + os.environ.get("PATH", ""))
    s = bench.PowerSampler(0)
    t0 = time.time()
    while len(s.samples) < 3 and time.time() - t0 < 20.0:          # (a loaded host may take its time to spawn the fake)
        time.sleep(0.05)
    got = s.stop()
    assert got is not None and got["cap_w"] == 1400.0 and got["package_w"] == 1370.0 and got["sclk_mhz"] == 1830 and got["samples"] >= 1
    monkeypatch.setenv("PATH", str(tmp_path / "nothing"))
    import shutil
    if shutil.which("rocm-smi") is None and not os.path.exists("/opt/rocm/bin/rocm-smi"):
        assert bench.PowerSampler(0).stop() is None


def test_bench_byte_model_matches_the_launch_structure_and_the_committed_traffic():
    """`roofline.frac` must be priced on the bytes of the launch structure that RAN, and counter
    bytes cannot be below them.  configs[1], default structure (conv1_i + conv10_i in one launch, conv2_i as a chain): 5F + 2B tiles
    of P x 256 B per block over two launches; the newest committed PMC traffic must be >= 0.95 x that (and < 1.3 x: no wasted
    re-reads inside a launch)."""
    import glob
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    g = PFNLGeometry()
    B, H, W, F = 4, 128, 128, 28

    def plan(structure, lpb, c10, chain, sf0=0):                     # what PFNLEngine.plan (pfnl_plan) returns for the structure (tests/test_gpu_forward.py::
        return {"structure": structure, "launches_per_block": lpb, "precision": "fp32", "conv3x3": "split16", "conv1x1": "split16",   # test_plan_is_what_runs ties
                "c10_fused": c10, "chain": chain, "sf0": sf0}                                                                        # these to the launches that run)
    # (structure, launches of the conv3x3 class per block, algorithmic tiles per block)
    for pl, launches, tiles in ((plan("chain2", 2, 1, 1), 2, 5 * F + 2 * B), (plan("split16_3", 3, 0, 1), 2, 5 * F + B), (plan("split16_3", 3, 1, 0), 3, 5 * F + 4 * B),
                                (plan("split16_4", 4, 0, 0), 3, 5 * F + 3 * B), (plan("mid4", 4, 0, 0), 3, 5 * F + 3 * B), (plan("chain2_sf0", 2, 1, 1, 1), 2, 5 * F + 2 * B)):
        rec = bench.conv3x3_roofline(g, {"conv3x3": {"ms": 2.0, "launches": 20}}, B, H, W, pl, "cfg2")
        assert rec["launches_per_step"] == launches * g.num_block, pl
        assert abs(rec["mbytes_per_launch"] * 1e6 - H * W * 256 * tiles / launches) < 1e4, (pl, rec["mbytes_per_launch"])
        assert rec["plan"] == pl["structure"]
        if pl["sf0"]:
            # the split-format copy of inp0 (blocks 0 .. nb-2) is REDUNDANT traffic: outside the algorithmic bytes `frac` is priced on, and named
            sc = rec["sf_copy"]
            assert abs(sc["redundant_mbytes_per_launch"] * 1e6 - H * W * 256 * F * (g.num_block - 1) / (2.0 * g.num_block)) < 1e4
            assert abs(sc["expected_traffic_over_algorithmic"] - (1 + F * 19 / 20.0 / (5 * F + 2 * B))) < 2e-3
        else:
            assert "sf_copy" not in rec
    rec = bench.conv3x3_roofline(g, {"conv3x3": {"ms": 2.0, "launches": 20}}, B, H, W, plan("chain2", 2, 1, 1), "cfg2")
    newest = sorted(glob.glob(os.path.join(root, "profiles", "r[0-9][0-9]_traffic_split16.json")))[-1]
    tj = json.load(open(newest))
    ratio = tj["hbm_bytes_per_launch_avg"] / (rec["mbytes_per_launch"] * 1e6)
    assert 0.95 <= ratio < 1.3, (newest, ratio)
    # what shares the CU's memory port with those bytes: one 73 728-byte half of the split weight pack per 8 x 32 tile, from L2
    port = rec["cu_port"]
    tiles = (H // 8) * (W // 32) * (2 * F + B) * g.num_block / rec["launches_per_step"]
    assert abs(port["l2_weight_stream_mbytes_per_launch"] * 1e6 - 73728 * tiles) < 1e4
    assert abs(port["mbytes_per_launch"] - rec["mbytes_per_launch"] - port["l2_weight_stream_mbytes_per_launch"]) < 0.02
    # bf16 trunk at 1080p: conv1_i + conv10_i, shared half, per-frame half = 5F + 4B tiles of P x 128 B over three launches
    rb = bench.conv3x3_roofline(g, {"conv3x3": {"ms": 3.0, "launches": 30}}, 1, 270, 480, {"structure": "bf16_3", "launches_per_block": 3, "precision": "bf16"}, "cfg4")
    assert abs(rb["mbytes_per_launch"] * 1e6 - 270 * 480 * 128 * (5 * 7 + 4) / 3) < 1e4



def test_bench_power_cap_model_and_the_committed_bench_line():
    """under the package power cap a launch takes a F + b B (tools/ubench/energy_mix.hip measured a and b).  The model
    is arithmetic on the launch's executed MFMA FLOPs (3 per product on the split-f16 path, conv10_i's included) and its HBM bytes - and
    the newest committed bench line must sit at that roofline (within the +-5 % the boxes of the pool differ by, both ways)."""
    import glob
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    g = PFNLGeometry()
    B, H, W, F = 4, 128, 128, 28
    pl = {"structure": "chain2", "launches_per_block": 2, "precision": "fp32", "conv3x3": "split16", "conv1x1": "split16", "c10_fused": 1, "chain": 1, "sf0": 0, "c1x1": 0}
    rec = bench.conv3x3_roofline(g, {"conv3x3": {"ms": 0.108 * 20, "launches": 20}}, B, H, W, pl, "cfg2")
    m = rec["power_cap_model"]
    flops = 3.0 * (2 * F + B) * H * W * 9 * 64 * 64 * 2 / 2 + 3.0 * F * H * W * 64 * 64 * 2 / 2       # per launch: half a block's 3x3s + conv10_i
    want = bench.POWER_CAP_MS_PER_TFLOP * flops / 1e12 + bench.POWER_CAP_US_PER_GB * 1e-3 * (H * W * 256 * (5 * F + 2 * B) / 2) / 1e9
    assert abs(m["model_ms_per_launch"] - want) < 2e-4 and abs(m["measured_ms_per_launch"] - 0.108) < 1e-6, (m, want)
    assert 0.10 < want < 0.11                                          # 106.5 us
    newest = sorted(glob.glob(os.path.join(root, "profiles", "r[0-9][0-9]_bench.json")))[-1]
    line = json.loads(open(newest).read().strip().splitlines()[-1])
    if "power_cap_model" in line["roofline"]:                          # (lines of the rounds before the model existed carry none)
        # (0.99 - 1.02 while every launch issued 32x32x16 MFMAs; with the chain launch on the cheaper 16x16x32 shape the roofline moved down to ~100 us per
        # launch and the two launches are 7 % above it: DESIGN.md R6.9 says where - the chain kernel's extra cycles, conv3x3_c1c10_kernel still on 32x32x16)
        assert 0.90 <= line["roofline"]["power_cap_model"]["model_over_measured"] <= 1.07, (newest, line["roofline"]["power_cap_model"])

def test_bench_nonlocal_flop_model_and_hbm_classes():
    """bench.py's `roofline_nl` prices the affinity class on SURVEY.md 8(a)-C's FLOPs (4 N^2 C + 4 N C^2 per clip:
    5.75 GFLOP at configs[1], 353.6 at 1080p) and on what the kernel's MFMAs execute (channels padded to 96, x3 for exactly split operands,
    x1 under precision=bf16); `roofline_hbm_classes` prices pack / conv0 / tail on the bytes their tensors have."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    g = PFNLGeometry()
    r = bench.nonlocal_roofline(g, {"nl_attn": 0.1}, 4, 128, 128, False)
    assert abs(r["algorithmic_gflop_per_step"] - 4 * 5.75) < 0.05 and r["keys"] == 4096 and r["channels"] == 84 and r["channels_padded"] == 96
    assert abs(r["achieved"] - 4 * 5.7519e9 / 1e-4 / 1e12) < 0.5 and abs(r["frac"] - r["achieved"] / 2500.0) < 1e-3
    ex = 4 * (4 * 4096 ** 2 * 96 * 3 + 4 * 4096 * 96 ** 2) / 1e-4 / 1e12
    assert abs(r["mfma_executed_tflops"] - ex) < 0.2 and r["mfma_per_product"] == 3
    rb = bench.nonlocal_roofline(g, {"nl_attn": 0.44}, 1, 270, 480, True)
    assert abs(rb["algorithmic_gflop_per_step"] - 353.6) < 0.5 and rb["mfma_per_product"] == 1 and rb["keys"] == 32400
    assert bench.nonlocal_roofline(g, {"nl_attn": 0.0}, 1, 32, 32, False) is None
    g5 = PFNLGeometry(num_frames=5, scale=2)
    assert bench.nonlocal_roofline(g5, {"nl_attn": 0.05}, 1, 64, 64, False)["channels"] == 60
    h = bench.hbm_class_rooflines(g, {"nl_pack": 0.012, "conv0": 0.035, "tail": 0.027, "merge1": 0.1}, 4, 128, 128)
    P = 128 * 128
    assert abs(h["tail"]["algorithmic_mbytes_per_step"] - 4 * (P * 48 * 4 + P * 12 + 16 * P * 12) / 1e6) < 1e-3
    assert abs(h["conv0"]["algorithmic_mbytes_per_step"] - 4 * (P // 4 * 96 * 4 + 7 * P * 256) / 1e6) < 1e-3
    assert abs(h["nl_pack"]["gbs"] - h["nl_pack"]["algorithmic_mbytes_per_step"] / 0.012) < 0.1 and 0 < h["tail"]["frac_of_hbm_peak"] < 1


def test_harness_numerics_match_the_reference_functions():
    """SURVEY.md 8(f)-3 / 8(f)-4 pinned to the reference's OWN code: tools/make_utils_golden.py takes gkern, _rgb2ycbcr, to_uint8 and
    AVG_PSNR out of /root/reference/utils.py (:95-105, :194-246) with `ast` and runs them on the real numpy / scipy in the build
    container; the fixture holds their outputs on seeded inputs (data only)."""
    from pfnl_amd import metrics
    gd = load_golden("utils_ref")
    k = synth.gaussian_kernel_1d(13, 1.6)
    assert np.abs(np.outer(k, k) - gd["blur"]).max() < 1e-15                    # BLUR = gkern(13, 1.6): separable, as built here
    assert abs(gd["blur"][6, 6] - 0.0621745) < 1e-7                             # (the centre tap SURVEY.md quotes)
    assert np.abs(metrics.rgb2ycbcr(gd["rgb"], 255.0) - gd["ycc255"]).max() < 1e-10
    assert np.abs(metrics.rgb2ycbcr(gd["rgb"] / 255.0, 1.0) - gd["ycc1"]).max() < 1e-12
    assert np.array_equal(metrics.to_uint8(gd["u8_in"], 0.0, 1.0), gd["u8_out"])  # np.round: ties to even, clipped
    vt, vp = gd["vid_true"], gd["vid_pred"]
    assert abs(metrics.avg_psnr(vt, vp, 0.0, 1.0) - gd["avg_psnr"][0]) < 1e-9
    assert abs(metrics.avg_psnr(vt * 255.0, vp * 255.0, 0.0, 255.0) - gd["avg_psnr"][1]) < 1e-9
    assert abs(metrics.avg_psnr(vt, vp, 0.0, 1.0, t_border=0, sp_border=4) - gd["avg_psnr"][2]) < 1e-9
    # the decimation the harness applies (utils.py:169-192 with this BLUR) as one dense correlation with the reference's 13x13 kernel
    rng = np.random.default_rng(5)
    hr = rng.random((2, 24, 32, 3))
    xp = np.pad(hr, ((0, 0), (6, 6), (6, 6), (0, 0)), mode="reflect")
    want = np.zeros((2, 6, 8, 3))
    for a in range(13):
        for b in range(13):
            want += gd["blur"][a, b] * xp[:, a:a + 21:4, b:b + 29:4]
    assert np.abs(synth.blur_decimate(hr, 4) - want).max() < 1e-7              # (blur_decimate returns float32)


def test_bench_dump_output_budget(tmp_path):
    """bench.py --dump-outputs writes float32 [B,1,sH,sW,3]; past the byte budget it keeps a fixed, seeded choice of whole clips
    (and, should one clip alone be over it, a seeded sample of that clip's values) - the same files from run to run."""
    import sys
    torch = pytest.importorskip("torch")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    out = torch.arange(6 * 1 * 8 * 8 * 3, dtype=torch.float32).reshape(6, 1, 8, 8, 3)
    rec = bench.dump_output(out, str(tmp_path / "a"), "output", 1 << 20)
    got = np.load(tmp_path / "a" / "output.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out.numpy()) and rec["clips"] == list(range(6))
    clip = out[0].numpy().nbytes
    rec = bench.dump_output(out, str(tmp_path / "b"), "output", 2 * clip + 7)
    got = np.load(tmp_path / "b" / "output.npy")
    assert len(rec["clips"]) == 2 and rec["clips"] == sorted(rec["clips"]) and np.array_equal(got, out.numpy()[rec["clips"]])
    assert bench.dump_output(out, str(tmp_path / "c"), "output", 2 * clip + 7) == rec
    rec = bench.dump_output(out, str(tmp_path / "d"), "output", 100)
    got = np.load(tmp_path / "d" / "output.npy")
    assert got.shape == (25,) and got.nbytes <= 100 and np.all(np.isin(got, out.numpy()[rec["clips"]]))
