"""tests/streams.py on the host (no GPU): the module imports without a device, the delay rule is the documented one, the fills are what
the probes say they are (quiet NaN for floating types, 0xA5 bytes for integers), the comparison is by bits, and the torch-side helpers
keep shape, type and bytes on CPU tensors."""
import numpy as np
import pytest

import streams as St


def test_delay_rule():
    """D = max(25 ms, 3 x the warm-up's wall time), capped at 250 ms."""
    assert St.delay_ms(0.0) == 25.0 and St.delay_ms(8.0) == 25.0
    assert St.delay_ms(20.0) == 60.0
    assert St.delay_ms(83.4) == pytest.approx(250.0, abs=0.21) and St.delay_ms(1e4) == 250.0
    assert St.CONTROL_D_MS == St.D_MIN_MS                       # the controls run at the smallest delay a probe can get


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8, np.uint16, np.int64])
def test_fill_is_nan_or_a5_bytes(dtype):
    a = np.zeros((3, 5), dtype)
    f = St.fill_like(a)
    assert f.shape == a.shape and f.dtype == a.dtype
    if np.issubdtype(dtype, np.floating):
        assert np.isnan(f).all()
    else:
        assert (f.reshape(-1).view(np.uint8) == 0xA5).all()
    assert St.same_bits(f, St.fill_like(a)) and not St.same_bits(f, a)


def test_same_bits_compares_integers_not_values():
    nan = np.full(4, np.nan, np.float32)
    assert St.same_bits(nan, nan.copy())                       # NaN equals NaN as bits
    assert not St.same_bits(np.float32([0.0]), np.float32([-0.0]))
    assert not St.same_bits(np.zeros(4, np.float32), np.zeros((2, 2), np.float32))
    assert not St.same_bits(np.zeros(4, np.float32), np.zeros(4, np.float64))


def test_torch_helpers_keep_the_bytes():
    torch = pytest.importorskip("torch")
    for dtype in (np.float32, np.uint8, np.uint16, np.int64, np.float64):
        a = (np.arange(24).reshape(2, 3, 4) * 37 % 251).astype(dtype)
        t = torch.from_numpy(a.view(np.int16) if dtype == np.uint16 else a)
        t = t.view(torch.uint16) if dtype == np.uint16 else t
        flat = St._as_int(t)
        assert flat.dim() == 1 and flat.numel() == a.size and flat.element_size() == a.dtype.itemsize
        assert St.same_bits(St.to_numpy(flat.clone(), t), a)
        St.fill_pattern(t)                                     # on a CPU tensor: the same fill the numpy side states
        assert St.same_bits(St.to_numpy(St._as_int(t), t), St.fill_like(a))
