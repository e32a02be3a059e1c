"""The streaming session's device-free side (include/pfnl_hip.h, pfnl_stream_*): its symbols are declared, exported and typed; its argument
validation needs no device; and the scheduling rule - pfnl_stream_next_batch, the one statement of which batch may launch when - forms
exactly the batches of the harness, each at the first push that completes its last window."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi

STREAM_SYMBOLS = ["pfnl_stream_open", "pfnl_stream_push", "pfnl_stream_end", "pfnl_stream_ready", "pfnl_stream_pop", "pfnl_stream_reset",
                  "pfnl_stream_close", "pfnl_stream_next_batch", "pfnl_op_gather_windows_u8"]


def test_stream_symbols_and_validation_without_gpu():
    text = open(os.path.join(ROOT, "include", "pfnl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pfnl_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(_capi.LIB_PATH)
    for name in STREAM_SYMBOLS:
        assert name in declared, f"include/pfnl_hip.h does not declare {name}"
        assert hasattr(raw, name), f"libpfnl_hip.so does not export {name}"
        assert name in _capi.SIGNATURES, f"_capi.SIGNATURES has no {name}"
    lib = _capi.load_library()
    assert lib.pfnl_version() == 4                                               # symbols were added, nothing changed
    s = C.c_void_p()
    dummy = C.c_void_p(16)                                                       # never dereferenced: the calls return first
    idx, got, n = C.c_longlong(0), C.c_int(0), C.c_int(0)
    assert lib.pfnl_stream_open(None, 16, 24, 1, None, C.byref(s)) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_open(dummy, 16, 24, 1, None, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_open(dummy, 16, 24, 0, None, C.byref(s)) == -1 and b"batch" in lib.pfnl_last_error()
    for H, W in [(15, 24), (16, 23), (0, 24), (16, -2)]:
        assert lib.pfnl_stream_open(dummy, H, W, 1, None, C.byref(s)) == -1 and b"even" in lib.pfnl_last_error()
    assert lib.pfnl_stream_push(None, dummy, 0) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_pop(None, dummy, 0, C.byref(idx), C.byref(got)) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_end(None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_ready(None, C.byref(n)) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_reset(None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_close(None) == -1 and b"NULL" in lib.pfnl_last_error()
    first, count = C.c_longlong(0), C.c_int(0)
    assert lib.pfnl_stream_next_batch(7, 1, 0, 0, 0, None, C.byref(count)) == -1
    assert lib.pfnl_stream_next_batch(4, 1, 0, 0, 0, C.byref(first), C.byref(count)) == -1       # even T
    assert lib.pfnl_stream_next_batch(7, 0, 0, 0, 0, C.byref(first), C.byref(count)) == -1       # batch 0
    assert lib.pfnl_stream_next_batch(7, 1, 2, 0, 3, C.byref(first), C.byref(count)) == -1       # launched > pushed
    # the op hook refuses before any HIP call as well
    op = lambda cap, last, first_, cnt, T, H, W: lib.pfnl_op_gather_windows_u8(dummy, dummy, cap, last, first_, cnt, T, H, W, None)  # noqa: E731
    assert lib.pfnl_op_gather_windows_u8(None, dummy, 8, 3, 0, 1, 7, 16, 24, None) == -1
    assert op(8, 3, 0, 1, 4, 16, 24) == -1                                        # even T
    assert op(8, 3, 0, 1, 7, 3, 3) == -1                                          # H*W*3 not a multiple of 4
    assert op(8, 3, 3, 2, 7, 16, 24) == -1 and b"last" in lib.pfnl_last_error()   # a centre frame beyond `last`
    assert op(4, 20, 10, 3, 7, 16, 24) == -1 and b"ring" in lib.pfnl_last_error()  # 9 frames named, 4 slots


@pytest.mark.parametrize("T", [3, 5, 7])
def test_scheduling_rule_forms_the_harness_batches(T):
    from pfnl_amd.model import sliding_windows
    from pfnl_amd.stream import next_batch
    for batch in range(1, 6):
        for F in range(0, 21):
            launches = []                                                        # (pushed at launch, ended, first, count)
            launched = 0

            def drain(pushed, ended):
                nonlocal launched
                while True:
                    first, count = next_batch(T, batch, pushed, ended, launched)
                    assert first == launched
                    if count == 0:
                        return
                    launches.append((pushed, ended, first, count))
                    launched += count

            drain(0, False)
            for pushed in range(1, F + 1):
                drain(pushed, False)
            assert launched <= max(F - T // 2, 0)                                # the remainder waits for `ended`
            drain(F, True)
            want = [(k * batch, min(batch, F - k * batch)) for k in range((F + batch - 1) // batch)]
            assert [(f, c) for _, _, f, c in launches] == want, (T, batch, F)
            if F == 0:
                assert launches == []
                continue
            windows = sliding_windows(np.arange(F), T)                           # [F,T]: the frame index in every slot
            for pushed, ended, first, count in launches:
                need = first + count - 1 + T // 2                                # the last window's newest frame
                if not ended:
                    assert count == batch and pushed == need + 1                 # at the FIRST push that has it, not later
                else:
                    assert need + 1 > F                                          # it could not have launched before the end
                last = pushed - 1
                for w in range(count):
                    idx = np.clip(first + w + np.arange(T) - T // 2, 0, last)    # what the session's gather names
                    assert np.array_equal(idx, windows[first + w]), (T, batch, F, first, w)
