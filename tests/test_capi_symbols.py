"""The C-ABI library loads without a GPU and exports every symbol include/pfnl_hip.h declares;
argument validation that needs no device works; compute without a device fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "pfnl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pfnl_[a-z0-9_]+)\s*\(", text)))


def test_library_built_and_exports_header_symbols():
    assert os.path.exists(_capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(_capi.LIB_PATH)
    syms = _declared_symbols()
    assert len(syms) >= 19
    for s in syms:
        assert hasattr(lib, s), f"libpfnl_hip.so does not export {s}"
    assert set(syms) == set(_capi.SIGNATURES), "ctypes signatures and header disagree"


def test_abi_v4_and_argument_validation_without_gpu():
    """ABI version 4 (the _ex op hooks); arguments that need no device are refused before any HIP call."""
    lib = _capi.load_library()
    assert lib.pfnl_version() == 4
    dummy = C.c_void_p(16)                                                     # never dereferenced: the hooks return first
    chain = lambda mfma, n_full, s, q: lib.pfnl_op_conv2_chain_ex(dummy, dummy, None, dummy, 7, dummy, dummy, 14, 8, 32, 1,  # noqa: E731
                                                                  mfma, n_full, s, q, None)
    assert chain(8, 0, 0, 0) == -1 and b"mfma" in lib.pfnl_last_error()
    assert chain(16, 8, 2, 4) == -1 and b"32x32x16" in lib.pfnl_last_error()
    assert lib.pfnl_op_conv3x3_bf16_ex(dummy, dummy, None, dummy, 7, dummy, dummy, 14, 8, 32, 1, 64, 0, 0, 0, None) == -1
    assert b"mfma" in lib.pfnl_last_error()
    assert lib.pfnl_op_conv3x3_bf16_ex(dummy, dummy, None, None, 7, None, dummy, 14, 8, 32, 1, 16, 0, 0, 0, None) == -1
    assert b"NULL" in lib.pfnl_last_error()
    for f32 in (0, 1):                                                         # pfnl_op_conv0_ex: an addition to v4, same checks as pfnl_op_conv0
        assert lib.pfnl_op_conv0_ex(None, dummy, None, dummy, 1, 7, 8, 8, f32, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert lib.pfnl_op_conv0_ex(dummy, dummy, None, dummy, 1, 4, 8, 8, f32, None) == -1 and b"geometry" in lib.pfnl_last_error()
    assert lib.pfnl_op_conv0_bf16(None, dummy, None, dummy, 1, 7, 8, 8, None) == -1 and b"NULL" in lib.pfnl_last_error()   # and its bf16 form
    assert lib.pfnl_op_conv0_bf16(dummy, dummy, None, None, 1, 7, 8, 8, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_op_conv0_bf16(dummy, dummy, None, dummy, 1, 4, 8, 8, None) == -1 and b"geometry" in lib.pfnl_last_error()
    assert lib.pfnl_op_conv0_bf16(dummy, dummy, None, dummy, 1, 7, 7, 8, None) == -1 and b"geometry" in lib.pfnl_last_error()
    h = C.c_void_p()
    bad = _capi.pfnl_config(4, 4, 64, 20, 0, (C.c_int32 * 3)(0, 0, 0))        # even num_frames
    assert lib.pfnl_create(C.byref(bad), C.byref(h)) == -1
    assert b"num_frames" in lib.pfnl_last_error()
    bad = _capi.pfnl_config(7, 3, 64, 20, 0, (C.c_int32 * 3)(0, 0, 0))        # scale 3
    assert lib.pfnl_create(C.byref(bad), C.byref(h)) == -1
    assert lib.pfnl_create(None, C.byref(h)) == -1


def test_no_cpu_fallback():
    """Without a device the product path must fail, not quietly compute somewhere else."""
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    from pfnl_amd.engine import PFNLEngine
    with pytest.raises(_capi.PFNLHipError, match="no HIP device"):
        PFNLEngine()
    from model.pfnl import PFNL
    with pytest.raises(_capi.PFNLHipError):
        PFNL().forward(np.zeros((1, 7, 8, 8, 3), np.float32))


def test_no_store_data_hazard_in_emitted_isa():
    """tools/lint_store_hazard.py over every kernel source: no VALU write to the data registers of a 16-byte buffer store
    with an SGPR offset within two issue slots (pfnl_amd/csrc/common.h, buffer_store_b128_guarded); and (round 5) no inline-asm
    instruction reading a register an MFMA wrote fewer than 11 issue slots earlier, no instruction at all reading the result of an
    inline-asm MFMA inside that window - the compiler pads neither (a fold of accumulators written as inline asm read them one MFMA
    after they were issued: repeatable at -O3, run-to-run noise in the -O1 ASAN build)."""
    import shutil
    import subprocess
    import sys

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    st = subprocess.run([sys.executable, os.path.join(root, "tools", "lint_store_hazard.py"), "--selftest"], capture_output=True, text=True)
    assert st.returncode == 0, st.stdout + st.stderr                 # the rule fires on known-bad snippets (VGPR and AGPR destinations), not on good ones
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "lint_store_hazard.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
