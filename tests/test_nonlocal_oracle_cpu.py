"""Golden F21 on the CPU: the numpy float64 restatement of spatial_pooling(x, 'nl') in tests/nonlocal_cases.py (explicit backward
formulas, the ones csrc/nonlocal.hip implements) against the reference's own float64 results, the tie guard of every case, and the
argument validation of the three mmif_nonlocal_spatial_* entry points (which runs before any launch, so it needs no GPU)."""
import ctypes
import os

import numpy as np
import pytest

import nonlocal_cases as NC


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(NC.F21) <= 802015, "f21_nonlocal.npz must not outgrow the largest older fixture (f3_conv.npz)"
    return np.load(NC.F21)


@pytest.mark.parametrize("name", list(NC.CASES))
def test_numpy_restatement_meets_the_reference_fixture(golden, name):
    x, g = NC.inputs(name), NC.upstream(name)
    assert x.min() >= 0 and x.max() > 0
    o = NC.nonlocal_f64(x, g)
    idx = NC.sample_index(x.size)
    for key in ("y", "dx"):
        ref = golden[f"{name}|{key}"]
        assert ref.shape == idx.shape and np.abs(ref).max() > 0
        err = np.abs(o[key].reshape(-1)[idx] - ref).max() / np.abs(ref).max()
        assert err <= 1e-10, (name, key, err)
    assert abs(o["lo"] - golden[f"{name}|lo"]) <= 1e-12 * abs(o["hi"]) and abs(o["hi"] - golden[f"{name}|hi"]) <= 1e-12 * abs(o["hi"])


@pytest.mark.parametrize("name", list(NC.CASES))
def test_tie_guard_holds(name):
    """unique extrema (torch splits the gradient across ties: such inputs are not in the table) and a range that is not tiny"""
    o = NC.nonlocal_f64(NC.inputs(name))
    assert o["gap_lo"] > NC.TIE_GAP and o["gap_hi"] > NC.TIE_GAP, (name, o["gap_lo"], o["gap_hi"])
    assert o["hi"] - o["lo"] > 1e-3 * abs(o["hi"])


def test_m1_case_is_the_identity_plus_the_pooled_row():
    """M = 1: S == 1, so y = x + P whatever lo and hi are, and dZ == 0"""
    x = NC.inputs("m1")
    o = NC.nonlocal_f64(x, NC.upstream("m1"))
    assert np.allclose(o["y"], x.astype(np.float64) + NC.pool8(x.astype(np.float64)), rtol=0, atol=1e-14)


def test_scale2_case_couples_the_samples():
    """the global min / max runs over the batch: sample 0's attention term (y - x) alone differs from the one it gets inside the batch by
    far more than any fp32 tolerance used on this case"""
    x = NC.inputs("scale2")
    both, alone = NC.nonlocal_f64(x)["y"][0], NC.nonlocal_f64(x[:1])["y"][0]
    assert np.abs(both - alone).max() > 1e-3 * np.abs(both - x[0]).max()
    assert np.abs(both - alone).max() > 5e-4 * np.abs(both).max()


def test_nonlocal_c_abi_exists_and_validates_before_any_launch():
    from mmif._lib import SIGNATURES, lib
    for name in ("mmif_nonlocal_spatial_workspace", "mmif_nonlocal_spatial_fwd", "mmif_nonlocal_spatial_bwd"):
        assert name in SIGNATURES and hasattr(lib, name), name
    f = (ctypes.c_float * 64)()
    big = 1 << 30
    ws_fn, fwd, bwd = lib.mmif_nonlocal_spatial_workspace, lib.mmif_nonlocal_spatial_fwd, lib.mmif_nonlocal_spatial_bwd
    for n, c, h, w in ((1, 16, 7, 16), (1, 16, 16, 7), (1, 0, 16, 16), (1, 257, 16, 16), (0, 16, 16, 16)):
        assert ws_fn(n, c, h, w) == 0
        assert fwd(f, f, f, f, n, c, h, w, f, big, None) == -1
        assert b"h, w >= 8" in lib.mmif_last_error() and b"mmif_nonlocal_spatial_fwd" in lib.mmif_last_error()
        assert bwd(f, f, f, f, f, f, n, c, h, w, f, big, None) == -1
        assert b"mmif_nonlocal_spatial_bwd" in lib.mmif_last_error()
    assert fwd(None, f, f, f, 1, 16, 16, 16, f, big, None) == -1
    assert b"null pointer" in lib.mmif_last_error()
    assert fwd(f, f, f, f, 1, 16, 16, 16, None, big, None) == -1
    assert bwd(f, f, f, f, None, f, 1, 16, 16, 16, f, big, None) == -1
    assert b"null pointer" in lib.mmif_last_error()
    need = ws_fn(1, 16, 16, 16)
    assert need > 0
    assert fwd(f, f, f, f, 1, 16, 16, 16, f, need - 1, None) == -3
    assert bwd(f, f, f, f, f, f, 1, 16, 16, 16, f, need - 1, None) == -3
    assert b"workspace" in lib.mmif_last_error()
    assert ws_fn(4, 112, 64, 64) > ws_fn(2, 112, 64, 64) > ws_fn(1, 112, 64, 64) > 0
    assert ws_fn(1, 256, 8, 8) > 0 and ws_fn(1, 1, 8, 8) > 0
    # the capability itself: far below one energy tensor (N * M * 4 bytes) at the training shape
    assert ws_fn(1, 112, 256, 256) < 65536 * 1024 * 4 // 4


def test_cpu_tensors_keep_the_composition(monkeypatch):
    """CPU tensors (and shapes outside the kernels' limits) stay on the tensor-level composition, under either switch setting"""
    import torch
    from core.fusion import spatial_pooling
    x = NC.inputs("b3c7")
    ref = NC.nonlocal_f64(x)["y"]
    for impl in ("hip", "torch"):
        monkeypatch.setenv("MMIF_NONLOCAL", impl)
        y = spatial_pooling(torch.from_numpy(x), 'nl').numpy()
        assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max()
    monkeypatch.setenv("MMIF_NONLOCAL", "triton")
    with pytest.raises(ValueError, match="MMIF_NONLOCAL"):
        spatial_pooling(torch.from_numpy(x), 'nl')
