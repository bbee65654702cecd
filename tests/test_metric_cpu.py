"""Fusion-quality metric entry points without a GPU: argument validation before any launch, and the stock-torch fallbacks of
calc_msssim (use_padding=True, images below 161 px) against golden F19."""
import ctypes as C

import numpy as np
import pytest
import torch

import metric_cases as MC
from mmif._lib import lib

P = C.c_void_p(0x1000)   # never dereferenced: every call below must fail validation first
NUL = None
TAPS = (C.c_float * 34)()


def _err():
    return lib.mmif_last_error().decode()


def test_moments_validation():
    imgs = (C.c_void_p * 3)(0x1000, 0x1000, 0x1000)
    ws = lib.mmif_metric_moments_workspace(2, 64, 64, 3)
    assert ws > 0 and lib.mmif_metric_moments_workspace(2, 64, 64, 4) == 0
    assert lib.mmif_metric_moments(imgs, 4, 2, 64, 64, P, P, ws, None) != 0 and "k must be 1, 2 or 3" in _err()
    assert lib.mmif_metric_moments(imgs, 0, 2, 64, 64, P, P, ws, None) != 0 and "k must be 1, 2 or 3" in _err()
    assert lib.mmif_metric_moments(None, 3, 2, 64, 64, P, P, ws, None) != 0 and "NULL" in _err()
    assert lib.mmif_metric_moments(imgs, 3, 2, 64, 64, NUL, P, ws, None) != 0 and "NULL" in _err()
    nul = (C.c_void_p * 3)(0x1000, 0, 0x1000)
    assert lib.mmif_metric_moments(nul, 3, 2, 64, 64, P, P, ws, None) != 0 and "NULL image 1" in _err()
    assert lib.mmif_metric_moments(imgs, 3, 2, 1, 64, P, P, ws, None) != 0 and "at least 2x2" in _err()
    assert lib.mmif_metric_moments(imgs, 3, 2, 64, 64, P, P, ws - 1, None) == -3 and "workspace too small" in _err()


def test_hist_entropy_validation():
    assert lib.mmif_metric_hist(P, NUL, 1, 8, 8, P, P, P, None) != 0 and "NULL" in _err()
    assert lib.mmif_metric_hist(P, P, 1, 8, 8, P, P, NUL, None) != 0 and "NULL" in _err()
    assert lib.mmif_metric_hist(P, P, 0, 8, 8, P, P, P, None) != 0 and "empty" in _err()
    assert lib.mmif_metric_entropy(P, P, NUL, 1, 64, P, None) != 0 and "NULL" in _err()
    assert lib.mmif_metric_entropy(P, P, P, 1, 0, P, None) != 0 and "positive" in _err()


def test_qabf_validation():
    ws = lib.mmif_metric_qabf_workspace(1, 32, 32)
    assert lib.mmif_metric_qabf(P, P, NUL, 1, 32, 32, 1.5, P, P, ws, None) != 0 and "NULL" in _err()
    assert lib.mmif_metric_qabf(P, P, P, 1, 1, 32, 1.5, P, P, ws, None) != 0 and "at least 2x2" in _err()
    assert lib.mmif_metric_qabf(P, P, P, 1, 32, 32, 1.5, P, P, ws - 8, None) == -3 and "workspace too small" in _err()


def test_vif_validation():
    assert lib.mmif_metric_vif_workspace(1, 40, 64) == 0 and lib.mmif_metric_vif_workspace(1, 41, 41) > 0
    ws = lib.mmif_metric_vif_workspace(1, 41, 45)
    assert lib.mmif_metric_vif(P, P, P, 1, 41, 45, None, P, P, ws, None) != 0 and "NULL" in _err()
    assert lib.mmif_metric_vif(P, P, P, 1, 40, 64, TAPS, P, P, 1 << 30, None) != 0 and "at least 41x41" in _err()
    assert lib.mmif_metric_vif(P, P, P, 1, 64, 40, TAPS, P, P, 1 << 30, None) != 0 and "at least 41x41" in _err()
    assert lib.mmif_metric_vif(P, P, P, 1, 41, 45, TAPS, P, P, ws - 8, None) == -3 and "workspace too small" in _err()


def test_msssim_validation():
    ws = lib.mmif_metric_msssim_workspace(1, 161, 161)
    assert lib.mmif_metric_msssim(P, None, NUL, 1, 161, 161, 255.0, P, P, ws, None) != 0 and "NULL" in _err()
    assert lib.mmif_metric_msssim(P, None, P, 1, 160, 200, 255.0, P, P, 1 << 30, None) != 0 and "161x161" in _err()
    assert lib.mmif_metric_msssim(P, None, P, 1, 161, 161, 255.0, P, P, ws - 4, None) == -3 and "workspace too small" in _err()


def test_python_validation_without_gpu():
    import core.metric as M
    x = torch.zeros(1, 1, 64, 64)
    with pytest.raises(RuntimeError):
        M.calc_std(x)
    with pytest.raises(RuntimeError):
        M.fusion_metrics(x[0], x[0], x[0])
    with pytest.raises(ValueError, match="41"):
        M.calc_viff(x[..., :40, :], x[..., :40, :], x[..., :40, :])
    assert M.__all__ == ['calc_mean', 'calc_std', 'calc_ag', 'calc_sf', 'calc_mse', 'calc_psnr', 'calc_cc', 'calc_scd', 'calc_entropy',
                         'calc_cross_ent', 'calc_mul_info', 'calc_Qabf', 'calc_Nabf', 'calc_Labf', 'calc_ssim', 'calc_msssim', 'calc_viff']


@pytest.mark.parametrize("case", list(MC.CASES))
def test_stock_msssim_fallbacks_match_reference(case):
    import core.metric as M
    f19 = MC.load_f19()
    a, b, f = (torch.from_numpy(x) for x in MC.build(case, f19))
    got = float(M.calc_msssim(a, f, use_padding=True))
    ref = float(f19[f"{case}|msssim_pad|64"])
    assert abs(got - ref) <= 1e-4 * abs(ref), (case, got, ref)
    if min(a.shape[-2:]) < M.MSSSIM_MIN:
        got = float(M.calc_msssim(a, f))
        ref = float(f19[f"{case}|msssim|64"])
        assert abs(got - ref) <= 1e-4 * abs(ref), (case, got, ref)
