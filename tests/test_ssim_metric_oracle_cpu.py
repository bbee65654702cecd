"""The metric-side SSIM / MS-SSIM without a GPU: the float64 definition of tests/ssim_metric_cases.py against the reference (golden F21,
tests/golden/make_golden_metric_ssim.py), the host-built window bit for bit, the argument validation of mmif_metric_ssim_maps and
mmif_metric_msssim_any before any launch, and the distance of every wrong-but-plausible variant from the definition."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ssim_metric_cases as SC
from mmif._lib import lib

P = C.c_void_p(0x1000)   # never dereferenced: every call below must fail validation first
F21 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F21_metric_ssim.npz")


@pytest.fixture(scope="module")
def f21():
    return np.load(F21)


def _err():
    return lib.mmif_last_error().decode()


@pytest.mark.parametrize("name", SC.SSIM_CASES)
def test_definition_matches_reference_maps(name, f21):
    ref = SC.reference(name)
    assert tuple(f21[f"{name}|shape"]) == ref["ssim"].shape, name
    want = f21[f"{name}|means"]
    assert abs(float(ref["ssim_pooled"]) - want[0]) <= 1e-10 and abs(float(ref["cs_pooled"]) - want[1]) <= 1e-10, name
    if f"{name}|ssim" in f21.files:
        assert np.abs(ref["ssim"] - f21[f"{name}|ssim"]).max() <= 1e-10 and np.abs(ref["cs"] - f21[f"{name}|cs"]).max() <= 1e-10, name


@pytest.mark.parametrize("name", SC.MS_CASES)
def test_definition_matches_reference_msssim(name, f21):
    ref = SC.reference(name)
    assert abs(float(ref["pooled"]) - float(f21[f"{name}|pooled"][0])) <= 1e-10, name
    assert np.abs(ref["value"] - f21[f"{name}|value"]).max() <= 1e-10, name


def test_map_extents_of_the_issue():
    """a 2 x 2 image gives a 3 x 3 padded map; 20 x 23 with win_size 8 gives 21 x 24; 10 x 10 padded is the 11 x 11 map"""
    z = np.zeros((1, 1, 2, 2), np.float32)
    assert SC.maps(z, z, 11, True)[0].shape[-2:] == (3, 3)
    z = np.zeros((1, 1, 20, 23), np.float32)
    assert SC.maps(z, z, 8, True)[0].shape[-2:] == (21, 24) and SC.maps(z, z, 8, False)[0].shape[-2:] == (13, 16)
    z = np.zeros((1, 1, 10, 10), np.float32)
    assert SC.maps(z, z, 11, True)[0].shape[-2:] == (11, 11)


def test_anti_cases_engage_the_clamp_and_const_is_one():
    for name in SC.MS_CASES:
        if name.endswith("anti"):
            assert (SC.reference(name)["levels"][:4] < 0).any(), name
    z = np.full((1, 1, 12, 12), 77.0, np.float32)
    assert float(SC.maps(z, z, 1, False)[0].min()) == 1.0            # a 1-tap window has weight exactly 1


@pytest.mark.parametrize("k", range(1, 12))
def test_host_window_bit_for_bit(k, f21):
    taps = (C.c_float * k)()
    win = (C.c_float * (k * k))()
    assert lib.mmif_metric_ssim_window(k, taps, win) == 0, _err()
    got_t, got_w = np.array(taps, np.float32), np.array(win, np.float32).reshape(k, k)
    assert np.array_equal(got_t.view(np.uint32), f21[f"taps|{k}"].view(np.uint32)), (k, got_t, f21[f"taps|{k}"])
    assert np.array_equal(got_w.view(np.uint32), f21[f"window|{k}"].view(np.uint32)), k
    # and the definition's own window is the reference's
    assert np.array_equal(SC.window(k).numpy().view(np.uint32), f21[f"window|{k}"].view(np.uint32)), k


def test_window_validation():
    buf = (C.c_float * 121)()
    assert lib.mmif_metric_ssim_window(0, buf, buf) == -1 and "1..11" in _err()
    assert lib.mmif_metric_ssim_window(12, buf, buf) == -1 and "1..11" in _err()
    assert lib.mmif_metric_ssim_window(3, None, buf) == -1 and "NULL" in _err()


def test_ssim_maps_validation():
    ws = lib.mmif_metric_ssim_maps_workspace(2, 20, 23, 8, 1)
    assert ws >= 2 * 2 * 4 * 8                                        # 21 x 24 map: 2 x 2 tiles, two fp64 sums each, two samples
    assert lib.mmif_metric_ssim_maps_workspace(2, 20, 23, 8, 0) >= 2 * 2 * 1 * 8
    assert lib.mmif_metric_ssim_maps_workspace(1, 64, 64, 12, 0) == 0 and lib.mmif_metric_ssim_maps_workspace(0, 64, 64, 11, 0) == 0
    assert lib.mmif_metric_ssim_maps_workspace(1, 5, 64, 12, 0) > 0   # the window shrinks to 5
    call = lib.mmif_metric_ssim_maps
    assert call(None, P, 2, 20, 23, 8, 1, 255.0, P, P, P, P, ws, None) == -1 and "NULL image" in _err()
    assert call(P, None, 2, 20, 23, 8, 1, 255.0, P, P, P, P, ws, None) == -1 and "NULL image" in _err()
    assert call(P, P, 0, 20, 23, 8, 1, 255.0, P, P, P, P, ws, None) == -1 and "n=0" in _err()
    assert call(P, P, 2, 20, 23, 0, 1, 255.0, P, P, P, P, ws, None) == -1 and "win_size" in _err()
    assert call(P, P, 2, 20, 23, -3, 1, 255.0, P, P, P, P, ws, None) == -1 and "win_size" in _err()
    assert call(P, P, 2, 20, 23, 12, 0, 255.0, P, P, P, P, 1 << 30, None) == -1 and "up to 11" in _err()
    assert call(P, P, 2, 20, 23, 8, 1, 255.0, None, None, None, P, ws, None) == -1 and "no output" in _err()
    assert call(P, P, 2, 20, 23, 8, 1, 255.0, P, P, P, P, ws - 8, None) == -3 and "workspace too small" in _err()
    assert call(P, P, 2, 20, 23, 8, 1, 255.0, None, None, P, None, ws, None) == -3 and "workspace too small" in _err()


def test_msssim_any_validation():
    ws = lib.mmif_metric_msssim_any_workspace(2, 40, 40)
    assert ws > 0 and lib.mmif_metric_msssim_any_workspace(2, 8, 40) == 0 and lib.mmif_metric_msssim_any_workspace(2, 9, 9) > 0
    call = lib.mmif_metric_msssim_any
    assert call(None, P, P, 2, 40, 40, 11, 0, 255.0, P, P, ws, None) == -1 and "NULL" in _err()
    assert call(P, None, None, 2, 40, 40, 11, 0, 255.0, P, P, ws, None) == -1 and "NULL" in _err()
    assert call(P, None, P, 2, 40, 40, 11, 0, 255.0, None, P, ws, None) == -1 and "NULL" in _err()
    assert call(P, P, P, 0, 40, 40, 11, 0, 255.0, P, P, ws, None) == -1 and "n=0" in _err()
    assert call(P, P, P, 2, 40, 40, 0, 0, 255.0, P, P, ws, None) == -1 and "win_size" in _err()
    assert call(P, P, P, 2, 8, 8, 11, 0, 255.0, P, P, 1 << 30, None) == -1 and "9x9" in _err()
    assert call(P, P, P, 2, 300, 8, 11, 1, 255.0, P, P, 1 << 30, None) == -1 and "9x9" in _err()
    assert call(P, P, P, 2, 40, 40, 12, 0, 255.0, P, P, 1 << 30, None) == -1 and "up to 11" in _err()
    assert call(P, P, P, 2, 40, 40, 11, 0, 255.0, P, P, ws - 8, None) == -3 and "workspace too small" in _err()
    assert call(P, P, P, 2, 40, 40, 11, 0, 255.0, P, None, ws, None) == -3 and "workspace too small" in _err()


def test_python_routes_without_gpu():
    """CPU tensors keep the stock composition (and its errors); windows above 11 and MS-SSIM below 9 px do too"""
    import core.metric as M
    a, b = (torch.from_numpy(np.array(x)) for x in SC.build("ssim-20x23-b1-k8-pad-rand255"))
    s, c = M.calc_ssim(a, b, 8, 255.0, True, False, True)
    ref = SC.reference("ssim-20x23-b1-k8-pad-rand255")
    assert s.dtype == torch.float32 and tuple(s.shape) == ref["ssim"].shape
    assert np.abs(s.numpy() - ref["ssim"]).max() <= ref["tol"]["ssim"] and np.abs(c.numpy() - ref["cs"]).max() <= ref["tol"]["cs"]
    with pytest.raises(RuntimeError):
        M.calc_msssim(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8), use_padding=True)


@pytest.mark.parametrize("variant", SC.VARIANTS + SC.MS_VARIANTS)
def test_variants_are_far(variant):
    """each wrong-but-plausible variant lies at least 20 tolerances from the definition on at least one case"""
    names = SC.MS_CASES if variant in SC.MS_VARIANTS else SC.SSIM_CASES
    dist = {n: SC.variant_distance(n, variant) for n in names}
    dist = {n: d for n, d in dist.items() if d is not None}
    far = max(dist, key=dist.get)
    print(f"{variant}: farthest on {far} at {dist[far]:.3g} tolerances; cases at >= 20: {sum(d >= 20 for d in dist.values())} of {len(dist)}")
    assert dist[far] >= 20.0, (variant, far, dist[far])
