"""The fp64 definition of the reflect-padded SSIM losses (tests/ssim_pad_cases.py) is what the reference computes, and the padding /
fold mistakes a kernel could make are far from it: (a) it equals torch float64 autograd of core/_stock.py's composition, value and
gradient, every mode; (b) it reproduces golden F16 (captured from the reference) at the bars of tests/test_stock_fallbacks_cpu.py;
(c) on every case of the GPU sweep's table the gradient of each wrong-but-plausible variant differs by at least 0.1 max|grad|;
(d) the new entry points refuse bad arguments before anything is launched.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
import ssim_pad_cases as PC
from oracle.fusion_oracle import closed_form_image

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------ (a) torch float64 autograd
def _autograd_params():
    """three shapes per mode, (81, 81) in all; (11, 11) where F.pad accepts it ('ms-ssim' pads a 6-pixel level by 5 at 81)"""
    for mode in PC.MODES:
        small = [('r255', 97, 83, 2, 0), ('wide', 161, 176, 1, 0)] if mode == 'ms-ssim' else [('rand', 11, 11, 2, 0), ('r255', 33, 47, 3, 0)]
        for case in small + [('cf', 81, 81, 1, 0)]:
            yield pytest.param(mode, case, id=f"{mode}-{LC.case_id(case)}")


@pytest.mark.parametrize("mode,case", list(_autograd_params()))
def test_definition_equals_torch_float64_autograd(mode, case):
    from core import _stock
    dr = PC.data_range(case)
    a, b, f = (torch.from_numpy(x) for x in LC.f64(*PC.build(case)))
    f.requires_grad_(True)
    loss = _stock.ssim_loss(mode, a, b, f, dr, True, PC.WEIGHT)
    loss.backward()
    want_l, want_g = PC.pad_loss(a.numpy(), b.numpy(), f.detach().numpy(), mode, PC.WEIGHT, dr)
    assert abs(want_l - loss.item()) <= 1e-10 * abs(loss.item()), (want_l, loss.item())
    assert _rel(want_g, f.grad.numpy()) <= 1e-10


@pytest.mark.parametrize("win", PC.WINDOWS)
def test_term_means_equal_the_stock_composition(win):
    from core import _stock
    a, _, f = LC.f64(*PC.build(('wide', win, win + 1, 2, 0)))
    got = PC.pad_terms(a, f, win)
    want = _stock.ssim_terms(torch.from_numpy(a), torch.from_numpy(f), win, 1.0, True, True, _stock.window(win).double())
    for k in ('ssim', 'cs', 'sigma'):
        assert _rel(got[k], want[k].numpy()) <= 1e-10, k


# ------------------------------------------------------------------ (b) golden F16
@pytest.fixture(scope="module")
def f16():
    return np.load(os.path.join(G, "f16_stock_fallbacks.npz"))


@pytest.mark.parametrize("mode,shape", [("ssim", (2, 1, 40, 52)), ("w-ssim", (2, 1, 40, 52)), ("msw-ssim", (2, 1, 40, 52)),
                                        ("ms-ssim", (1, 1, 192, 208))])
def test_definition_reproduces_golden_f16_losses(f16, mode, shape):
    trip = LC.f64(*(closed_form_image(shape, p) for p in (0.3, 1.7, 2.9)))
    loss, grad = PC.pad_loss(*trip, mode, 0.7)
    assert abs(loss - float(f16[f"pad_{mode}__loss"])) <= 2e-6
    assert _rel(grad, f16[f"pad_{mode}__grad"]) <= 1e-4


def test_definition_reproduces_golden_f16_modules(f16):
    i1, f = LC.f64(closed_form_image((2, 1, 40, 52), 0.3), closed_form_image((2, 1, 40, 52), 2.9))
    t = PC.pad_terms(i1, f, 7)
    for k in ("ssim", "cs", "sigma"):
        assert t[k].shape == f16[f"ssim_pad7__{k}"].shape
        assert _rel(t[k], f16[f"ssim_pad7__{k}"]) <= 2e-5, k
    big = (1, 1, 192, 208)
    a, f = LC.f64(closed_form_image(big, 0.3), closed_form_image(big, 2.9))
    loss, _ = PC.pad_loss(a, a, f, 'ms-ssim', 1.0, need_grad=False)      # loss(a, a, f) = 1 - ms(a, f)
    assert _rel([1.0 - loss], f16["msssim_pad"]) <= 2e-5


# ------------------------------------------------------------------ (c) wrong-but-plausible variants
@pytest.mark.parametrize("mode,case", PC.all_loss_cases(), ids=[f"{m}-{PC.case_id(c)}" for m, c in PC.all_loss_cases()])
def test_wrong_padding_variants_are_far_from_the_definition(mode, case):
    """the gradient separates them; the value does not (the 'symmetric' variant comes within 4e-5 of the value at msw-ssim 33 x 47)"""
    _, want = PC.reference(mode, case)
    trip = LC.f64(*PC.build(case))
    for name, padding in PC.VARIANTS.items():
        _, g = PC.pad_loss(*trip, mode, PC.WEIGHT, PC.data_range(case), padding=padding)
        gap = _rel(g, want)
        print(f"{mode} {PC.case_id(case)} {name}: gradient gap {gap:.3f}")
        assert gap >= 0.1, (name, gap)


def test_variant_paddings_are_adjoint_pairs():
    """<pad(x), y> == <x, unpad(y)> for every variant that claims a fold, and for the definition's own pair"""
    rng = np.random.default_rng(5)
    x, y = rng.random((2, 1, 7, 9)), rng.random((2, 1, 17, 19))
    for name, (pad, unpad) in dict(PC.VARIANTS, reflect=PC.REFLECT).items():
        if name == 'no-fold':
            continue
        assert abs((pad(x, 5) * y).sum() - (x * unpad(y, 5)).sum()) <= 1e-12 * (x.size + y.size), name


# ------------------------------------------------------------------ (d) host argument checks
def test_c_abi_validation_of_the_padded_entry_points_without_gpu():
    from mmif._lib import lib
    f = (ctypes.c_float * 16)()
    big = 1 << 30
    assert lib.mmif_ssim_loss_pad(f, f, f, 1, 32, 32, 1.0, 1.0, 4, f, None, f, big, None) == -1
    assert b"only supported ['ssim', 'w-ssim', 'ms-ssim', 'msw-ssim'] mode" in lib.mmif_last_error()
    assert lib.mmif_ssim_loss_pad(f, f, f, 1, 32, 32, 1.0, 1.0, -1, f, None, f, big, None) == -1
    for mode in (0, 1, 3):
        assert lib.mmif_ssim_loss_pad(f, f, f, 1, 10, 10, 1.0, 1.0, mode, f, None, f, big, None) == -1
        assert b"smaller than the 11x11 window (10x10)" in lib.mmif_last_error()
        assert lib.mmif_ssim_loss_pad(f, f, f, 1, 11, 10, 1.0, 1.0, mode, f, None, f, big, None) == -1
    for h, w in ((80, 80), (81, 80), (80, 200)):
        assert lib.mmif_ssim_loss_pad(f, f, f, 1, h, w, 1.0, 1.0, 2, f, None, f, big, None) == -1
        assert b"at least 81x81" in lib.mmif_last_error()
    assert lib.mmif_ssim_loss_pad(None, f, f, 1, 32, 32, 1.0, 1.0, 0, f, None, f, big, None) == -1
    for mode, (h, w) in ((0, (11, 11)), (1, (32, 33)), (2, (81, 81)), (3, (11, 11))):
        need = lib.mmif_ssim_loss_pad_workspace(2, h, w, mode)
        assert need > 0
        assert lib.mmif_ssim_loss_pad(f, f, f, 2, h, w, 1.0, 1.0, mode, f, None, f, need - 1, None) == -3
        assert b"workspace too small" in lib.mmif_last_error()
        # no padded image or gradient buffer: the unpadded layout of the same mode ('ssim' takes 'w-ssim''s)
        assert need == lib.mmif_ssim_loss_mode_workspace(2, h, w, max(mode, 1))
    assert lib.mmif_ssim_terms_pad(f, f, 1, 32, 32, 4, 1.0, f, f, big, None) == -1
    assert b"win_size must be 3, 5, 7, 9 or 11" in lib.mmif_last_error()
    assert lib.mmif_ssim_terms_pad(f, f, 1, 6, 7, 7, 1.0, f, f, big, None) == -1
    assert lib.mmif_ssim_terms_pad(f, f, 1, 7, 7, 7, 1.0, f, f, 16, None) == -3
