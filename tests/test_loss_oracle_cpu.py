"""Pin the fp64 loss oracle (oracle/fusion_oracle.py: every mode of pixel_loss / grad_loss / ssim_loss / ssim_mode_loss / tv_loss /
fusion_losses) to the reference's float64 modules and autograd (golden F20, tests/golden/make_golden_losses.py), prove the defaults of
the extended signatures unchanged against goldens F1 / F2 / F9, and hold the case table of the GPU sweep (tests/loss_cases.py) to its
exclusion cap with the oracle alone.  No GPU."""
import json
import os

import numpy as np
import pytest

import loss_cases as LC
from oracle import fusion_oracle as O
from test_oracle_golden import G, close, f2_inputs

# Both sides are fp64 on identical inputs and identical tap values; they differ by summation order only.
# Largest figures measured over F20: values 4.3e-16 relative, gradients 1.5e-14 of max|ref| ('msw-ssim' at data_range 255).
F20_VALUE_RTOL = 1e-12
F20_GRAD_RTOL = 1e-10

ENTRIES = LC.f20_entries()


@pytest.fixture(scope="module")
def f20():
    return dict(np.load(LC.F20))


def test_f20_manifest_matches_case_table():
    want = {k: {"kind": v["kind"], "args": v["args"], "cases": list(v["cases"])} for k, v in ENTRIES.items()}
    assert json.load(open(LC.F20_MANIFEST)) == want


def test_f20_no_array_is_all_zero(f20):
    assert len(f20) == 2 * sum(len(e["cases"]) for e in ENTRIES.values()) + len(LC.WIN_SIZES)
    for k, v in f20.items():
        assert v.dtype == np.float64 and np.isfinite(v).all() and np.abs(v).max() > 0.0, k


@pytest.mark.parametrize("k", LC.WIN_SIZES)
def test_window_taps_bit_for_bit(k, f20):
    """create_window(k) holds the reference's float32 values for every window size (the 3-tap window's normaliser is torch's float32
    sum, one ulp above the correctly rounded one)"""
    w = O.create_window(k)
    assert w.dtype == np.float32 and np.array_equal(w.astype(np.float64), f20[f"window|{k}"])


@pytest.mark.parametrize("name", list(ENTRIES))
def test_f20_fp64_oracle_vs_reference(name, f20):
    """value to 1e-12 relative, gradient to 1e-10 of max|ref| with no pixel left out"""
    entry = ENTRIES[name]
    for case in entry["cases"]:
        arrays = LC.f64(*LC.f20_inputs(entry["kind"], case))
        loss, grad = LC.oracle_f20(entry, arrays)
        ref_l, ref_g = float(f20[f"{name}|{case}|loss"]), f20[f"{name}|{case}|grad"]
        assert np.asarray(loss).dtype == np.float64 and grad.dtype == np.float64 and grad.shape == ref_g.shape, (name, case)
        ev = abs(float(loss) - ref_l) / abs(ref_l)
        eg = np.abs(grad - ref_g).max() / np.abs(ref_g).max()
        print(f"F20 {name} {case}: value {ev:.2e}, gradient {eg:.2e}")
        assert ev <= F20_VALUE_RTOL and eg <= F20_GRAD_RTOL, (name, case, ev, eg)


def test_f20_dyadic_cases_hold_exact_ties():
    """the fixture's 'dyadic' inputs tie exactly (d == 0, gx == 0) on some but not all pixels"""
    a, b, f = LC.f64(*LC.f20_inputs('pixel', 'dyadic-1x33x47'))
    for d in (f - np.maximum(a, b), f - a, O._sobel(f)[1][..., 1:-1], O._sobel(f)[2][..., 1:-1, :]):
        share = float((d == 0).mean())
        assert 0.001 < share < 0.9, share


def test_ms_ssim_clamps_of_the_anti_inputs():
    """'anti': every level mean of the first source is below the 1e-7 clamp, none of the second; 'anti2': both clamped, and the
    oracle's gradient is exactly zero"""
    win = O.create_window(11)
    a, b, f = LC.f64(*LC.triple('anti', 161, 176, 1, 0))
    for src, clamped in ((a, True), (b, False)):
        x, y = src, f
        for lvl in range(5):
            t = O.ssim_full_terms(x, y, win)
            v = float((t["cs"] if lvl < 4 else t["S"]).mean())
            assert (v < -0.01) if clamped else True, (lvl, v)
            x, y = O._avg_pool_pad(x), O._avg_pool_pad(y)
    _, g = O.ssim_mode_loss(a, b, f, 'ms-ssim')
    assert np.abs(g).max() > 0.0
    for shape in ((161, 161), (176, 177)):
        l, g = O.ssim_mode_loss(*LC.f64(*LC.triple('anti2', *shape, 2, 0)), 'ms-ssim')
        assert not g.any() and 0.0 < 1.0 - l < 2e-7, (shape, l)     # every level at the clamp: ms = prod 1e-7^w_i


# ------------------------------------------------------------------ defaults of the extended signatures: goldens F1 / F2 / F9
def test_defaults_unchanged_f1():
    import torch
    ref = json.load(open(os.path.join(G, "f1_loss_known_answer.json")))
    torch.manual_seed(0)
    x1, x2, y = (torch.rand(2, 1, 256, 256).numpy() for _ in range(3))
    for mode in ("avg", "max"):
        l, _ = O.pixel_loss(x1, x2, y, 0.01, mode, False, norm="l1")
        assert abs(l - ref[f"pixel_{mode}"]) < 1e-8 and l == O.pixel_loss(x1, x2, y, 0.01, mode, False)[0]
        l, _ = O.grad_loss(x1, x2, y, 0.1, mode, False, norm="l1")
        assert abs(l - ref[f"grad_{mode}"]) < 5e-7 and l == O.grad_loss(x1, x2, y, 0.1, mode, False)[0]
    (a, b, c, tot), _ = O.fusion_losses(x1, x2, y, need_grad=False, pixel_mode="max", grad_mode="max", pixel_norm="l1", grad_norm="l1", data_range=1.0)
    assert abs(a - ref["ssim"]) < 2e-6 and abs(tot - ref["total_max"]) < 3e-6
    assert (a, b, c, tot) == O.fusion_losses(x1, x2, y, need_grad=False)[0]


@pytest.mark.parametrize("case", list("abcd"))
def test_defaults_unchanged_f2(case):
    ref = np.load(os.path.join(G, "f2_loss_grads.npz"))
    i1, i2, f = f2_inputs(case)
    l2, g2 = O.pixel_loss(i1, i2, f, 0.01, "max", True, "l1")
    l3, g3 = O.grad_loss(i1, i2, f, 0.1, "max", True, "l1")
    assert abs(l2 - ref[f"{case}_l_pixel"]) < 1e-7 and abs(l3 - ref[f"{case}_l_grad"]) < 1e-6
    close(g2, ref[f"{case}_g_pixel"], 1e-6, "g_pixel")
    close(g3, ref[f"{case}_g_grad"], 1e-6, "g_grad")
    assert abs(O.pixel_loss(i1, i2, f, 0.01, "avg", False, "l1")[0] - ref[f"{case}_l_pixel_avg"]) < 1e-7
    assert abs(O.grad_loss(i1, i2, f, 0.1, "avg", False, "l1")[0] - ref[f"{case}_l_grad_avg"]) < 1e-6
    (a, b, c, tot), g = O.fusion_losses(i1, i2, f, pixel_mode="max", grad_mode="max", pixel_norm="l1", grad_norm="l1", data_range=1.0)
    assert abs(a - ref[f"{case}_l_ssim"]) < 3e-6 and b == l2 and c == l3
    close(g, ref[f"{case}_g_total"], 5e-3 if case == "c" else 2e-4, "g_total")
    (_, _, _, tot0), g0 = O.fusion_losses(i1, i2, f)
    assert tot0 == tot and np.array_equal(g0, g) and g.dtype == np.float32


def test_defaults_unchanged_f9():
    ref = np.load(os.path.join(G, "f9_ssim_modes.npz"))
    for mode, shape in (("w-ssim", (3, 1, 33, 47)), ("msw-ssim", (1, 1, 33, 47)), ("ms-ssim", (1, 1, 192, 208))):
        tag = f"{mode}_{shape[0]}x{shape[2]}x{shape[3]}"
        i1, i2, f = O.closed_form_image(shape, 0.3), O.closed_form_image(shape, 1.7), O.closed_form_image(shape, 2.9)
        loss, grad = O.ssim_mode_loss(i1, i2, f, mode, weight=0.7, data_range=1.0)
        assert grad.dtype == np.float32 and abs(float(loss) - float(ref[tag + "__loss"])) <= 2e-5
        close(grad, ref[tag + "__grad"], 2e-4, tag)


def test_l2_and_avg_satisfy_their_definitions():
    """the new arms against the definitions written out directly (fp64, finite differences of the value for the Sobel term)"""
    a, b, f = LC.f64(*LC.triple('rand', 7, 9, 2, 0))
    l, g = O.pixel_loss(a, b, f, 0.3, "avg", True, "l2")
    assert abs(l - 0.3 * 0.5 * (((f - a) ** 2).mean() + ((f - b) ** 2).mean())) < 1e-15
    assert np.abs(g - 0.3 * ((f - a) + (f - b)) / f.size).max() < 1e-16
    for mode in ("avg", "max"):
        l, g = O.grad_loss(a, b, f, 0.7, mode, True, "l2")
        rng = np.random.default_rng(0)
        d = rng.standard_normal(f.shape)
        eps = 1e-7
        num = (O.grad_loss(a, b, f + eps * d, 0.7, mode, False, "l2")[0] - O.grad_loss(a, b, f - eps * d, 0.7, mode, False, "l2")[0]) / (2 * eps)
        assert abs(num - float((g * d).sum())) <= 1e-6 * abs(num), (mode, num, float((g * d).sum()))
    with pytest.raises(ValueError):
        O.pixel_loss(a, b, f, 1.0, "max", True, "l3")


# ------------------------------------------------------------------ the exclusion cap, met by the oracle alone
def _l1_sobel_cases():
    seen, out = set(), []
    fused16 = [('rand', h, w, 2, 0) for h, w in LC.RAGGED]
    for case in LC.pixgrad_cases() + LC.fused_train_cases() + fused16:
        if case not in seen:
            seen.add(case)
            out.append(case)
    return out


@pytest.mark.parametrize("case", _l1_sobel_cases(), ids=LC.case_id)
def test_exclusion_cap_met_by_the_oracle(case):
    """every (distribution, shape) on which the sweep compares an l1 Sobel gradient: the pixels the rule of loss_cases.sobel_l1_excluded
    leaves out are at most 0.1 % of the case, none on images of fewer than 1000 pixels, and none at all on 'dyadic'"""
    a, b, f = LC.build(case)
    for mode in ("max", "avg"):
        excl = LC.sobel_l1_excluded(a, b, f, mode)
        LC.check_cap(excl, f"{LC.case_id(case)} {mode}")
        if case[0] == 'dyadic':
            assert not excl.any()
