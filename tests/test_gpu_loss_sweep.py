"""Loss kernels (core/loss.py on csrc/loss.hip and csrc/loss_modes.hip: value AND d/d(fused image)) against the fp64 oracle
(oracle/fusion_oracle.py on float64 copies of the same arrays; pinned to the reference's float64 autograd by golden F20 in
tests/test_loss_oracle_cpu.py) at the modes, shapes and edges the golden fixtures of test_gpu_loss.py do not hold: 'l2' and 'avg' arms,
data_range = 255, one-row SSIM maps, the ST = 32 / LT = 16 / MT_ = 16 tile edges, the Sobel reflect fold at h, w = 2 and 3, the
ms-ssim threshold with B > 1 and an active 1e-7 clamp, exact ties, 1024x1224, and the direct-read path of the fused finish kernel.
Inputs and case tables: tests/loss_cases.py.

Run time on one MI355X: 33 s for the 227 cases (the fp64 numpy oracle at 1024x1224 and at 64 x 256x256 is most of it).
"""
import numpy as np
import pytest
import torch

import loss_cases as LC
from oracle import fusion_oracle as O

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ tolerances
# Values: |got - ref| / max(|ref|, floor).  floor = 1e-3 x weight for the losses (weight x a mean of O(0.01 .. 1) quantities); 0.1 for
# the SSIM / MS_SSIM / MSW_SSIM modules, which return means of per-pixel values in [-1, 1] whose fp32 rounding error is absolute.
# Smooth gradients (every SSIM flavour, both l2 terms, the fused total): max|got - ref| / max|ref|.
# Each constant = largest error measured on an MI355X over this file (printed as LOSS_SWEEP_MARGINS, run with -s) times a margin of at
# most 4, never looser than 1e-4 (values), 3e-4 ('ssim' gradient) and 5e-4 (the other gradients), the bars test_gpu_loss.py holds.
# Measured, values: ssim 1.07e-6 (flat fused 26x27), ssim255 6.5e-8, pixel 1.59e-7 (l2 max wide 2x11x300), grad 1.62e-7 (l1 avg cf
# 2x3x3), tv 1.19e-7, w-ssim 5.1e-7 (anti 2x256x256), msw-ssim 6.4e-7 (anti 2x42x42), ms-ssim 4.6e-7 (rand 2x161x161), w-ssim255 7.4e-8,
# msw-ssim255 2.2e-7, fused total 2.4e-7 (rand 1x11x11); modules: SSIM terms 2.46e-5 (SSIM(3) 'ssim', flatsrc 1x64x80), MS_SSIM 1.7e-7, MSW_SSIM 2.7e-6.
# Measured, gradients: ssim 8.5e-6 (anti 3x42x42), ssim255 5.5e-7, pixel_l2 1.64e-7, grad_l2 2.09e-7 (wide 2x11x300), tv_l2 1.76e-7,
# w-ssim 1.35e-5 (anti 2x256x256), msw-ssim 2.33e-5 (rand 1x1024x1224), ms-ssim 1.27e-5 (rand 2x161x161), w-ssim255 6.2e-7, msw-ssim255
# 1.23e-5 (1x64x80), MSW_SSIM 4.5e-6, fused 1.04e-5 (mixed 16x40x56); l1: pixel 8.1e-8, Sobel 1.15e-7, tv 1.21e-7 (against GTOL_L1);
# flat fused 'ssim' 5.0e-7 (against GTOL_FLAT_FUSED).
VTOL = {
    'ssim': 4e-6, 'ssim255': 2.5e-7, 'pixel': 6e-7, 'grad': 6e-7, 'tv': 4.5e-7, 'w-ssim': 2e-6, 'msw-ssim': 2.5e-6, 'ms-ssim': 1.8e-6,
    'w-ssim255': 2.5e-7, 'msw-ssim255': 8e-7, 'terms': 9.8e-5, 'MS_SSIM': 6.5e-7, 'MSW_SSIM': 1e-5, 'fused': 9e-7,
}
MODULE_KEYS = ('terms', 'MS_SSIM', 'MSW_SSIM')
GTOL = {
    'ssim': 3e-5, 'ssim255': 2e-6, 'pixel_l2': 6e-7, 'grad_l2': 8e-7, 'tv_l2': 7e-7, 'w-ssim': 5e-5, 'msw-ssim': 9e-5, 'ms-ssim': 5e-5,
    'w-ssim255': 2.4e-6, 'msw-ssim255': 4.5e-5, 'MSW_SSIM': 1.8e-5, 'fused': 4e-5,
}
# A constant fused image has sigma_f^2 == 0 up to rounding: the clamp mask of the variance (sf_raw > 0) is decided by rounding noise in
# fp32 and in fp64 alike, and the reference's own gradient is ill-conditioned there (golden F2 case c holds 5e-3 for the same reason).
GTOL_FLAT_FUSED = 5e-3
# l1 gradients are piecewise constant: weight / count (one fp32 rounding) times a sum of small integers and halves (exact; TVLoss adds
# up to four such terms of two scales).  Where the sgn() decisions agree the result is within two fp32 ulps of the oracle's: the bar is
# 4 ulps of the largest entry.
GTOL_L1 = 4 * 2.0 ** -24
# img1 == img2 == imgf: every map pixel has m1 == m2 and v1 == v2 bit for bit, so S = m1 v1 (1 / (m2 v2)) is 1 to three fp32 roundings
# (2e-7); the mean of such values keeps that to the summation error of the fixed-order block sums (< 1e-6 relative).
SSIM_SELF_BOUND = 2e-6
FF_CAP = 12288      # csrc/loss.hip: floats of LDS staging in fusion_finish_kernel; longer partial lists are read directly

_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    print("\nLOSS_SWEEP_MARGINS (largest error per entry point): " + "; ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in sorted(_WORST.items())))


def _note(key, err, what):
    _WORST[key] = max(_WORST.get(key, (0.0, '')), (float(err), what))


def dev(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def check_value(got, ref, key, weight, what):
    err = abs(float(got) - float(ref)) / max(abs(float(ref)), 0.1 if key in MODULE_KEYS else 1e-3 * weight)
    _note('v ' + key, err, what)
    print(f"{what}: value err {err:.2e}")
    assert err <= VTOL[key], (what, float(got), float(ref), err)


def check_grad(got, ref, key, what, tol=None, excl=None):
    """max|got - ref| / max|ref| over every pixel that the l1 exclusion rule does not leave out"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert np.abs(ref).max() > 0.0, f"{what}: all-zero reference gradient"
    d = np.abs(got - ref)
    if excl is not None:
        d = np.where(excl, 0.0, d)
    err = d.max() / np.abs(ref).max()
    _note('g ' + key, err, what)
    print(f"{what}: gradient err {err:.2e}" + (f", left out {int(excl.sum())}" if excl is not None else ""))
    assert err <= (GTOL[key] if tol is None else tol), (what, err)


def run(fn, *xs):
    """value (0-dim tensor) and gradient w.r.t. the last argument; the value-only call returns the same bits"""
    f = xs[-1].clone().requires_grad_(True)
    loss = fn(*xs[:-1], f)
    loss.backward()
    with torch.no_grad():
        assert torch.equal(fn(*xs).detach(), loss.detach()), "value-only call differs from the call that writes the gradient"
    assert f.grad.shape == f.shape and f.grad.dtype == f.dtype
    return loss.detach(), f.grad


def ids(cases):
    return [LC.case_id(c) for c in cases]


# ------------------------------------------------------------------ SSIMLoss('ssim')
@pytest.mark.parametrize("case", LC.ssim_cases(), ids=ids(LC.ssim_cases()))
def test_ssim_vs_oracle(case):
    from core.loss import SSIMLoss
    trip = LC.build(case)
    want_l, want_g = O.ssim_loss(*LC.f64(*trip), 0.7)
    l, g = run(SSIMLoss('ssim', weight=0.7), *dev(*trip))
    what = "ssim " + LC.case_id(case)
    check_value(l, want_l, 'ssim', 0.7, what)
    check_grad(g.cpu().numpy(), want_g, 'ssim', what)


@pytest.mark.parametrize("shape,n", [((11, 11), 3), ((12, 13), 1), ((33, 47), 2), ((42, 43), 3), ((97, 130), 1), ((256, 256), 2)])
def test_ssim_data_range_255_vs_oracle(shape, n):
    from core.loss import SSIMLoss
    trip = LC.triple('r255', *shape, n)
    want_l, want_g = O.ssim_loss(*LC.f64(*trip), 0.7, 255.0)
    l, g = run(SSIMLoss('ssim', data_range=255, weight=0.7), *dev(*trip))
    what = f"ssim255 {n}x{shape[0]}x{shape[1]}"
    check_value(l, want_l, 'ssim255', 0.7, what)
    check_grad(g.cpu().numpy(), want_g, 'ssim255', what)


def test_ssim_constant_fused_image():
    """F2 case c's rule at another shape and B = 2"""
    from core.loss import SSIMLoss
    a, b, _ = LC.triple('rand', 26, 27, 2)
    f = np.full_like(a, 0.375)
    want_l, want_g = O.ssim_loss(*LC.f64(a, b, f), 1.0)
    l, g = run(SSIMLoss('ssim'), *dev(a, b, f))
    check_value(l, want_l, 'ssim', 1.0, "ssim flat fused")
    check_grad(g.cpu().numpy(), want_g, 'ssim_flat', "ssim flat fused", tol=GTOL_FLAT_FUSED)


# ------------------------------------------------------------------ PixelLoss / GradLoss, 2 x 2 each
@pytest.mark.parametrize("case", LC.pixgrad_cases(), ids=ids(LC.pixgrad_cases()))
def test_pixel_and_grad_all_modes_vs_oracle(case):
    """PixelLoss and GradLoss in {l1, l2} x {max, avg}.  l1 gradients: nothing left out on 'dyadic'; on the float distributions the
    Sobel term leaves out what loss_cases.sobel_l1_excluded names (capped; the pixel term leaves nothing out: the sign of an fp32
    difference of two fp32 numbers is exact)."""
    from core.loss import GradLoss, PixelLoss
    trip = LC.build(case)
    t64, td = LC.f64(*trip), dev(*trip)
    for norm in ('l1', 'l2'):
        for mode in ('max', 'avg'):
            what = f"{norm} {mode} {LC.case_id(case)}"
            want_l, want_g = O.pixel_loss(*t64, 0.3, mode, True, norm)
            l, g = run(lambda a, b, f: PixelLoss(norm, weight=0.3)(a, b, f, mode=mode), *td)
            check_value(l, want_l, 'pixel', 0.3, "pixel " + what)
            if np.abs(want_g).max() > 0.0:
                check_grad(g.cpu().numpy(), want_g, 'pixel_' + norm, "pixel " + what, tol=GTOL_L1 if norm == 'l1' else None)
            else:       # (avg l1 on a few pixels: every sgn pair cancels)
                assert not g.any().item(), what
            want_l, want_g = O.grad_loss(*t64, 0.7, mode, True, norm)
            l, g = run(lambda a, b, f: GradLoss(norm, weight=0.7)(a, b, f, mode=mode), *td)
            check_value(l, want_l, 'grad', 0.7, "grad " + what)
            excl = None
            if norm == 'l1':
                excl = LC.sobel_l1_excluded(*trip, mode)
                LC.check_cap(excl, what)
                assert case[0] != 'dyadic' or not excl.any()
            if np.abs(want_g).max() > 0.0:
                check_grad(g.cpu().numpy(), want_g, 'grad_' + norm, "grad " + what, tol=GTOL_L1 if norm == 'l1' else None, excl=excl)
            else:
                assert not g.any().item(), what


# ------------------------------------------------------------------ TVLoss
@pytest.mark.parametrize("case", LC.tv_cases(), ids=ids(LC.tv_cases()))
def test_tv_vs_oracle(case):
    from core.loss import TVLoss
    x = LC.build(case)[2]
    for norm in ('l1', 'l2'):
        want_l, want_g = O.tv_loss(x.astype(np.float64), norm, 0.3)
        l, g = run(TVLoss(norm, weight=0.3), *dev(x))
        what = f"tv {norm} {LC.case_id(case)}"
        check_value(l, want_l, 'tv', 0.3, what)
        check_grad(g.cpu().numpy(), want_g, 'tv_' + norm, what, tol=GTOL_L1 if norm == 'l1' else None)


def test_tv_folds_leading_dimensions():
    from core.loss import TVLoss
    x = LC.triple('rand', 13, 21, 6)[2].reshape(2, 3, 13, 21)
    for norm in ('l1', 'l2'):
        want_l, want_g = O.tv_loss(x.astype(np.float64), norm, 0.3)
        l, g = run(TVLoss(norm, weight=0.3), *dev(x))
        check_value(l, want_l, 'tv', 0.3, "tv [2,3,h,w] " + norm)
        check_grad(g.cpu().numpy(), want_g, 'tv_' + norm, "tv [2,3,h,w] " + norm, tol=GTOL_L1 if norm == 'l1' else None)


# ------------------------------------------------------------------ SSIMLoss 'w-ssim' / 'msw-ssim' / 'ms-ssim'
def _mode_params():
    for mode in ('w-ssim', 'msw-ssim', 'ms-ssim'):
        for case in LC.mode_cases(mode):
            yield pytest.param(mode, case, id=f"{mode}-{LC.case_id(case)}")


@pytest.mark.parametrize("mode,case", list(_mode_params()))
def test_ssim_modes_vs_oracle(mode, case):
    from core.loss import SSIMLoss
    trip = LC.build(case)
    want_l, want_g = O.ssim_mode_loss(*LC.f64(*trip), mode, 0.7)
    l, g = run(SSIMLoss(mode, weight=0.7), *dev(*trip))
    what = f"{mode} {LC.case_id(case)}"
    check_value(l, want_l, mode, 0.7, what)
    check_grad(g.cpu().numpy(), want_g, mode, what)


@pytest.mark.parametrize("mode", ['w-ssim', 'msw-ssim'])
@pytest.mark.parametrize("shape,n", [((11, 11), 2), ((33, 47), 3), ((64, 80), 1)])
def test_ssim_modes_data_range_255_vs_oracle(mode, shape, n):
    from core.loss import SSIMLoss
    trip = LC.triple('r255', *shape, n)
    want_l, want_g = O.ssim_mode_loss(*LC.f64(*trip), mode, 0.7, 255.0)
    l, g = run(SSIMLoss(mode, data_range=255, weight=0.7), *dev(*trip))
    what = f"{mode}255 {n}x{shape[0]}x{shape[1]}"
    check_value(l, want_l, mode + '255', 0.7, what)
    check_grad(g.cpu().numpy(), want_g, mode + '255', what)


def test_ms_ssim_below_its_threshold_raises():
    from core.loss import SSIMLoss
    z = dev(*LC.triple('rand', 160, 200, 1))
    with pytest.raises(Exception, match="161x161"):
        SSIMLoss('ms-ssim')(*z)


def test_ms_ssim_every_level_clamped_gives_exactly_zero_gradient():
    """'anti2': the level means of both sources are negative on all five levels, so ms_weights_kernel's clamped arm zeroes every
    weight (the oracle's gradient is exactly zero too: tests/test_loss_oracle_cpu.py)"""
    from core.loss import SSIMLoss
    for shape, n in (((161, 161), 2), ((176, 177), 1)):
        trip = LC.triple('anti2', *shape, n)
        want_l, want_g = O.ssim_mode_loss(*LC.f64(*trip), 'ms-ssim', 0.7)
        assert not want_g.any()
        l, g = run(SSIMLoss('ms-ssim', weight=0.7), *dev(*trip))
        check_value(l, want_l, 'ms-ssim', 0.7, f"ms-ssim anti2 {shape}")
        assert not g.any().item(), shape


# ------------------------------------------------------------------ SSIM / MS_SSIM / MSW_SSIM modules
@pytest.mark.parametrize("win", LC.WIN_SIZES)
def test_ssim_module_terms_vs_oracle(win):
    from core.loss import SSIM
    for (h, w), n, dist in (((11, 11), 2, 'rand'), ((12, 13), 3, 'cf'), ((33, 47), 3, 'wide'), ((64, 80), 1, 'flatsrc')):
        a, _, f = LC.triple(dist, h, w, n)
        out = SSIM(win)(*dev(a, f))
        t = O.ssim_full_terms(*LC.f64(a, f), O.create_window(win))
        for key, ref in (("ssim", t["S"]), ("cs", t["cs"]), ("sigma", t["sigma"])):
            want = ref.mean(axis=(1, 2, 3))
            got = out[key].detach().cpu().numpy()
            assert got.shape == (n,)
            for s in range(n):
                check_value(got[s], want[s], 'terms', 1.0, f"SSIM({win}) {key} {dist} {n}x{h}x{w} sample {s}")


def test_ms_ssim_and_msw_ssim_modules_vs_oracle():
    from core.loss import MS_SSIM, MSW_SSIM
    a, b, f = LC.triple('cf', 161, 176, 2)
    ms = MS_SSIM()(*dev(a, f)).cpu().numpy()
    for i in range(2):       # loss(a, a, f) = 1 - ms(a, f) for one sample
        l, _ = O.ssim_mode_loss(*LC.f64(a[i:i + 1], a[i:i + 1], f[i:i + 1]), "ms-ssim", need_grad=False)
        check_value(ms[i], 1.0 - l, 'MS_SSIM', 1.0, f"MS_SSIM sample {i}")
    a, b, f = LC.triple('rand', 33, 47, 3)
    want_l, want_g = O.ssim_mode_loss(*LC.f64(a, b, f), "msw-ssim", 1.0)
    v, g = run(MSW_SSIM(), *dev(a, b, f))
    check_value(v, 1.0 - want_l, 'MSW_SSIM', 1.0, "MSW_SSIM")
    check_grad(g.cpu().numpy(), -want_g, 'MSW_SSIM', "MSW_SSIM")


# ------------------------------------------------------------------ the fused call
_FUSED_REF = {}     # (case, configuration) -> the oracle's result: each big reference is built once per module


def _fused_ref(case, trip, pm, pn, gm, gn):
    key = (case, pm, pn, gm, gn)
    if key not in _FUSED_REF:
        _FUSED_REF[key] = O.fusion_losses(*LC.f64(*trip), 1.0, 0.01, 0.1, True, pm, gm, pn, gn)
    return _FUSED_REF[key]


def _check_fused(case, pn, pm, gn, gm):
    from core.loss import FusionLoss, GradLoss, PixelLoss, SSIMLoss
    trip = LC.build(case)
    td = dev(*trip)
    what = f"fused {pn}/{pm}/{gn}/{gm} {LC.case_id(case)}"
    l1, l2, l3 = SSIMLoss('ssim', weight=1.0), PixelLoss(pn, weight=0.01), GradLoss(gn, weight=0.1)
    fl = FusionLoss(l1, l2, l3, pm, gm)
    tot, g = run(fl, *td)
    v = fl.values.cpu().numpy()
    # against the oracle
    (w1, w2, w3, wtot), want_g = _fused_ref(case, trip, pm, pn, gm, gn)
    check_value(v[1], w1, 'ssim', 1.0, what + " ssim")
    check_value(v[2], w2, 'pixel', 0.01, what + " pixel")
    check_value(v[3], w3, 'grad', 0.1, what + " grad")
    check_value(tot, wtot, 'fused', 1.0, what + " total")
    excl = None
    if gn == 'l1':
        excl = LC.sobel_l1_excluded(*trip, gm)
        LC.check_cap(excl, what)
    check_grad(g.cpu().numpy(), want_g, 'fused', what, excl=excl)
    # the identities of test_gpu_loss.test_fusion_loss_equals_the_three_modules, at this shape and configuration
    f = td[2].clone().requires_grad_(True)
    a, b, c = l1(td[0], td[1], f), l2(td[0], td[1], f, mode=pm), l3(td[0], td[1], f, mode=gm)
    (a + b + c).backward()
    assert v[1] == a.item() and abs(v[2] - b.item()) <= 1e-6 * abs(b.item()) and v[3] == c.item(), (what, v, a.item(), b.item(), c.item())
    assert tot.item() == v[0] and abs(v[0] - (a + b + c).item()) <= 1.2e-7 * abs(v[0])
    e = float((g - f.grad).abs().max() / f.grad.abs().max())
    assert e <= 2e-6, (what, e)


_COMBOS = [(pn, pm, gn, gm) for pn in ('l1', 'l2') for pm in ('max', 'avg') for gn in ('l1', 'l2') for gm in ('max', 'avg')]


@pytest.mark.parametrize("shape", LC.RAGGED, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pn,pm,gn,gm", _COMBOS, ids=["-".join(c) for c in _COMBOS])
def test_fused_all_16_configurations(shape, pn, pm, gn, gm):
    """bit 0 / bit 1 of px_mode and the l2 / avg arms of the Sobel term inside mmif_fusion_loss"""
    _check_fused(('rand', *shape, 2, 0), pn, pm, gn, gm)


@pytest.mark.parametrize("case", LC.fused_train_cases(), ids=ids(LC.fused_train_cases()))
def test_fused_train_configuration(case):
    _, h, w, n, _ = case
    tiles = -(-h // 16) * -(-w // 16) * n
    if case[1:4] in ((256, 256, 64), (*LC.BIG, 3)):
        # one float per 16 x 16 Sobel tile per image: longer than FF_CAP, so fusion_finish_kernel reads the partials directly
        assert tiles > FF_CAP, tiles
    else:
        assert tiles <= FF_CAP
    _check_fused(case, 'l1', 'max', 'l1', 'max')


# ------------------------------------------------------------------ batch consistency
def _entries():
    from core.loss import FusionLoss, GradLoss, PixelLoss, SSIMLoss, TVLoss
    pix = lambda n, m: (lambda a, b, f: PixelLoss(n, weight=0.3)(a, b, f, mode=m))
    grd = lambda n, m: (lambda a, b, f: GradLoss(n, weight=0.7)(a, b, f, mode=m))
    return {
        'ssim': (SSIMLoss('ssim', weight=0.7), 'ssim', 0.7), 'pixel l1 max': (pix('l1', 'max'), 'pixel', 0.3),
        'pixel l2 avg': (pix('l2', 'avg'), 'pixel', 0.3), 'grad l1 avg': (grd('l1', 'avg'), 'grad', 0.7),
        'grad l2 max': (grd('l2', 'max'), 'grad', 0.7), 'w-ssim': (SSIMLoss('w-ssim', weight=0.7), 'w-ssim', 0.7),
        'msw-ssim': (SSIMLoss('msw-ssim', weight=0.7), 'msw-ssim', 0.7), 'ms-ssim': (SSIMLoss('ms-ssim', weight=0.7), 'ms-ssim', 0.7),
        'tv l2': ((lambda a, b, f: TVLoss('l2', weight=0.3)(f)), 'tv', 0.3),
        'fused': (FusionLoss(SSIMLoss('ssim'), PixelLoss('l1', weight=0.01), GradLoss('l1', weight=0.1), 'max', 'max'), 'fused', 1.0),
    }


@pytest.mark.parametrize("name", ['ssim', 'pixel l1 max', 'pixel l2 avg', 'grad l1 avg', 'grad l2 max', 'w-ssim', 'msw-ssim', 'ms-ssim', 'tv l2', 'fused'])
def test_batch_of_16_is_the_mean_of_16_single_calls(name):
    """every loss is a mean of per-sample values and the scale weight / count is applied once per pixel: sample i's slice of the B = 16
    gradient is 1/16 of the B = 1 gradient on that sample to two fp32 roundings, the value is the mean of the 16 single values to fp32
    summation order"""
    fn, key, weight = _entries()[name]
    h, w = (161, 163) if name == 'ms-ssim' else (40, 56)
    a, b, f = dev(*LC.mixed_batch(h, w, 16))
    l16, g16 = run(fn, a, b, f)
    vals = []
    for i in range(16):
        l1, g1 = run(fn, a[i:i + 1], b[i:i + 1], f[i:i + 1])
        vals.append(float(l1))
        want = g1.double() / 16.0
        d = (g16[i:i + 1].double() - want).abs()
        assert bool((d <= 2.0 ** -23 * want.abs() + 1e-37).all()), (name, i, float(d.max()), float(want.abs().max()))
    check_value(l16, float(np.mean(vals)), key, weight, f"B=16 {name}")


# ------------------------------------------------------------------ input forms
@pytest.mark.parametrize("name", ['ssim', 'pixel l2 avg', 'grad l1 avg', 'w-ssim', 'tv l2', 'fused'])
@pytest.mark.parametrize("form", ['window', 'fp64', 'bf16'])
def test_input_forms_bitwise(name, form):
    """a non-contiguous column window, an fp64 and a bf16 tensor give bitwise the value and gradient of their contiguous fp32 copy,
    and imgf.grad has imgf's shape and dtype (the gradient of a bf16 image is the fp32 gradient rounded to bf16 by autograd)"""
    fn, _, _ = _entries()[name]
    a, b, f = (torch.from_numpy(x) for x in LC.triple('rand', 40, 56, 2))
    if form == 'window':
        xs = [torch.cat([torch.zeros(2, 1, 40, 7), x, torch.ones(2, 1, 40, 5)], 3).cuda()[..., 7:63] for x in (a, b, f)]
        assert not xs[2].is_contiguous()
    elif form == 'fp64':
        xs = [(x.double() / 3.0).cuda() for x in (a, b, f)]
    else:
        xs = [x.bfloat16().cuda() for x in (a, b, f)]
    base = [x.float().contiguous() for x in xs]
    f1 = xs[2].clone().requires_grad_(True) if form != 'window' else xs[2].detach().requires_grad_(True)
    f0 = base[2].clone().requires_grad_(True)
    l1, l0 = fn(xs[0], xs[1], f1), fn(base[0], base[1], f0)
    l1.backward()
    l0.backward()
    assert torch.equal(l1.detach(), l0.detach()), (name, form)
    assert f1.grad.shape == f1.shape and f1.grad.dtype == f1.dtype
    assert torch.equal(f1.grad, f0.grad.to(f1.dtype)), (name, form)
    assert float(f0.grad.abs().max()) > 0.0


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("shape,n", [((3, 3), 1), ((33, 47), 3), ((97, 130), 2)])
def test_exact_zeros(shape, n):
    from core.loss import FusionLoss, GradLoss, PixelLoss, SSIMLoss
    a, b, _ = LC.triple('rand', *shape, n)
    da, db = dev(a, b)
    (dmax,) = dev(np.maximum(a, b))
    (dconst,) = dev(np.full_like(a, 0.375))
    for norm in ('l1', 'l2'):
        # imgf = max(img1, img2): the pixel-max term and its gradient are exactly 0
        l, g = run(lambda x, y, f: PixelLoss(norm, weight=0.3)(x, y, f, mode='max'), da, db, dmax)
        assert l.item() == 0.0 and not g.any().item(), norm
        for mode in ('max', 'avg'):
            # img1 = img2 = imgf: pixel and Sobel terms exactly 0 (avg: both differences; max: max(x, x) = x)
            l, g = run(lambda x, y, f: PixelLoss(norm, weight=0.3)(x, y, f, mode=mode), da, da, da)
            assert l.item() == 0.0 and not g.any().item(), (norm, mode)
            l, g = run(lambda x, y, f: GradLoss(norm, weight=0.7)(x, y, f, mode=mode), da, da, da)
            assert l.item() == 0.0 and not g.any().item(), (norm, mode)
            # a constant fused image: gx = gy = 0 on every pixel, sgn(0) = 0 -> the Sobel gradient is exactly zero (F2 case c's rule)
            l, g = run(lambda x, y, f: GradLoss(norm, weight=0.7)(x, y, f, mode=mode), da, db, dconst)
            assert l.item() > 0.0 and not g.any().item(), (norm, mode)
            if shape[0] >= 11:   # ... and through the fused call, with the other two terms weighted 0
                fl = FusionLoss(SSIMLoss('ssim', weight=0.0), PixelLoss(norm, weight=0.0), GradLoss(norm, weight=0.7), mode, mode)
                l, g = run(fl, da, db, dconst)
                assert l.item() > 0.0 and not g.any().item(), (norm, mode)
    if shape[0] >= 11:
        l, g = run(SSIMLoss('ssim'), da, da, da)
        assert abs(l.item()) <= SSIM_SELF_BOUND, l.item()
