"""The reflect-padded SSIM losses (SSIMLoss(mode, use_padding=True), SSIM / MS_SSIM / MSW_SSIM with use_padding=True) on the padded
kernels of csrc/loss_modes.hip -- reflected reads in the statistics pass, the fold of the border taps in the gradient pass -- against
the fp64 definition of tests/ssim_pad_cases.py (pinned to torch float64 autograd and to golden F16 by
tests/test_ssim_pad_oracle_cpu.py, which also shows that a missing fold or a 'symmetric' / 'replicate' / zero padding is at least
0.1 max|grad| away on every case here).  Through the C ABI: a workspace of exactly the queried size with a guard behind it, grad_out
NULL, and a second call, all with the same bits.  Through core/loss.py: no core/_stock.py function is reached on CUDA tensors,
use_padding=False keeps its bits, CPU tensors keep the stock composition.

Tolerances: value |got - ref| / max(|ref|, floor) with floor = 1e-3 x weight (losses) or 0.1 (module means); gradient
max|got - ref| / max|ref|.  Each bar = largest error measured on an MI355X over this file (printed as SSIM_PAD_SWEEP_MARGINS, run with
-s) times at most 4, never looser than the bars of tests/test_gpu_loss.py: 1e-4 (values), 3e-4 ('ssim' gradient), 5e-4 (the others).
Measured on an MI355X, values: ssim 1.32e-6 (anti 3x12x11), w-ssim 5.8e-7 (anti 3x32x33), ms-ssim 2.54e-6 (flatsrc 3x81x96), msw-ssim
6.4e-7 (anti 1x64x80), term means 2.85e-5 (SSIM(3) 'cs', rand 1x16x17; bar stays 1e-4), modules: SSIM 6.2e-7, MS_SSIM 1.98e-6, MSW_SSIM
2.57e-6.  Measured, gradients: ssim 1.17e-5 (anti 3x12x11), w-ssim 8.8e-6 (anti 3x32x33), msw-ssim 3.22e-5 (cf 1x11x11), modules: SSIM
4.2e-7, MS_SSIM 1.2e-5, MSW_SSIM 1.12e-5; ms-ssim 1.52e-4 on 'same' 3x97x83 and at most 9.9e-6 on the other eight cases (bar stays 5e-4):
the level-0 cs mean of that case's first sample is 9.1e-5, a mean of O(0.1) values whose fp32 rounding error of about 1e-8 is 1e-4 of it,
and the gradient of that level carries the factor ms / v of the reference's own formula.

Run time on one MI355X: 8 s for the 79 cases.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_cases as LC
import ssim_pad_cases as PC

pytestmark = pytest.mark.gpu

VTOL = {'ssim': 5e-6, 'w-ssim': 2.2e-6, 'ms-ssim': 1e-5, 'msw-ssim': 2.5e-6, 'terms': 1e-4, 'SSIM': 2.4e-6, 'MS_SSIM': 7.5e-6, 'MSW_SSIM': 1e-5}
GTOL = {'ssim': 4.5e-5, 'w-ssim': 3.5e-5, 'ms-ssim': 5e-4, 'msw-ssim': 1.25e-4, 'SSIM': 1.6e-6, 'MS_SSIM': 4.8e-5, 'MSW_SSIM': 4.4e-5}
MODULE_KEYS = ('terms', 'SSIM', 'MS_SSIM', 'MSW_SSIM')
GUARD = 1024            # floats behind the workspace that must keep their bits

_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    print("\nSSIM_PAD_SWEEP_MARGINS (largest error per entry point): " + "; ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in sorted(_WORST.items())))


def _note(key, err, what):
    _WORST[key] = max(_WORST.get(key, (0.0, '')), (float(err), what))


def dev(*xs):
    return [torch.from_numpy(np.array(x)).cuda() for x in xs]      # (a copy: the shared inputs are read-only)


def check_value(got, ref, key, weight, what):
    err = abs(float(got) - float(ref)) / max(abs(float(ref)), 0.1 if key in MODULE_KEYS else 1e-3 * weight)
    _note('v ' + key, err, what)
    print(f"{what}: value err {err:.2e}")
    assert err <= VTOL[key], (what, float(got), float(ref), err)


def check_grad(got, ref, key, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert np.abs(ref).max() > 0.0, f"{what}: all-zero reference gradient"
    err = np.abs(got - ref).max() / np.abs(ref).max()
    _note('g ' + key, err, what)
    print(f"{what}: gradient err {err:.2e}")
    assert err <= GTOL[key], (what, err)


def term_err(key, got, ref):
    """'ssim' / 'cs' are means of values in [-1, 1] (absolute fp32 error: floor 0.1); 'sigma' is at least its 1e-4 clamp: relative"""
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 0.1 if key != 'sigma' else 1e-4)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(nbytes):
    """a workspace of exactly nbytes (a multiple of 4) followed by GUARD floats of a known pattern"""
    assert nbytes % 4 == 0
    buf = torch.full((nbytes // 4 + GUARD,), -7.25, dtype=torch.float32, device='cuda')
    return buf, buf[nbytes // 4:]


def call_pad(mode, a, b, f, weight, dr, want_grad=True):
    """mmif_ssim_loss_pad on device tensors [n,1,h,w] -> (value tensor [1], gradient or None)"""
    from mmif._lib import check, lib
    n, _, h, w = f.shape
    k = PC.MODES.index(mode)
    nbytes = lib.mmif_ssim_loss_pad_workspace(n, h, w, k)
    ws, guard = _guarded(nbytes)
    out = torch.empty(1, dtype=torch.float32, device='cuda')
    grad = torch.full_like(f, float('nan')) if want_grad else None
    check(lib.mmif_ssim_loss_pad(_ptr(a), _ptr(b), _ptr(f), n, h, w, weight, dr, k, _ptr(out), _ptr(grad), _ptr(ws), nbytes, None), "ssim_loss_pad")
    torch.cuda.synchronize()
    assert bool((guard == -7.25).all()), f"{mode}: wrote behind a workspace of the queried size"
    return out, grad


# ------------------------------------------------------------------ the C ABI
def test_library_exports_the_padded_entry_points():
    from mmif._lib import SIGNATURES, lib
    for name in ("mmif_ssim_loss_pad_workspace", "mmif_ssim_loss_pad", "mmif_ssim_terms_pad"):
        assert hasattr(lib, name) and name in SIGNATURES, name


@pytest.mark.parametrize("mode,case", PC.all_loss_cases(), ids=[f"{m}-{PC.case_id(c)}" for m, c in PC.all_loss_cases()])
def test_loss_pad_vs_definition(mode, case):
    want_l, want_g = PC.reference(mode, case)
    a, b, f = dev(*PC.build(case))
    dr = PC.data_range(case)
    l, g = call_pad(mode, a, b, f, PC.WEIGHT, dr)
    what = f"pad {mode} {PC.case_id(case)}"
    check_value(l.item(), want_l, mode, PC.WEIGHT, what)
    check_grad(g.cpu().numpy(), want_g, mode, what)
    l0, _ = call_pad(mode, a, b, f, PC.WEIGHT, dr, want_grad=False)
    assert torch.equal(l0, l), f"{what}: grad_out NULL changes the value"
    l2, g2 = call_pad(mode, a, b, f, PC.WEIGHT, dr)
    assert torch.equal(l2, l) and torch.equal(g2, g), f"{what}: a second call gives other bits"


@pytest.mark.parametrize("case", PC.module_cases(), ids=[f"win{c[0]}-{PC.case_id(c[1:])}" for c in PC.module_cases()])
def test_terms_pad_vs_definition(case):
    from mmif._lib import check, lib
    win, case = case[0], case[1:]
    dr = PC.data_range(case)
    a, _, f = PC.build(case)
    n, _, h, w = a.shape
    want = PC.pad_terms(*LC.f64(a, f), win, dr)
    da, df = dev(a, f)
    nbytes = lib.mmif_ssim_loss_pad_workspace(n, h, w, 1)
    outs = []
    for _ in range(2):
        ws, guard = _guarded(nbytes)
        out = torch.empty((3, n), dtype=torch.float32, device='cuda')
        check(lib.mmif_ssim_terms_pad(_ptr(da), _ptr(df), n, h, w, win, dr, _ptr(out), _ptr(ws), nbytes, None), "ssim_terms_pad")
        torch.cuda.synchronize()
        assert bool((guard == -7.25).all())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu().numpy()
    for i, key in enumerate(('ssim', 'cs', 'sigma')):
        for s in range(n):
            ref = want[key][s]
            err = term_err(key, got[i, s], ref)
            _note('v terms', err, f"win {win} {key} {PC.case_id(case)}")
            assert err <= VTOL['terms'], (win, key, PC.case_id(case), s, got[i, s], ref, err)


# ------------------------------------------------------------------ core/loss.py
@pytest.fixture
def no_stock(monkeypatch):
    """every composition of core/_stock.py that the padded options used to run raises"""
    from core import _stock

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"core._stock.{name} reached for a CUDA input inside the kernels' limits")
        return f
    for name in ("ssim_loss", "ssim_terms", "msssim", "mswssim"):
        monkeypatch.setattr(_stock, name, refuse(name))


def run(fn, *xs):
    f = xs[-1].clone().requires_grad_(True)
    out = fn(*xs[:-1], f)
    out.sum().backward()
    return out.detach(), f.grad


@pytest.mark.parametrize("mode,case", [('ssim', ('rand', 33, 47, 2, 0)), ('w-ssim', ('flatsrc', 16, 17, 3, 0)), ('msw-ssim', ('r255', 11, 11, 2, 0)),
                                       ('ms-ssim', ('cf', 81, 96, 2, 0)), ('ssim', ('mixed', 33, 47, 5, 0))])
def test_ssim_loss_module_runs_the_padded_kernels(no_stock, mode, case):
    from core.loss import SSIMLoss
    want_l, want_g = PC.reference(mode, case)
    a, b, f = dev(*PC.build(case))
    dr = PC.data_range(case)
    l, g = run(SSIMLoss(mode, data_range=dr, use_padding=True, weight=PC.WEIGHT), a, b, f)
    what = f"SSIMLoss pad {mode} {PC.case_id(case)}"
    check_value(l, want_l, mode, PC.WEIGHT, what)
    check_grad(g.cpu().numpy(), want_g, mode, what)
    l_abi, g_abi = call_pad(mode, a, b, f, PC.WEIGHT, dr)
    assert l.item() == l_abi.item() and torch.equal(g, g_abi), "the module and the C ABI call differ"
    with torch.no_grad():
        assert torch.equal(SSIMLoss(mode, data_range=dr, use_padding=True, weight=PC.WEIGHT)(a, b, f), l)


@pytest.mark.parametrize("win,case", [(11, ('rand', 16, 17, 3, 0)), (11, ('wide', 11, 12, 2, 0)), (7, ('cf', 33, 47, 2, 0)), (3, ('r255', 3, 4, 1, 0))])
def test_ssim_module_padded(no_stock, win, case):
    from core.loss import SSIM
    a, _, f = PC.build(case)
    dr = PC.data_range(case)
    n = a.shape[0]
    want = PC.pad_terms(*LC.f64(a, f), win, dr)
    da, df = dev(a, f)
    mod = SSIM(win, dr, True, True)
    out = mod(da, df)
    for key in ('ssim', 'cs', 'sigma'):
        assert tuple(out[key].shape) == (n,)
        for s in range(n):
            ref = want[key][s]
            err = term_err(key, out[key][s].item(), ref)
            _note('v terms', err, f"SSIM({win}) pad {key}")
            assert err <= VTOL['terms'], (win, key, s, err)
    if win == 11:       # differentiable w.r.t. the second argument, per sample: loss(a_i, a_i, f_i) = 1 - ssim_i
        fg = df.clone().requires_grad_(True)
        res = mod(da, fg)['ssim']
        res.sum().backward()
        for s in range(n):
            l, g = PC.pad_loss(*LC.f64(a[s:s + 1], a[s:s + 1], f[s:s + 1]), 'ssim', 1.0, dr)
            check_value(res[s].item(), 1.0 - l, 'SSIM', 1.0, f"SSIM(11) pad sample {s}")
            check_grad(fg.grad[s:s + 1].cpu().numpy(), -g, 'SSIM', f"SSIM(11) pad sample {s}")


def test_ms_ssim_and_msw_ssim_modules_padded(no_stock):
    from core.loss import MS_SSIM, MSW_SSIM
    a, b, f = PC.build(('cf', 97, 83, 2, 0))
    v, g = run(MS_SSIM(11, 1.0, True, True), *dev(a, f))
    assert tuple(v.shape) == (2,)
    for s in range(2):
        l, gs = PC.pad_loss(*LC.f64(a[s:s + 1], a[s:s + 1], f[s:s + 1]), 'ms-ssim', 1.0)
        check_value(v[s].item(), 1.0 - l, 'MS_SSIM', 1.0, f"MS_SSIM pad sample {s}")
        check_grad(g[s:s + 1].cpu().numpy(), -gs, 'MS_SSIM', f"MS_SSIM pad sample {s}")
    a, b, f = PC.build(('rand', 33, 47, 3, 0))
    want_l, want_g = PC.pad_loss(*LC.f64(a, b, f), 'msw-ssim', 1.0)
    v, g = run(MSW_SSIM((11, 9, 7, 5, 3), 1.0, True, False), *dev(a, b, f))
    check_value(v, 1.0 - want_l, 'MSW_SSIM', 1.0, "MSW_SSIM pad")
    check_grad(g.cpu().numpy(), -want_g, 'MSW_SSIM', "MSW_SSIM pad")


def test_unpadded_options_keep_their_bits():
    """use_padding=False is the entry point it was: the same bits as _LossFn / _SsimLossFn(_UNPADDED) called directly"""
    from core import loss as L
    a, b, f = dev(*LC.triple('rand', 40, 56, 2))
    big = dev(*LC.triple('cf', 161, 163, 1))
    for mode, xs in (('ssim', (a, b, f)), ('w-ssim', (a, b, f)), ('msw-ssim', (a, b, f)), ('ms-ssim', big)):
        l, g = run(L.SSIMLoss(mode, use_padding=False, weight=0.7), *xs)
        if mode == 'ssim':
            l0, g0 = run(lambda x, y, z: L._LossFn.apply(z, x, y, 0, 0.7, 1.0, 0), *xs)
        else:
            l0, g0 = run(lambda x, y, z: L._SsimLossFn.apply(z, x, y, L._UNPADDED, L._SSIM_MODES[mode], 0.7, 1.0), *xs)
        assert torch.equal(l, l0) and torch.equal(g, g0), mode
    v, g = run(L.MSW_SSIM(), a, b, f)
    v0, g0 = run(lambda x, y, z: 1.0 - L._SsimLossFn.apply(z, x, y, L._UNPADDED, 3, 1.0, 1.0), a, b, f)
    assert torch.equal(v, v0) and torch.equal(g, g0)


def test_cpu_tensors_and_small_images_keep_the_stock_composition(monkeypatch):
    from core import _stock
    from core.loss import MS_SSIM, SSIM, SSIMLoss
    seen = []
    for name in ("ssim_loss", "ssim_terms", "msssim"):
        orig = getattr(_stock, name)
        monkeypatch.setattr(_stock, name, (lambda o, nm: (lambda *x, **k: (seen.append(nm), o(*x, **k))[1]))(orig, name))
    a, b, f = (torch.from_numpy(x) for x in PC.build(('rand', 33, 47, 2, 0)))
    l = SSIMLoss('w-ssim', use_padding=True, weight=0.7)(a, b, f)
    assert seen[0] == "ssim_loss" and abs(l.item() - PC.reference('w-ssim', ('rand', 33, 47, 2, 0))[0]) <= 1e-5
    del seen[:]
    SSIM(7, 1.0, True, True)(a, f)
    assert seen == ["ssim_terms"]
    del seen[:]
    # below the limits on the device: 10 x 10 for the losses, 80 x 80 for the pyramid
    SSIMLoss('ssim', use_padding=True)(a[..., :10, :10].cuda(), b[..., :10, :10].cuda(), f[..., :10, :10].cuda())
    assert seen[0] == "ssim_loss"
    del seen[:]
    x = torch.from_numpy(LC.triple('rand', 80, 80, 1)[0]).cuda()
    with pytest.raises(RuntimeError):       # F.pad refuses to pad the 5 x 5 level by 5, as in the reference
        MS_SSIM(11, 1.0, True, True)(x, x)
    assert seen[0] == "msssim"
    # per-pixel maps stay stock as well
    del seen[:]
    SSIM(11, 1.0, True, False)(a.cuda(), f.cuda())
    assert seen == ["ssim_terms"]


def test_fusion_loss_refuses_a_padded_ssim_loss():
    from core.loss import FusionLoss, GradLoss, PixelLoss, SSIMLoss
    with pytest.raises(ValueError, match="padding"):
        FusionLoss(SSIMLoss('ssim', use_padding=True), PixelLoss('l1'), GradLoss('l1'))
    FusionLoss(SSIMLoss('ssim'), PixelLoss('l1'), GradLoss('l1'))
