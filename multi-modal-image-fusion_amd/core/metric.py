# -*- coding: utf-8 -*-
"""Evaluation metrics -- API mirror of the reference's core/metric.py (the 17 names of its __all__) plus `fusion_metrics`, the
per-sample table of eval.py:29-76.

`calc_ssim` in the configuration test.py:49-52 prints per fused image (11x11 window, valid correlation, scalar mean, images of at
least 11 px) shares its maths with SSIMLoss and runs on the same fused HIP kernel (csrc/loss_modes.hip: separable window through LDS,
block sums, fixed-order second stage).  Every other calc_ssim call on CUDA tensors -- any win_size with min(win_size, h, w) <= 11 (even
and shrunk windows included), use_padding=True, size_average=False, full=True -- runs on mmif_metric_ssim_maps (csrc/metric_ssim.hip:
run-time window, reflect padding in the tile loader, fp64 arithmetic, optional ssim / cs maps and fp64 per-sample sums).
`calc_msssim` keeps mmif_metric_msssim (the loss's SSIM kernels and pyramid) for win_size 11 without padding from 161 px up; every other
CUDA call on images of at least 9x9 runs on mmif_metric_msssim_any (the same window kernel on an fp64 pyramid), and so does the
ssim / msssim pair of `fusion_metrics` below 161 px, in one call for the whole batch.  The other metrics run on csrc/metric.hip (moments,
histograms, entropies, Qabf, VIF).  Every kernel emits PER-SAMPLE raw terms (sums, counts), finished here in fp64 into
  * the reference's value for a [B,1,H,W] batch -- for B > 1 the POOLED value (e.g. the entropy of the summed histogram), and
  * `fusion_metrics`: one value per sample.
Values are 0-dim fp64 device tensors (calc_ssim: fp32, as the stock composition returned).  What stays on stock torch ops
(core/_stock.py), errors included: calc_ssim / calc_msssim on CPU tensors, windows above 11, and MS-SSIM below 9 px (where the
reference itself raises: level 3 is 1 px wide).
"""
import ctypes as C
from math import exp

import torch

from mmif import tensor as T
from mmif._lib import check, lib

from .loss import ssim_terms

__all__ = [
    'calc_mean', 'calc_std', 'calc_ag', 'calc_sf', 'calc_mse', 'calc_psnr',
    'calc_cc', 'calc_scd', 'calc_entropy', 'calc_cross_ent', 'calc_mul_info',
    'calc_Qabf', 'calc_Nabf', 'calc_Labf', 'calc_ssim', 'calc_msssim',
    'calc_viff'
]


def calc_ssim(img1, img2, win_size=11, data_range=255.0, use_padding=False, size_average=True, full=False):
    """SSIM of two single-channel image batches [B,1,H,W] (reference default data_range=255; test.py passes 1.0): the mean over the
    whole batch as a 0-dim tensor, or with size_average=False the per-pixel map [B,1,Hm,Wm]; full=True returns the pair (ssim, cs).
    The window is min(win_size, h, w) taps wide.  test.py's configuration runs on mmif_ssim_terms, every other call on CUDA tensors
    with a window of at most 11 on mmif_metric_ssim_maps; CPU tensors and larger windows run as stock torch ops (core/_stock.py)."""
    if img1.shape != img2.shape:
        raise ValueError("img1 and img2 must have the same shape")
    if img1.dim() != 4 or img1.shape[1] != 1:
        # the reference's window is [1,1,k,k] with groups=channel: it also only works for C == 1
        raise RuntimeError(f"calc_ssim takes single-channel images [B,1,H,W]; got {tuple(img1.shape)}")
    n, _, h, w = img1.shape
    if win_size != 11 or min(h, w) < 11 or use_padding or not size_average or full:
        if not (img1.is_cuda and img2.is_cuda) or win_size < 1 or min(win_size, h, w) > 11 or min(n, h, w) < 1:
            from . import _stock
            return _stock.metric_ssim(img1.float(), img2.float(), win_size, data_range, use_padding, size_average, full)
        a, b = _images(img1, img2, min_size=1, what='calc_ssim')
        if size_average:
            sums, hm, wm = _ssim_maps(a, b, win_size, use_padding, data_range, maps=False)
            ssim, cs = (sums.sum(0) / (n * hm * wm)).float()
        else:
            ssim, cs = _ssim_maps(a, b, win_size, use_padding, data_range, maps=True, cs=full)
        return (ssim, cs) if full else ssim
    T.require_device(img1, "img1")
    T.require_device(img2, "img2")
    a = img1.detach().contiguous().float()
    b = img2.detach().contiguous().float()
    # one evaluation of SSIM(a, b): the per-sample means of mmif_ssim_terms (csrc/loss_modes.hip, the kernel behind core.loss.SSIM);
    # equal-sized samples => mean of the per-sample means = the reference's mean over the whole batch.  (Rounds 1-4 went through the
    # two-source loss kernel with both sources = a, i.e. computed the same map twice.)
    return ssim_terms(a, b, 11, data_range, False)[0].mean()


# ------------------------------------------------------------------ input handling and the per-sample kernels
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
VIF_MIN = 41        # scale-4 map needs 3 px: 3 <- 7 <- 17 <- 41 through the valid filters and the [::2, ::2] decimations
MSSSIM_MIN = 161    # mmif_metric_msssim keeps the 11x11 window down to level 4
MSSSIM_ANY_MIN = 9  # mmif_metric_msssim_any: level 3 of a smaller image is 1 px wide and cannot be reflect-padded (the reference raises)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _images(*imgs, min_size=2, what='metric'):
    """validated contiguous fp32 [n][h][w] device views of equally-shaped [B,1,H,W] tensors"""
    shape = imgs[0].shape
    for t in imgs:
        if t.dim() != 4 or t.shape[1] != 1:
            raise RuntimeError(f"{what} takes single-channel images [B,1,H,W]; got {tuple(t.shape)}")
        if t.shape != shape:
            raise ValueError(f"{what}: all images must have the same shape; got {tuple(shape)} and {tuple(t.shape)}")
    if shape[-2] < min_size or shape[-1] < min_size:
        raise ValueError(f"{what} needs images of at least {min_size}x{min_size}; got {shape[-2]}x{shape[-1]}")
    for i, t in enumerate(imgs):
        T.require_device(t, f"{what} image {i}")
    return [t.detach().float().contiguous() for t in imgs]


def _workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dev)


def _moments(imgs):
    """[n, k + k*k + 3k] fp64: means, centred Gram matrix, AG sum, sum dy^2, sum dx^2 of each sample (mmif_metric_moments)"""
    k = len(imgs)
    n, _, h, w = imgs[0].shape
    out = torch.empty((n, k + k * k + 3 * k), dtype=torch.float64, device=imgs[0].device)
    ws = _workspace(lib.mmif_metric_moments_workspace(n, h, w, k), out.device)
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in imgs])
    check(lib.mmif_metric_moments(ptrs, k, n, h, w, _p(out), _p(ws), ws.numel(), T.stream_ptr()), "metric_moments")
    return out


def _stats(mo, k, h, w, pooled):
    """means mu [g,k], centred Gram G [g,k,k], AG / SF sums [g,k] and the pixel count of each group g: the samples themselves, or
    one pooled group (sums of the per-sample terms; the Gram matrix moves to the pooled means)"""
    mu = mo[:, :k]
    G = mo[:, k:k + k * k].reshape(-1, k, k)
    ag, sfr, sfc = mo[:, k + k * k:k + k * k + k], mo[:, k + k * k + k:k + k * k + 2 * k], mo[:, k + k * k + 2 * k:]
    npix = h * w
    if not pooled:
        return mu, G, ag, sfr, sfc, 1
    m = mu.mean(0, keepdim=True)
    d = mu - m
    G = G.sum(0, keepdim=True) + npix * torch.einsum('sj,sl->jl', d, d)[None]
    return m, G, ag.sum(0, keepdim=True), sfr.sum(0, keepdim=True), sfc.sum(0, keepdim=True), mo.shape[0]


def _hist(x, y):
    """u32 counts (held in int32 tensors) [n,256], [n,256], [n,65536] of x, y and (x, y)"""
    n, _, h, w = x.shape
    hx = torch.empty((n, 256), dtype=torch.int32, device=x.device)
    hy = torch.empty((n, 256), dtype=torch.int32, device=x.device)
    hxy = torch.empty((n, 65536), dtype=torch.int32, device=x.device)
    check(lib.mmif_metric_hist(_p(x), _p(y), n, h, w, _p(hx), _p(hy), _p(hxy), T.stream_ptr()), "metric_hist")
    return hx, hy, hxy


def _entropy(hx, hy, hxy, numel):
    """[n,4] fp64: EN(x), EN(y), joint entropy, CE(x||y)"""
    n = hx.shape[0]
    out = torch.empty((n, 4), dtype=torch.float64, device=hx.device)
    check(lib.mmif_metric_entropy(_p(hx), _p(hy), _p(hxy), n, int(numel), _p(out), T.stream_ptr()), "metric_entropy")
    return out


def _pooled_entropy(x, y):
    """entropy terms of the whole batch: one histogram of all its pixels"""
    hx, hy, hxy = _hist(x, y)
    if x.shape[0] > 1:
        hx, hy, hxy = (t.sum(0, keepdim=True, dtype=torch.int64).to(torch.int32) for t in (hx, hy, hxy))
    return _entropy(hx, hy, hxy, x.numel())[0]


def _qabf(a, b, f, L):
    """[n,5] fp64 Qabf-family sums (mmif_metric_qabf)"""
    n, _, h, w = a.shape
    out = torch.empty((n, 5), dtype=torch.float64, device=a.device)
    ws = _workspace(lib.mmif_metric_qabf_workspace(n, h, w), a.device)
    check(lib.mmif_metric_qabf(_p(a), _p(b), _p(f), n, h, w, float(L), _p(out), _p(ws), ws.numel(), T.stream_ptr()), "metric_qabf")
    return out


_VIF_TAPS = None


def _vif_taps():
    """the four normalised 1-D Gaussians of the VIF scales, built as the reference's create_window does (fp32 taps / fp32 sum)"""
    global _VIF_TAPS
    if _VIF_TAPS is None:
        taps = []
        for scale in range(1, 5):
            k = 2 ** (4 - scale + 1) + 1
            sigma = k / 5
            g = torch.FloatTensor([exp(-(x - k // 2) ** 2 / (2.0 * sigma ** 2)) for x in range(k)])
            taps += (g / g.sum()).tolist()
        _VIF_TAPS = (C.c_float * len(taps))(*taps)
    return _VIF_TAPS


def _vif(a, b, f):
    """[4,n,6] fp64: per scale sum N1, D1, N2, D2, sum (g1 < g2 ? N1 : N2), sum (g1 < g2 ? D1 : D2)"""
    n, _, h, w = a.shape
    out = torch.empty((4, n, 6), dtype=torch.float64, device=a.device)
    ws = _workspace(lib.mmif_metric_vif_workspace(n, h, w), a.device)
    check(lib.mmif_metric_vif(_p(a), _p(b), _p(f), n, h, w, _vif_taps(), _p(out), _p(ws), ws.numel(), T.stream_ptr()), "metric_vif")
    return out


def _msssim_terms(a, b, f, data_range):
    """[2,6,n] fp32: per pair (a, f) | (b, f) the cs means of levels 0..3, the ssim mean of level 4, the level-0 ssim mean"""
    n, _, h, w = a.shape
    out = torch.empty((2, 6, n), dtype=torch.float32, device=a.device)
    ws = _workspace(lib.mmif_metric_msssim_workspace(n, h, w), a.device)
    check(lib.mmif_metric_msssim(_p(a), _p(b) if b is not None else None, _p(f), n, h, w, float(data_range), _p(out), _p(ws), ws.numel(),
                                 T.stream_ptr()), "metric_msssim")
    return out


def _ssim_maps(a, b, win_size, use_padding, data_range, maps, cs=True):
    """mmif_metric_ssim_maps on fp32 [n,1,h,w] images: maps=False -> (fp64 sums [n, 2] = sum ssim, sum cs of each sample, Hm, Wm);
    maps=True -> (ssim map, cs map | None) fp32 [n,1,Hm,Wm]"""
    n, _, h, w = a.shape
    k = min(win_size, h, w)
    p = k // 2 if use_padding else 0
    hm, wm = h + 2 * p - k + 1, w + 2 * p - k + 1
    if maps:
        sm = torch.empty((n, 1, hm, wm), dtype=torch.float32, device=a.device)
        cm = torch.empty_like(sm) if cs else None
        check(lib.mmif_metric_ssim_maps(_p(a), _p(b), n, h, w, int(win_size), int(bool(use_padding)), float(data_range), _p(sm),
                                        _p(cm) if cs else None, None, None, 0, T.stream_ptr()), "metric_ssim_maps")
        return sm, cm
    sums = torch.empty((n, 2), dtype=torch.float64, device=a.device)
    ws = _workspace(lib.mmif_metric_ssim_maps_workspace(n, h, w, int(win_size), int(bool(use_padding))), a.device)
    check(lib.mmif_metric_ssim_maps(_p(a), _p(b), n, h, w, int(win_size), int(bool(use_padding)), float(data_range), None, None, _p(sums),
                                    _p(ws), ws.numel(), T.stream_ptr()), "metric_ssim_maps")
    return sums, hm, wm


def _msssim_any(a, b, f, win_size, use_padding, data_range):
    """[2,6,n] fp64 in the layout of _msssim_terms, for any window up to 11, padded or not, images from 9x9 (mmif_metric_msssim_any)"""
    n, _, h, w = a.shape
    out = torch.empty((2, 6, n), dtype=torch.float64, device=a.device)
    ws = _workspace(lib.mmif_metric_msssim_any_workspace(n, h, w), a.device)
    check(lib.mmif_metric_msssim_any(_p(a), _p(b) if b is not None else None, _p(f), n, h, w, int(win_size), int(bool(use_padding)),
                                     float(data_range), _p(out), _p(ws), ws.numel(), T.stream_ptr()), "metric_msssim_any")
    return out


def _ms_combine(vals):
    """prod_l clamp(v_l, 1e-7)^w_l over the first axis (core/metric.py:398-401), as elementwise products in level order: a torch
    reduction over that axis may order its work by the width of the other axes, and a sample's value must not depend on B"""
    wts = torch.tensor(MS_WEIGHTS, dtype=torch.float32).to(vals)
    v = vals.clamp(min=1e-7)
    out = v[0] ** wts[0]
    for lvl in range(1, len(MS_WEIGHTS)):
        out = out * v[lvl] ** wts[lvl]
    return out


_VIF_P = torch.tensor([1.0, 0.0, 0.15, 1.0], dtype=torch.float32) / 2.15


def _viff_value(v, simple):
    """calc_viff from [4, g, 6] scale sums (g = samples or one pooled group)"""
    tot = lambda t: t[0] + t[1] + t[2] + t[3]   # scale order, elementwise (see _ms_combine)
    if simple:
        return tot(v[:, :, 0]) / tot(v[:, :, 1]) + tot(v[:, :, 2]) / tot(v[:, :, 3])
    p = _VIF_P.to(v)
    return tot(p[:, None] * (v[:, :, 4] / v[:, :, 5]))


# ------------------------------------------------------------------ the reference's functions (pooled over the batch)
def calc_mean(img):
    (x,) = _images(img, what='calc_mean')
    mu, *_ = _stats(_moments([x]), 1, x.shape[-2], x.shape[-1], True)
    return mu[0, 0]


def calc_std(img):
    (x,) = _images(img, what='calc_std')
    n, _, h, w = x.shape
    _, G, _, _, _, g = _stats(_moments([x]), 1, h, w, True)
    return (G[0, 0, 0] / (g * h * w)).sqrt()


def calc_ag(img):
    (x,) = _images(img, what='calc_ag')
    n, _, h, w = x.shape
    _, _, ag, _, _, g = _stats(_moments([x]), 1, h, w, True)
    return ag[0, 0] / (g * (h - 1) * (w - 1))


def calc_sf(img):
    (x,) = _images(img, what='calc_sf')
    n, _, h, w = x.shape
    _, _, _, sfr, sfc, g = _stats(_moments([x]), 1, h, w, True)
    return (sfr[0, 0] / (g * (h - 1) * w) + sfc[0, 0] / (g * h * (w - 1))).sqrt()


def _mse_of(mu, G, npix, i, j):
    """MSE / 255^2 of images i, j of a group from the centred Gram matrix: (sum (x_i' - x_j')^2 + N (mu_i - mu_j)^2) / N / 255^2"""
    return ((G[:, i, i] - 2.0 * G[:, i, j] + G[:, j, j]) / npix + (mu[:, i] - mu[:, j]) ** 2) / (255.0 * 255.0)


def calc_mse(img1, img2):
    a, b = _images(img1, img2, what='calc_mse')
    n, _, h, w = a.shape
    mu, G, _, _, _, g = _stats(_moments([a, b]), 2, h, w, True)
    return _mse_of(mu, G, g * h * w, 0, 1)[0]


def calc_psnr(mse, L=1.0, root=False):
    if root:
        return 20.0 * torch.log10(L / mse**0.5)
    return 10.0 * torch.log10(L**2 / mse)


def _cc_of(G, i, j):
    return G[:, i, j] / (G[:, i, i] * G[:, j, j]).sqrt()


def _scd_of(G, a, b, f):
    """cc(f - a, b) + cc(f - b, a) from the Gram matrix of (a, b, f): sum (f - a)'b' = sum f'b' - sum a'b'"""
    c1 = (G[:, f, b] - G[:, a, b]) / ((G[:, f, f] - 2.0 * G[:, f, a] + G[:, a, a]) * G[:, b, b]).sqrt()
    c2 = (G[:, f, a] - G[:, b, a]) / ((G[:, f, f] - 2.0 * G[:, f, b] + G[:, b, b]) * G[:, a, a]).sqrt()
    return c1 + c2


def calc_cc(img1, img2):
    a, b = _images(img1, img2, what='calc_cc')
    _, G, *_ = _stats(_moments([a, b]), 2, a.shape[-2], a.shape[-1], True)
    return _cc_of(G, 0, 1)[0]


def calc_scd(img1, img2, imgf):
    a, b, f = _images(img1, img2, imgf, what='calc_scd')
    _, G, *_ = _stats(_moments([a, b, f]), 3, a.shape[-2], a.shape[-1], True)
    return _scd_of(G, 0, 1, 2)[0]


def calc_entropy(img):
    (x,) = _images(img, min_size=1, what='calc_entropy')
    return _pooled_entropy(x, x)[0]


def calc_cross_ent(img1, img2):
    a, b = _images(img1, img2, min_size=1, what='calc_cross_ent')
    return _pooled_entropy(a, b)[3]


def calc_mul_info(img1, img2, normalized=False):
    a, b = _images(img1, img2, min_size=1, what='calc_mul_info')
    e = _pooled_entropy(a, b)
    mi = e[0] + e[1] - e[2]
    if normalized:
        return 2.0 * mi / (e[0] + e[1])
    return mi


def _qabf_sums(img1, img2, imgf, L, what):
    a, b, f = _images(img1, img2, imgf, what=what)
    return _qabf(a, b, f, L).sum(0)


def calc_Qabf(img1, img2, imgf, L=1.5, full=False):
    s = _qabf_sums(img1, img2, imgf, L, 'calc_Qabf')
    if full:
        return s[0] / s[1], s[2] / s[1], s[3] / s[1]   # qabf + nabf + labf = 1
    return s[0] / s[1]


def calc_Nabf(img1, img2, imgf, L=1.5, modified=True):
    s = _qabf_sums(img1, img2, imgf, L, 'calc_Nabf')
    return s[2] / s[1] if modified else s[4] / s[1]


def calc_Labf(img1, img2, imgf, L=1.5):
    s = _qabf_sums(img1, img2, imgf, L, 'calc_Labf')
    return s[3] / s[1]


def calc_msssim(img1, img2, win_size=11, data_range=255.0, use_padding=False):
    """MS-SSIM of two batches (pooled means per level).  win_size 11 without padding on images >= 161 px runs on mmif_metric_msssim;
    every other call on CUDA tensors of at least 9x9 with a window of at most 11 on mmif_metric_msssim_any; the rest (CPU tensors,
    larger windows, images below 9 px, where the reference raises) as stock torch ops."""
    if img1.dim() != 4 or img1.shape[1] != 1 or img1.shape != img2.shape:
        raise RuntimeError(f"calc_msssim takes two single-channel batches [B,1,H,W] of one shape; got {tuple(img1.shape)}, {tuple(img2.shape)}")
    n, _, h, w = img1.shape
    if win_size != 11 or use_padding or min(h, w) < MSSSIM_MIN:
        if not (img1.is_cuda and img2.is_cuda) or win_size < 1 or min(win_size, h, w) > 11 or min(h, w) < MSSSIM_ANY_MIN or n < 1:
            from . import _stock
            return _stock.metric_msssim(img1.double(), img2.double(), win_size, data_range, use_padding)
        a, b = _images(img1, img2, what='calc_msssim')
        return _ms_combine(_msssim_any(a, None, b, win_size, use_padding, data_range)[0, :5].mean(1))
    a, b = _images(img1, img2, what='calc_msssim')
    v = _msssim_terms(a, None, b, data_range)[0, :5].double().mean(1)
    return _ms_combine(v)


def calc_viff(img1, img2, imgf, simple=True):
    a, b, f = _images(img1, img2, imgf, min_size=VIF_MIN, what='calc_viff')
    v = _vif(a, b, f).sum(1, keepdim=True)
    return _viff_value(v, simple)[0]


# ------------------------------------------------------------------ eval.py's table, one value per sample
FUSION_METRICS = ('sd', 'ag', 'sf', 'mse', 'psnr', 'cc', 'scd', 'en', 'ce', 'mi', 'qabf', 'nabf', 'labf', 'ssim', 'msssim', 'viff')


def fusion_metrics(img1, img2, imgf):
    """The 16 values of the reference's eval_metrics (eval.py:29-76) for every sample of a [B,1,H,W] triple (sources img1, img2,
    fused imgf, 0..255 values): a dict of [B] fp64 device tensors.  One call per kernel family for the whole batch, no host sync.
    Images of at least 41x41 (VIF); below 161 px ssim and msssim come from one mmif_metric_msssim_any call."""
    a, b, f = _images(img1, img2, imgf, min_size=VIF_MIN, what='fusion_metrics')
    n, _, h, w = a.shape
    npix = h * w
    mu, G, ag, sfr, sfc, _ = _stats(_moments([a, b, f]), 3, h, w, False)
    r = {}
    r['sd'] = (G[:, 2, 2] / npix).sqrt()
    r['ag'] = ag[:, 2] / ((h - 1) * (w - 1))
    r['sf'] = (sfr[:, 2] / ((h - 1) * w) + sfc[:, 2] / (h * (w - 1))).sqrt()
    r['mse'] = (_mse_of(mu, G, npix, 0, 2) + _mse_of(mu, G, npix, 1, 2)) * 0.5
    r['psnr'] = calc_psnr(r['mse'])
    r['cc'] = (_cc_of(G, 0, 2) + _cc_of(G, 1, 2)) * 0.5
    r['scd'] = _scd_of(G, 0, 1, 2)
    e = _entropy(*_hist(torch.cat([a, b]), torch.cat([f, f])), npix)   # rows: (a, f) of every sample, then (b, f)
    ea, eb = e[:n], e[n:]
    r['en'] = ea[:, 1]
    r['ce'] = ea[:, 3] + eb[:, 3]
    r['mi'] = (2.0 * (ea[:, 0] + ea[:, 1] - ea[:, 2]) / (ea[:, 0] + ea[:, 1])
               + 2.0 * (eb[:, 0] + eb[:, 1] - eb[:, 2]) / (eb[:, 0] + eb[:, 1]))
    q = _qabf(a, b, f, 1.5)
    r['qabf'], r['nabf'], r['labf'] = q[:, 0] / q[:, 1], q[:, 2] / q[:, 1], q[:, 3] / q[:, 1]
    if min(h, w) >= MSSSIM_MIN:
        ms = _msssim_terms(a, b, f, 255.0).double()
    else:
        ms = _msssim_any(a, b, f, 11, False, 255.0)
    r['ssim'] = (ms[0, 5] + ms[1, 5]) * 0.5
    r['msssim'] = (_ms_combine(ms[0, :5]) + _ms_combine(ms[1, :5])) * 0.5
    r['viff'] = _viff_value(_vif(a, b, f), False)
    return {k: r[k] for k in FUSION_METRICS}
