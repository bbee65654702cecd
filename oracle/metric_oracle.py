"""fp64 CPU oracle of the fusion-quality metrics (core/metric.py on csrc/metric.hip and mmif_metric_msssim).

TEST INFRASTRUCTURE ONLY, like fusion_oracle.py: nothing under ``multi-modal-image-fusion_amd/`` imports it.  Pinned to the
reference by golden F19 (tests/test_metric_oracle_cpu.py); tests/test_gpu_metric_sweep.py then compares the kernels against it at
shapes, values and batch sizes F19 does not hold.

Inputs are numpy arrays [B,1,H,W] (any real dtype; everything is computed in float64).  Each metric is restated from its definition:

* mean, sd         mean of x; sqrt(mean((x - mean)^2))
* ag               mean over the (H-1)(W-1) top-left pixels of sqrt((dx^2 + dy^2) / 2), dx = x[i, j+1] - x[i, j], dy = x[i+1, j] - x[i, j]
* sf               sqrt(mean(dy^2) + mean(dx^2)), dy over (H-1) x W pixel pairs, dx over H x (W-1)
* mse              mean((x / 255 - y / 255)^2);  psnr = 10 log10(L^2 / mse), root form 20 log10(L / sqrt(mse))
* cc               sum(x' y') / sqrt(sum(x'^2) sum(y'^2)) of the mean-removed images;  scd = cc(f - a, b) + cc(f - b, a)
* histograms       256 unit bins on [0, 256): bin floor(v), v == 256 counts in bin 255, anything else (v < 0, v > 256, NaN) is
                   dropped but still counted in numel; joint histogram the same in both coordinates
* en               -sum p log2 p over the non-empty bins of p = hist / numel
* ce(x, y)         sum p1 log2(p1 / p2) over the bins where p1 p2 != 0
* mi               en(x) + en(y) - je(x, y); normalised 2 mi / (en(x) + en(y)) (0/0 = NaN is kept)
* Qabf family      Sobel cross-correlation ([[-1,0,1],[-2,0,2],[-1,0,1]] and its transpose) on a 1-px reflect pad; g = |grad|,
                   a = atan2(gy, gx).  Per pair (x, f): G = min(gx, gf) / max(gx, gf) with 0/0 -> 0,
                   A = ||a_x - a_f| - pi/2| * 2/pi, Q = 0.9994 / (1 + exp(-15 (G - 0.5))) * 0.9879 / (1 + exp(-22 (A - 0.8))).
                   wa = ga^L, wb = gb^L, AM = [gf > max(ga, gb)], RR = [gf <= max(ga, gb)]:
                   qabf = sum(Qaf wa + Qbf wb) / sum(wa + wb); nabf (modified) = sum AM ((1-Qaf) wa + (1-Qbf) wb) / sum(wa + wb);
                   nabf (original) = sum AM (2 - Qaf - Qbf)(wa + wb) / sum(wa + wb); labf = the modified nabf sum under RR
* ssim, msssim     core/_stock.py (metric_ssim / metric_msssim) on float64 tensors, pinned to F19 by tests/test_metric_cpu.py
* viff             4 scales, window of scale s (1..4) K = 2^(5-s) + 1 taps of a Gaussian with sigma K / 5: fp32 taps divided by
                   their fp32 sum, 2-D weight = fp32 product of two taps, applied in fp64 as a valid correlation.  Scales > 1 first
                   filter the previous level with their own window and keep [::2, ::2].  Per pair (x, f) and pixel, with
                   s1 = E[x^2] - mu_x^2, s2 = E[f^2] - mu_f^2, s12 = E[x f] - mu_x mu_f, eps = 1e-10, sn = 0.005 * 255^2, in order:
                   s1, s2 clamped at 0; g = s12 / (s1 + eps); sv = s2 - g s12; where s1 < eps: g = 0, sv = s2, s1 = 0;
                   where s2 < eps: g = 0, sv = 0; where g < 0: sv = s2, g = 0; sv clamped at eps.
                   N = log2(1 + g^2 s1 / (sv + sn)), D = log2(1 + s1 / sn).
                   simple: sum N1 / sum D1 + sum N2 / sum D2 over all scales;
                   full: sum_s p_s sum(g1 < g2 ? N1 : N2) / sum(g1 < g2 ? D1 : D2), p = (1, 0, 0.15, 1) / 2.15 (fp32).
                   The reference keeps the four per-scale ratios of the full form in an fp32 tensor; here (as in the kernels) they
                   stay fp64, so viff_full agrees with F19 to fp32 rounding only (~1e-7 relative).

A batch is one image set for the mirror functions (pooled means, summed histograms, sums over all samples); `eval_table` gives
eval.py's 16 values per sample.
"""
from math import exp, pi

import numpy as np
import torch
import torch.nn.functional as F

FUSION_METRICS = ('sd', 'ag', 'sf', 'mse', 'psnr', 'cc', 'scd', 'en', 'ce', 'mi', 'qabf', 'nabf', 'labf', 'ssim', 'msssim', 'viff')
VIF_P = (torch.tensor([1.0, 0.0, 0.15, 1.0], dtype=torch.float32) / 2.15).double().numpy()


def _d(x):
    return np.asarray(x, dtype=np.float64)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(_d(x)))


# ------------------------------------------------------------------ moments family (any batch: pooled over all of it)
def mean(x):
    return _d(x).mean()


def std(x):
    x = _d(x)
    return np.sqrt(((x - x.mean()) ** 2).mean())


def ag(x):
    x = _d(x)
    dx = x[..., :-1, 1:] - x[..., :-1, :-1]
    dy = x[..., 1:, :-1] - x[..., :-1, :-1]
    return np.sqrt((dx * dx + dy * dy) * 0.5).mean()


def sf(x):
    x = _d(x)
    dy = x[..., 1:, :] - x[..., :-1, :]
    dx = x[..., :, 1:] - x[..., :, :-1]
    return np.sqrt((dy * dy).mean() + (dx * dx).mean())


def mse(x, y):
    e = _d(x) / 255.0 - _d(y) / 255.0
    return (e * e).mean()


def psnr(m, L=1.0, root=False):
    with np.errstate(divide='ignore'):
        return 20.0 * np.log10(L / np.sqrt(m)) if root else 10.0 * np.log10(L * L / m)


def cc(x, y):
    x, y = _d(x), _d(y)
    x, y = x - x.mean(), y - y.mean()
    with np.errstate(invalid='ignore', divide='ignore'):
        return (x * y).sum() / np.sqrt((x * x).sum() * (y * y).sum())


def scd(a, b, f):
    a, b, f = _d(a), _d(b), _d(f)
    return cc(f - a, b) + cc(f - b, a)


# ------------------------------------------------------------------ histograms and entropies
def hist(x):
    return np.histogram(_d(x).ravel(), 256, (0.0, 256.0))[0]


def hist2(x, y):
    return np.histogram2d(_d(x).ravel(), _d(y).ravel(), 256, ((0.0, 256.0), (0.0, 256.0)))[0]


def _ent(p):
    p = p[p != 0]
    return -(p * np.log2(p)).sum()


def entropy(x):
    return _ent(hist(x) / np.size(x))


def cross_ent(x, y):
    p1, p2 = hist(x) / np.size(x), hist(y) / np.size(y)
    m = p1 * p2 != 0
    return (p1[m] * np.log2(p1[m] / p2[m])).sum()


def mul_info(x, y, normalized=False):
    e1, e2, je = entropy(x), entropy(y), _ent(hist2(x, y) / np.size(x))
    mi = e1 + e2 - je
    if normalized:
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.float64(2.0) * mi / (e1 + e2)
    return mi


# ------------------------------------------------------------------ Qabf family: per-pixel maps, summed per sample or pooled
_SOBEL_X = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=torch.float64)[None, None]


def sobel(x):
    """(|grad|, atan2(gy, gx)) of the 3x3 Sobel correlation on a 1-px reflect pad, [B,1,H,W] fp64 tensors"""
    p = F.pad(_t(x), (1, 1, 1, 1), mode='reflect')
    gx = F.conv2d(p, _SOBEL_X)
    gy = F.conv2d(p, _SOBEL_X.transpose(-1, -2))
    return (gx * gx + gy * gy).sqrt(), torch.atan2(gy, gx)


def _qxy(g1, a1, g2, a2):
    G = torch.min(g1, g2) / torch.max(g1, g2)
    G = torch.where(torch.isnan(G), torch.zeros_like(G), G)
    A = ((a1 - a2).abs() - pi / 2).abs() * 2 / pi
    return 0.9994 / (1 + torch.exp(-15 * (G - 0.5))) * (0.9879 / (1 + torch.exp(-22 * (A - 0.8))))


def qabf_sums(a, b, f, Ls=(1.5,)):
    """[len(Ls), B, 5] fp64 per-sample sums for each exponent L: sum(Qaf wa + Qbf wb), sum(wa + wb), sum AM loss, sum RR loss,
    sum AM (2 - Qaf - Qbf)(wa + wb), loss = (1 - Qaf) wa + (1 - Qbf) wb"""
    (ga, aa), (gb, ab), (gf, af) = sobel(a), sobel(b), sobel(f)
    qaf, qbf = _qxy(ga, aa, gf, af), _qxy(gb, ab, gf, af)
    gm = torch.max(ga, gb)
    am, rr = gf > gm, gf <= gm
    out = []
    for L in Ls:
        wa, wb = ga ** L, gb ** L
        loss = (1.0 - qaf) * wa + (1.0 - qbf) * wb
        z = torch.zeros_like(loss)
        terms = [qaf * wa + qbf * wb, wa + wb, torch.where(am, loss, z), torch.where(rr, loss, z),
                 torch.where(am, (2.0 - qaf - qbf) * (wa + wb), z)]
        out.append(torch.stack([t.sum(dim=(1, 2, 3)) for t in terms], 1))
    return torch.stack(out).numpy()


def _qabf_values(s):
    """qabf, nabf (modified), labf, nabf (original) of [..., 5] sums"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return s[..., 0] / s[..., 1], s[..., 2] / s[..., 1], s[..., 3] / s[..., 1], s[..., 4] / s[..., 1]


# ------------------------------------------------------------------ VIF
def vif_window(k):
    """[1,1,k,k] fp64 tensor holding fp32(t_u * t_v) of the fp32 taps t = g / sum(g), g_i = exp(-(i - k//2)^2 / (2 (k/5)^2))"""
    sigma = k / 5
    g = torch.tensor([exp(-(i - k // 2) ** 2 / (2.0 * sigma ** 2)) for i in range(k)], dtype=torch.float32)
    t = g / g.sum()
    return (t[:, None] * t[None, :]).double()[None, None]


def _vif_pair(mx, mf, exx, eff, exf):
    eps, sn = 1e-10, 0.005 * 255 * 255
    s1 = (exx - mx * mx).clamp(min=0)
    s2 = (eff - mf * mf).clamp(min=0)
    s12 = exf - mx * mf
    g = s12 / (s1 + eps)
    sv = s2 - g * s12
    m = s1 < eps
    g, sv, s1 = torch.where(m, 0.0, g), torch.where(m, s2, sv), torch.where(m, 0.0, s1)
    m = s2 < eps
    g, sv = torch.where(m, 0.0, g), torch.where(m, 0.0, sv)
    m = g < 0
    sv, g = torch.where(m, s2, sv), torch.where(m, 0.0, g)
    sv = sv.clamp(min=eps)
    return torch.log2(1 + g * g * s1 / (sv + sn)), torch.log2(1 + s1 / sn), g


def vif_sums(a, b, f):
    """[4, B, 6] fp64 per scale and sample: sum N1, D1, N2, D2, sum (g1 < g2 ? N1 : N2), sum (g1 < g2 ? D1 : D2)"""
    x = torch.cat([_t(a), _t(b), _t(f)], 1)   # [B,3,H,W]
    out = []
    for scale in range(1, 5):
        k = 2 ** (4 - scale + 1) + 1
        win = vif_window(k).expand(3, 1, k, k)
        if scale > 1:
            x = F.conv2d(x, win, groups=3)[..., ::2, ::2]
        w8 = vif_window(k).expand(8, 1, k, k)
        a_, b_, f_ = x[:, 0:1], x[:, 1:2], x[:, 2:3]
        m = F.conv2d(torch.cat([a_, b_, f_, a_ * a_, b_ * b_, f_ * f_, a_ * f_, b_ * f_], 1), w8, groups=8)
        n1, d1, g1 = _vif_pair(m[:, 0], m[:, 2], m[:, 3], m[:, 5], m[:, 6])
        n2, d2, g2 = _vif_pair(m[:, 1], m[:, 2], m[:, 4], m[:, 5], m[:, 7])
        sel = g1 < g2
        terms = [n1, d1, n2, d2, torch.where(sel, n1, n2), torch.where(sel, d1, d2)]
        out.append(torch.stack([t.sum(dim=(1, 2)) for t in terms], 1))
    return torch.stack(out).numpy()


def viff_value(v, simple):
    """viff of [4, 6] scale sums"""
    with np.errstate(invalid='ignore', divide='ignore'):
        if simple:
            return v[:, 0].sum() / v[:, 1].sum() + v[:, 2].sum() / v[:, 3].sum()
        return (VIF_P * (v[:, 4] / v[:, 5])).sum()


def viff(a, b, f, simple=True):
    return viff_value(vif_sums(a, b, f).sum(1), simple)


# ------------------------------------------------------------------ SSIM family (stock torch, fp64)
def ssim(x, y, data_range=255.0):
    from core import _stock
    return float(_stock.metric_ssim(_t(x), _t(y), 11, data_range))


def msssim(x, y, data_range=255.0, use_padding=False):
    from core import _stock
    return float(_stock.metric_msssim(_t(x), _t(y), 11, data_range, use_padding))


# ------------------------------------------------------------------ the whole tables
MOMENT_KEYS = ('mean', 'std', 'ag', 'sf', 'mse', 'psnr', 'psnr_root', 'cc', 'scd')
ENTROPY_KEYS = ('en', 'en_a', 'ce', 'mi', 'mi_norm')
QABF_KEYS = ('qabf', 'qabf_L1', 'nabf', 'nabf_orig', 'labf', 'qabf_full_q', 'qabf_full_n', 'qabf_full_l')
SSIM_KEYS = ('ssim', 'msssim', 'msssim_pad')
VIF_KEYS = ('viff', 'viff_full')


def mirror(a, b, f, parts=('moments', 'entropy', 'qabf', 'ssim', 'vif')):
    """the reference's functions as tests/test_gpu_metric.py calls them, pooled over the batch; `parts` picks the families"""
    v = {}
    if 'moments' in parts:
        m = mse(a, f)
        v.update(mean=mean(f), std=std(f), ag=ag(f), sf=sf(f), mse=m, psnr=psnr(m), psnr_root=psnr(m, 1.0, True), cc=cc(a, f),
                 scd=scd(a, b, f))
    if 'entropy' in parts:
        v.update(en=entropy(f), en_a=entropy(a), ce=cross_ent(a, f), mi=mul_info(a, f), mi_norm=mul_info(a, f, True))
    if 'qabf' in parts:
        s15, s10 = qabf_sums(a, b, f, (1.5, 1.0)).sum(1)
        (q, n, lb, n0), q1 = _qabf_values(s15), _qabf_values(s10)[0]
        v.update(qabf=q, qabf_L1=q1, nabf=n, nabf_orig=n0, labf=lb, qabf_full_q=q, qabf_full_n=n, qabf_full_l=lb)
    if 'ssim' in parts:
        v.update(ssim=ssim(a, f), msssim=msssim(a, f), msssim_pad=msssim(a, f, use_padding=True))
    if 'vif' in parts and min(np.shape(a)[-2:]) >= 41:
        s = vif_sums(a, b, f).sum(1)
        v.update(viff=viff_value(s, True), viff_full=viff_value(s, False))
    return {k: np.float64(x) for k, x in v.items()}


def eval_table(a, b, f, vif=None):
    """eval.py's 16 values for every sample: {name: [B] fp64}; `vif` = vif_sums(a, b, f) if already at hand"""
    a, b, f = _d(a), _d(b), _d(f)
    rows = []
    q = qabf_sums(a, b, f)[0]
    vs = vif_sums(a, b, f) if vif is None else vif
    for s in range(a.shape[0]):
        x, y, z = a[s:s + 1], b[s:s + 1], f[s:s + 1]
        m = (mse(x, z) + mse(y, z)) * 0.5
        qa, na, la, _ = _qabf_values(q[s])
        rows.append({
            'sd': std(z), 'ag': ag(z), 'sf': sf(z), 'mse': m, 'psnr': psnr(m), 'cc': (cc(x, z) + cc(y, z)) * 0.5, 'scd': scd(x, y, z),
            'en': entropy(z), 'ce': cross_ent(x, z) + cross_ent(y, z), 'mi': mul_info(x, z, True) + mul_info(y, z, True),
            'qabf': qa, 'nabf': na, 'labf': la, 'ssim': (ssim(x, z) + ssim(y, z)) * 0.5, 'msssim': (msssim(x, z) + msssim(y, z)) * 0.5,
            'viff': viff_value(vs[:, s], False),
        })
    return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in FUSION_METRICS}
