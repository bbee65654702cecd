"""The case table and the torch definition of the metric-side SSIM / MS-SSIM (mmif_metric_ssim_maps, mmif_metric_msssim_any and the
calc_ssim / calc_msssim / fusion_metrics routes of core/metric.py), shared by tests/test_ssim_metric_oracle_cpu.py (which pins the
definition, run in float64, to the reference through golden F21) and tests/test_gpu_ssim_metric_sweep.py.

The definition (`maps`, `ms_levels`, `ms_value`), written from the maths:
  window  k = min(win_size, h, w); taps exp(-(i - k // 2)^2 / (2 * 1.5^2)) in double -> float32, divided by their float32 sum; the k x k
          weights are the float32 products of two taps, cast to the images' dtype
  pass    correlation of the (optionally reflect-padded by p = k // 2) image with the window: (h + 2p - k + 1) x (w + 2p - k + 1)
  pixel   var_i = max(E[x_i^2] - mu_i^2, 0), cov = E[x1 x2] - mu1 mu2 (not clamped), C1 = (0.01 L)^2, C2 = (0.03 L)^2,
          cs = (2 cov + C2) / (var1 + var2 + C2),  ssim = (2 mu1 mu2 + C1)(2 cov + C2) / ((mu1^2 + mu2^2 + C1)(var1 + var2 + C2))
  pyramid 2 x 2 means of the image reflect-padded by one row / column at the bottom / right when the extent is odd; five levels, the
          window re-derived per level; means of cs on levels 0-3 and of ssim on level 4, clamped at 1e-7, to the powers MS_WEIGHTS (held in float32)
`dtype` selects the precision of everything after the window (float64: the definition; float32: the yardstick of the tolerances);
`variant` swaps in one of the wrong-but-plausible VARIANTS.

Tolerances (`tol`): 8 x the error of the float32 evaluation of the same case on the CPU -- per case and per output, the per-pixel maximum
for maps and the absolute error for means -- with a floor of 2^-22 relative to max(|ref|, 0.1).  Nothing is measured on the code under test.

Shapes: every window class (1, even, odd, 11) on 20 x 23; images smaller than the window (1 x 1 ... 10 x 10, 9 x 300); map extents 15 /
16 / 17 / 33 around the 16-pixel tile in each axis; MS-SSIM from the smallest image (9 x 9: levels 9, 5, 3, 2, 1) over 40 x 40 (level
windows 11, 11, 10, 5, 3) to the 161 class that the 11-tap pyramid kernel takes without padding."""
import functools
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
DISTS = ('rand1', 'rand255', 'blend', 'flat', 'anti', 'const')
VARIANTS = ('loss-sigma', 'no-shrink', 'symmetric', 'cov-clamped', 'even-crop')          # of the maps
MS_VARIANTS = ('frozen-window', 'last-cs')                                                # of the pyramid
FLOOR = 2.0 ** -22


def data_range(dist):
    return 1.0 if dist == 'rand1' else 255.0


# name -> (kind, h, w, n, win_size, use_padding, dist)
CASES = {}


def _add(kind, h, w, n, win, pad, dist):
    CASES[f"{kind}-{h}x{w}-b{n}-k{win}-{'pad' if pad else 'valid'}-{dist}"] = (kind, h, w, n, win, int(pad), dist)


_i = 0
for _win in (1, 2, 3, 8, 10, 11):                                    # (a) every window class
    for _pad in (0, 1):
        _add('ssim', 20, 23, 1 + (_i // 2) % 3, _win, _pad, DISTS[_i % 6])
        _i += 1
for _h, _w in ((1, 1), (2, 2), (3, 5), (9, 300), (10, 10)):          # (b) the window shrinks to the image
    for _pad in (0, 1):
        _add('ssim', _h, _w, 1 + (_i // 2) % 3, 11, _pad, DISTS[_i % 6])
        _i += 1
for _hm, _wm in ((15, 33), (16, 17), (17, 16), (33, 15), (16, 16)):  # (c) map extents around the tile edge
    _add('ssim', _hm + 10, _wm + 10, 1 + _i % 3, 11, 0, DISTS[_i % 6])
    _add('ssim', _hm, _wm, 1 + (_i + 1) % 3, 11, 1, DISTS[(_i + 3) % 6])
    _i += 1
for _d in ('flat', 'anti', 'const', 'blend'):                        # (g) every distribution at one mid-size shape, even padded window
    _add('ssim', 37, 52, 2, 8, 1, _d)
_add('ssim', 200, 200, 1, 11, 0, 'blend')
for _h, _w in ((9, 9), (9, 300), (16, 16), (17, 31), (40, 40)):      # (d) the pyramid
    for _pad in (0, 1):
        _add('ms', _h, _w, 1 + (_i // 2) % 3, 11, _pad, DISTS[_i % 5])
        _i += 1
_add('ms', 40, 40, 2, 7, 0, 'anti')
_add('ms', 40, 40, 3, 8, 1, 'flat')
_add('ms', 64, 80, 2, 11, 0, 'anti')
_add('ms', 33, 47, 1, 11, 1, 'const')
_add('ms', 160, 200, 1, 11, 1, 'blend')
_add('ms', 161, 176, 2, 11, 1, 'rand255')
_add('ms', 161, 176, 2, 11, 0, 'blend')          # through mmif_metric_msssim_any directly; core.metric keeps mmif_metric_msssim here
SSIM_CASES = [k for k, v in CASES.items() if v[0] == 'ssim']
MS_CASES = [k for k, v in CASES.items() if v[0] == 'ms']


@functools.lru_cache(maxsize=None)
def build(name):
    """float32 (img1, img2) [n,1,h,w]; read-only: shared between tests"""
    _, h, w, n, _, _, dist = CASES[name]
    rng = np.random.RandomState(abs(hash_name(name)) % (2 ** 31))
    shape = (n, 1, h, w)
    if dist == 'rand1':
        a, b = rng.rand(*shape), rng.rand(*shape)
    elif dist == 'rand255':
        a, b = 255.0 * rng.rand(*shape), 255.0 * rng.rand(*shape)
    elif dist == 'blend':            # a fused image against one of its sources: values far from 0, strongly correlated
        a = 255.0 * rng.rand(*shape)
        b = np.clip(0.5 * (a + 255.0 * rng.rand(*shape)) + 4.0 * rng.randn(*shape), 0.0, 255.0)
    elif dist == 'flat':             # E[x^2] - mu^2 cancels five digits
        a, b = 200.0 + 0.5 * rng.rand(*shape), 200.0 + 0.5 * rng.rand(*shape)
    elif dist == 'anti':             # negative covariance everywhere: the level cs means are negative and the 1e-7 clamp engages
        a = 255.0 * rng.rand(*shape)
        b = 255.0 - a + rng.randn(*shape)
    elif dist == 'const':            # both images one constant per sample
        a = np.ones(shape) * (40.0 + 60.0 * np.arange(n).reshape(n, 1, 1, 1))
        b = a.copy()
    out = (np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32))
    for x in out:
        x.setflags(write=False)
    return out


def hash_name(name):
    v = 2166136261
    for ch in name.encode():
        v = ((v ^ ch) * 16777619) % (2 ** 32)
    return v


# ------------------------------------------------------------------ the definition
def taps(k, sigma=1.5):
    g = torch.tensor([exp(-(i - k // 2) ** 2 / (2.0 * sigma ** 2)) for i in range(k)], dtype=torch.float32)
    return g / g.sum()


def window(k, sigma=1.5):
    t = taps(k, sigma)
    return t[:, None] * t[None, :]          # float32 products


def _t(x, dtype):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.array(x))).to(dtype)


def _sym_pad(x, p):
    """numpy 'symmetric': the edge pixel IS repeated"""
    return torch.from_numpy(np.pad(x.numpy(), ((0, 0), (0, 0), (p, p), (p, p)), mode='symmetric'))


def maps(img1, img2, win_size=11, use_padding=False, dr=255.0, dtype=torch.float64, variant=None):
    """(ssim map, cs map) [n,1,Hm,Wm] in `dtype`"""
    a, b = (_t(x, dtype) for x in (img1, img2))
    h, w = a.shape[-2:]
    k = win_size if variant == 'no-shrink' else min(win_size, h, w)
    sigma = 0.15 * (k - 1) if (variant == 'loss-sigma' and k != 11) else 1.5
    win = window(k, sigma).to(dtype)[None, None]
    p = k // 2 if use_padding else 0

    def blur(x):
        if p:
            x = _sym_pad(x, p) if variant == 'symmetric' else F.pad(x, (p, p, p, p), 'reflect')
        return F.conv2d(x, win)
    mu1, mu2 = blur(a), blur(b)
    var1 = (blur(a * a) - mu1 * mu1).clamp(min=0)
    var2 = (blur(b * b) - mu2 * mu2).clamp(min=0)
    cov = blur(a * b) - mu1 * mu2
    if variant == 'cov-clamped':
        cov = cov.clamp(min=0)
    c1, c2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    v1, v2 = 2.0 * cov + c2, var1 + var2 + c2
    cs = v1 / v2
    ssim = (2.0 * mu1 * mu2 + c1) * v1 / ((mu1 * mu1 + mu2 * mu2 + c1) * v2)
    if variant == 'even-crop' and p and k % 2 == 0:
        ssim, cs = ssim[..., :h, :w], cs[..., :h, :w]
    return ssim, cs


def pool(x):
    """2 x 2 means of x reflect-padded to even extents"""
    ph, pw = x.shape[-2] % 2, x.shape[-1] % 2
    return F.avg_pool2d(F.pad(x, (0, pw, 0, ph), 'reflect'), 2, 2)


def ms_levels(img1, img2, win_size=11, use_padding=False, dr=255.0, dtype=torch.float64, variant=None):
    """[6, n] per-sample means in `dtype`: cs of levels 0-3, ssim of level 4, slot 5 = the level-0 ssim (the layout of mmif_metric_msssim)"""
    a, b = (_t(x, dtype) for x in (img1, img2))
    k0 = min(win_size, a.shape[-2], a.shape[-1])
    rows, first = [], None
    for lvl in range(5):
        if variant == 'frozen-window':
            ssim, cs = maps(a, b, k0, use_padding, dr, dtype, 'no-shrink')
        else:
            ssim, cs = maps(a, b, win_size, use_padding, dr, dtype)
        if lvl == 0:
            first = ssim.mean(dim=(1, 2, 3))
        rows.append((cs if (lvl < 4 or variant == 'last-cs') else ssim).mean(dim=(1, 2, 3)))
        if lvl < 4:
            a, b = pool(a), pool(b)
    return torch.stack(rows + [first])


def ms_value(levels):
    """prod_l max(v_l, 1e-7)^w_l over the first five rows of `levels` ([6, ...] or [5, ...]), in level order"""
    wts = torch.tensor(MS_WEIGHTS, dtype=torch.float32).to(levels.dtype)     # the reference holds its weights in float32
    v = levels[:5].clamp(min=1e-7)
    out = v[0] ** wts[0]
    for lvl in range(1, 5):
        out = out * v[lvl] ** wts[lvl]
    return out


# ------------------------------------------------------------------ references, yardsticks, distances
def _np(t):
    x = t.to(torch.float64).numpy()
    x.setflags(write=False)
    return x


def tol_of(ref, f32):
    """8 x the float32 evaluation's error (maximum over the array), floored at 2^-22 max(|ref|, 0.1)"""
    ref, f32 = np.asarray(ref, np.float64), np.asarray(f32, np.float64)
    return max(8.0 * float(np.abs(f32 - ref).max()), FLOOR * max(float(np.abs(ref).max()), 0.1))


@functools.lru_cache(maxsize=None)
def reference(name):
    """name -> dict of read-only float64 arrays with a 'tol' dict next to them.
    'ssim' cases: ssim, cs [n,1,Hm,Wm]; ssim_mean, cs_mean [n] (per sample); ssim_pooled, cs_pooled (whole batch)
    'ms' cases:   levels [6, n] (per sample), value [n] (per sample), pooled (the batch value: levels averaged over the samples first)"""
    kind, h, w, n, win, pad, dist = CASES[name]
    a, b = build(name)
    dr = data_range(dist)
    out = {}
    for bits, dt in (("64", torch.float64), ("32", torch.float32)):
        if kind == 'ssim':
            s, c = maps(a, b, win, pad, dr, dt)
            r = {"ssim": s, "cs": c, "ssim_mean": s.mean(dim=(1, 2, 3)), "cs_mean": c.mean(dim=(1, 2, 3)), "ssim_pooled": s.mean(), "cs_pooled": c.mean()}
        else:
            lv = ms_levels(a, b, win, pad, dr, dt)
            r = {"levels": lv, "value": ms_value(lv), "pooled": ms_value(lv.mean(dim=1))}
        out[bits] = {k: _np(v) for k, v in r.items()}
    ref = dict(out["64"])
    ref["tol"] = {k: tol_of(out["64"][k], out["32"][k]) for k in out["64"]}
    ref["err32"] = {k: float(np.abs(out["32"][k] - out["64"][k]).max()) for k in out["64"]}
    return ref


def variant_distance(name, variant):
    """how far the variant lies from the definition on this case, in tolerances of the compared output: element-wise over the maps where
    the shapes agree, else between the pooled means; None where the variant cannot be evaluated (e.g. a window larger than the image)
    or coincides by construction"""
    kind, h, w, n, win, pad, dist = CASES[name]
    a, b = build(name)
    dr = data_range(dist)
    ref = reference(name)
    try:
        if kind == 'ssim':
            s, c = maps(a, b, win, pad, dr, torch.float64, variant)
            if tuple(s.shape) == ref["ssim"].shape:
                return max(float(np.abs(_np(s) - ref["ssim"]).max()) / ref["tol"]["ssim"], float(np.abs(_np(c) - ref["cs"]).max()) / ref["tol"]["cs"])
            return max(abs(float(s.mean()) - float(ref["ssim_pooled"])) / ref["tol"]["ssim_pooled"],
                       abs(float(c.mean()) - float(ref["cs_pooled"])) / ref["tol"]["cs_pooled"])
        lv = ms_levels(a, b, win, pad, dr, torch.float64, variant)
        return max(float(np.abs(_np(lv) - ref["levels"]).max()) / ref["tol"]["levels"],
                   float(np.abs(_np(ms_value(lv)) - ref["value"]).max()) / ref["tol"]["value"])
    except (RuntimeError, ZeroDivisionError, ValueError):
        return None
