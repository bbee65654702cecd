"""The fp64 definition and the case table of the reflect-padded SSIM losses (SSIMLoss(mode, use_padding=True) and the SSIM / MS_SSIM /
MSW_SSIM modules with use_padding=True; reference core/loss.py:42-49: F.pad(img, k // 2, 'reflect') before every window pass), shared by
tests/test_ssim_pad_oracle_cpu.py and tests/test_gpu_ssim_pad_sweep.py.

The definition is composed from what oracle/fusion_oracle.py exports: reflect_pad the three images by p = k // 2, ssim_full_terms /
ssim_grad_weighted on the padded arrays (maps of h x w, counts h * w), reflect_pad_adjoint of the padded-domain gradient, the
_avg_pool_pad / _avg_pool_pad_bwd pyramid on the UNPADDED images, and the weights of ssim_mode_loss.  `pad` / `unpad` can be swapped
for the wrong-but-plausible variants of VARIANTS, which the CPU test shows to be far from the definition on every case.

Shapes come from the constants of csrc/loss_modes.hip (MT_ = 16 map / gradient tiles, p <= 5): one tile whose rows all fold (11, 12),
the tile edge (16, 17), two tiles whose border bands meet (21, 32, 33), interior tiles (64 x 80, 256 x 256), and for 'ms-ssim' the
smallest image (81: level 4 is 6 x 6, every row has two or three pre-images) up to 161 x 176.  Inputs: tests/loss_cases.py."""
import functools

import numpy as np

import loss_cases as LC
from oracle import fusion_oracle as O

MODES = ('ssim', 'w-ssim', 'ms-ssim', 'msw-ssim')          # index = the mode argument of mmif_ssim_loss_pad
WINDOWS = (11, 9, 7, 5, 3)
DISTS = ('rand', 'cf', 'anti', 'flatsrc', 'same', 'wide', 'dyadic', 'r255')     # 'r255' runs with data_range = 255
SHAPES = [(11, 11), (11, 12), (12, 11), (16, 16), (16, 17), (17, 16), (21, 37), (32, 33), (33, 47), (64, 80)]
MS_SHAPES = [(81, 81), (81, 96), (97, 83), (161, 176)]
WEIGHT = 0.7


def data_range(case):
    return 255.0 if case[0] == 'r255' else 1.0


def loss_cases(mode):
    """(dist, h, w, n, seed) of one SSIMLoss mode: every shape, distributions and batches 1..3 in rotation (offset per mode), 256 x 256
    once, one mixed batch"""
    k = MODES.index(mode)
    if mode == 'ms-ssim':
        out = []
        for i, (h, w) in enumerate(MS_SHAPES):
            out += [(DISTS[(2 * i + j) % 8], h, w, 1 + (i + j) % 3, 0) for j in range(2)]
        return out + [('mixed', 81, 83, 4, 0)]
    out = [(DISTS[(i + 3 * k) % 8], h, w, 1 + (i + k) % 3, 0) for i, (h, w) in enumerate(SHAPES)]
    return out + [(DISTS[k], 256, 256, 1, 0), ('mixed', 33, 47, 5, 0)]


def module_cases():
    """(win, dist, h, w, n, seed) of the SSIM module: every window at (k, k), (k, k + 1), (16, 17), (33, 47)"""
    out = []
    for a, k in enumerate(WINDOWS):
        for b, (h, w) in enumerate([(k, k), (k, k + 1), (16, 17), (33, 47)]):
            out.append((k, DISTS[(a + 2 * b) % 8], h, w, 1 + (a + b) % 3, 0))
    return out


def all_loss_cases():
    return [(m, c) for m in MODES for c in loss_cases(m)]


def case_id(case):
    return LC.case_id(case)


@functools.lru_cache(maxsize=None)
def build(case):
    """float32 (img1, img2, imgf); read-only: shared between tests"""
    trip = LC.build(case)
    for x in trip:
        x.setflags(write=False)
    return trip


# ------------------------------------------------------------------ padding variants: (pad, adjoint of pad)
def _index_pad(mode):
    """(pad, unpad) through an index map; `mode` as numpy.pad's.  'constant' (zeros) has no source pixel: its ring gets no gradient."""
    def idx(n, p):
        return np.pad(np.arange(n), (p, p), mode=mode) if mode != 'constant' else np.pad(np.arange(n), (p, p), constant_values=-1)

    def pad(x, p):
        return np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)), mode=mode)

    def unpad(g, p):
        h, w = g.shape[2] - 2 * p, g.shape[3] - 2 * p
        iy, ix = idx(h, p), idx(w, p)
        t = np.zeros(g.shape[:2] + (h, g.shape[3]), g.dtype)
        np.add.at(t, (slice(None), slice(None), iy[iy >= 0]), g[:, :, iy >= 0])
        out = np.zeros(g.shape[:2] + (h, w), g.dtype)
        np.add.at(out, (slice(None), slice(None), slice(None), ix[ix >= 0]), t[:, :, :, ix >= 0])
        return out
    return pad, unpad


def _crop(g, p):
    return g[:, :, p:g.shape[2] - p, p:g.shape[3] - p]


REFLECT = (O.reflect_pad, O.reflect_pad_adjoint)
VARIANTS = {
    'no-fold': (O.reflect_pad, _crop),                  # reflected reads, but the pad ring's gradient is dropped
    'symmetric': _index_pad('symmetric'),               # the edge pixel is repeated
    'replicate': _index_pad('edge'),
    'zero': _index_pad('constant'),
}


# ------------------------------------------------------------------ the definition
def _terms(x, f, k, dr, pad):
    p = k // 2
    return O.ssim_full_terms(pad(x, p), pad(f, p), O.create_window(k), dr)


def _grad(t, k, Wt, quantity, unpad):
    return unpad(O.ssim_grad_weighted(t, O.create_window(k), Wt, quantity), k // 2)


def pad_terms(img1, img2, win, dr=1.0):
    """per-sample means [n] of the padded ssim / cs / sigma maps of (img1, img2): what SSIM(win, dr, True, True) returns"""
    t = _terms(img1, img2, win, dr, O.reflect_pad)
    return {'ssim': t["S"].mean(axis=(1, 2, 3)), 'cs': t["cs"].mean(axis=(1, 2, 3)), 'sigma': t["sigma"].mean(axis=(1, 2, 3))}


def pad_loss(img1, img2, imgf, mode, weight=1.0, dr=1.0, need_grad=True, padding=REFLECT):
    """SSIMLoss(mode, use_padding=True) core/loss.py:252-284 in the arrays' dtype: (loss, dloss/dimgf)"""
    pad, unpad = padding
    N, _, H, W = imgf.shape
    dt = imgf.dtype
    eps = dt.type(1e-7)
    cnt = H * W
    grad = np.zeros_like(imgf) if need_grad else None
    if mode in ('ssim', 'w-ssim'):
        t1, t2 = _terms(img1, imgf, 11, dr, pad), _terms(img2, imgf, 11, dr, pad)
        if mode == 'ssim':
            gamma = np.full(N, 0.5, dt)
        else:
            sg1, sg2 = t1["sigma"].mean(axis=(1, 2, 3)), t2["sigma"].mean(axis=(1, 2, 3))
            gamma = sg1 / np.maximum(sg1 + sg2, eps)
        s1, s2 = t1["S"].mean(axis=(1, 2, 3)), t2["S"].mean(axis=(1, 2, 3))
        val = (gamma * s1).mean() + ((1.0 - gamma) * s2).mean()
        if need_grad:
            g4 = gamma.reshape(N, 1, 1, 1)
            grad = _grad(t1, 11, -weight * g4 / (N * cnt) * np.ones_like(t1["S"]), "ssim", unpad) + \
                _grad(t2, 11, -weight * (1.0 - g4) / (N * cnt) * np.ones_like(t2["S"]), "ssim", unpad)
        return weight * (1.0 - val), grad
    if mode == 'msw-ssim':
        val = 0.0
        for k in WINDOWS:
            t1, t2 = _terms(img1, imgf, k, dr, pad), _terms(img2, imgf, k, dr, pad)
            gamma = t1["sigma"] / np.maximum(t1["sigma"] + t2["sigma"], eps)
            val = val + (gamma * t1["S"]).mean() + ((1.0 - gamma) * t2["S"]).mean()
            if need_grad:
                grad = grad + _grad(t1, k, -weight * gamma / (len(WINDOWS) * N * cnt), "ssim", unpad) + \
                    _grad(t2, k, -weight * (1.0 - gamma) / (len(WINDOWS) * N * cnt), "ssim", unpad)
        return weight * (1.0 - val / len(WINDOWS)), grad
    if mode == 'ms-ssim':
        msw = O.MS_WEIGHTS.astype(dt)
        total = 0.0
        for src in (img1, img2):
            x, f = src, imgf
            terms, shapes, vals = [], [], []
            for lvl in range(5):
                t = _terms(x, f, 11, dr, pad)
                terms.append(t)
                shapes.append(f.shape[2:])
                vals.append((t["cs"] if lvl < 4 else t["S"]).mean(axis=(1, 2, 3)))
                if lvl < 4:
                    x, f = O._avg_pool_pad(x), O._avg_pool_pad(f)
            raw = np.stack(vals)
            v = np.maximum(raw, eps)
            ms = np.prod(v ** msw[:, None], axis=0)
            total = total + ms.mean()
            if need_grad:
                g_next = None
                for lvl in range(4, -1, -1):
                    t = terms[lvl]
                    nmap = shapes[lvl][0] * shapes[lvl][1]
                    dv = np.where(raw[lvl] > eps, -weight * 0.5 / N * msw[lvl] * ms / v[lvl], 0.0).astype(dt)
                    g = _grad(t, 11, (dv / nmap).reshape(N, 1, 1, 1) * np.ones_like(t["S"]), "cs" if lvl < 4 else "ssim", unpad)
                    if g_next is not None:
                        g = g + O._avg_pool_pad_bwd(g_next, *shapes[lvl])
                    g_next = g
                grad = grad + g_next
        return weight * (1.0 - 0.5 * total), grad
    raise ValueError("only supported ['ssim', 'w-ssim', 'ms-ssim', 'msw-ssim'] mode")


@functools.lru_cache(maxsize=None)
def reference(mode, case):
    """(loss, gradient) of the definition on float64 copies of build(case), weight WEIGHT; computed once per session"""
    loss, grad = pad_loss(*LC.f64(*build(case)), mode, WEIGHT, data_range(case))
    grad.setflags(write=False)
    return float(loss), grad
