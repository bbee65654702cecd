"""Inputs of golden F19 (fusion-quality metrics): rebuilt from closed-form images and the stored uint8 crops, so the generator
(tests/golden/make_golden_metrics.py) and the tests see the same [B,1,H,W] float32 triples of 0..255 values."""
import json
import os

import numpy as np

from oracle.fusion_oracle import closed_form_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F19 = os.path.join(GOLDEN, "f19_metrics.npz")
F19_MANIFEST = os.path.join(GOLDEN, "f19_manifest.json")

# name -> (kind, (h, w)); 'int' = round(255 v), 'frac' = 255 v of the closed-form images
CASES = {
    "cf256_int": ("int", (256, 256)),
    "cf480x640_frac": ("frac", (480, 640)),
    "cf181x203_int": ("int", (181, 203)),
    "cf97x130_frac": ("frac", (97, 130)),
    "cf41x45_int": ("int", (41, 45)),
    "nat256x320": ("nat", (256, 320)),
    "natconst256x320": ("natconst", (256, 320)),
    "pooled2x256": ("pooled", (256, 256)),
    "allconst64": ("const", (64, 64)),
    "histedge64x80": ("edge", (64, 80)),
}


def fuse_int(a, b):
    """the fixed integer fusion rule of the fixtures: (3 max + min) // 4"""
    return np.floor((3.0 * np.maximum(a, b) + np.minimum(a, b)) / 4.0).astype(np.float32)


def _cf(h, w, frac):
    a = 255.0 * closed_form_image((1, 1, h, w), 0.3, np.float64)
    b = 255.0 * closed_form_image((1, 1, h, w), 1.7, np.float64)
    if frac:
        a, b = a.astype(np.float32), b.astype(np.float32)
        return a, b, (0.6 * a + 0.4 * b).astype(np.float32)
    a, b = np.round(a).astype(np.float32), np.round(b).astype(np.float32)
    return a, b, fuse_int(a, b)


def natural(store):
    """the stored 256x320 uint8 crops (vis, ir) as float32 [1,1,h,w]"""
    return store["nat_vis"].astype(np.float32)[None, None], store["nat_ir"].astype(np.float32)[None, None]


def build(name, store):
    """(img1, img2, imgf) float32 [B,1,H,W] of case `name`; `store` = the loaded f19 npz (for the natural crops)"""
    kind, (h, w) = CASES[name]
    if kind in ("int", "frac"):
        return _cf(h, w, kind == "frac")
    if kind in ("nat", "natconst"):
        a, b = natural(store)
        if kind == "natconst":
            a, b = a.copy(), b.copy()
            a[..., 40:120, 60:200] = 128.0
            b[..., 40:120, 60:200] = 128.0
        return a, b, fuse_int(a, b)
    if kind == "pooled":
        a0, b0, f0 = _cf(h, w, False)
        a1, b1 = natural(store)
        a1, b1 = a1[..., :h, :w], b1[..., :h, :w]
        return np.concatenate([a0, a1]), np.concatenate([b0, b1]), np.concatenate([f0, fuse_int(a1, b1)])
    if kind == "const":
        c = np.full((1, 1, h, w), 100.0, np.float32)
        return c, c.copy(), c.copy()
    if kind == "edge":   # histogram edges: exactly 256.0, below 0, above 256, one ulp below an integer
        a, b, f = _cf(h, w, True)
        a[..., 0, :10] = 256.0
        a[..., 1, :7] = -3.5
        a[..., 2, :5] = 300.0
        a[..., 3, :4] = np.nextafter(np.float32(17.0), np.float32(0.0))
        f[..., 4, :6] = 256.0
        f[..., 5, :3] = -0.25
        return a, b, f
    raise KeyError(name)


def load_f19():
    """flat dict of golden F19: 'nat_vis', 'nat_ir', '<case>|<metric>|<bits>' and '<case>|eval_<name>|<sample>|<bits>'"""
    raw = dict(np.load(F19))
    names = json.load(open(F19_MANIFEST))
    d = {"nat_vis": raw["nat_vis"], "nat_ir": raw["nat_ir"]}
    for case, m in names.items():
        for bits in ("64", "32"):
            for part in ("mirror", "eval"):
                key = f"{case}|{part}|{bits}"
                if key not in raw:
                    continue
                v = raw[key].astype(np.float64)
                if key + "|nan" in raw:
                    v = np.where(raw[key + "|nan"] != 0, np.nan, v)
                if part == "mirror":
                    d.update({f"{case}|{k}|{bits}": v[i] for i, k in enumerate(m["mirror"])})
                else:
                    d.update({f"{case}|eval_{k}|{s}|{bits}": v[s, i] for s in range(v.shape[0]) for i, k in enumerate(m["eval"])})
    return d


# ------------------------------------------------------------------ sweep inputs (tests/test_gpu_metric_sweep.py against oracle/metric_oracle.py)
# name -> what it exercises:
#   int     integer 0..255; f equals a on the left half, so gf == max(ga, gb) ties hit the Nabf / Labf masks
#   frac    fractional fp32 values
#   ramp    diamond ramps: Sobel responses in all four quadrants, exact zeros on the symmetry axes and the reflected borders
#   flat    zero patches in all three images, in f alone and in a alone (VIF's eps branches, Qabf's 0 / 0)
#   anti    f = 255 - a (negative CC, VIF's g < 0 branch)
#   same    a == b (g1 == g2 ties of the full VIF)
#   onebin  every pixel of all three images in bin 100 (entropies 0, normalised MI 0 / 0 = NaN)
#   edge    fractional values with histogram edge values scattered over all three images
SWEEP_DISTS = ('int', 'frac', 'ramp', 'flat', 'anti', 'same', 'onebin', 'edge')

_F = np.float32
# 256.0, -0.0, values in (255, 256), one ulp below integers, the joint histogram's 64-row slab edges, below 0 and above 256
EDGE_VALUES = np.array([256.0, -0.0, 0.0, 255.0, 255.5, np.nextafter(_F(256), _F(0)), np.nextafter(_F(1), _F(0)), np.nextafter(_F(17), _F(0)),
                        63.0, 64.0, np.nextafter(_F(64), _F(0)), 127.0, 128.0, np.nextafter(_F(128), _F(0)), 191.0, 192.0,
                        np.nextafter(_F(192), _F(0)), -3.5, np.nextafter(_F(256), _F(300)), 300.0], np.float32)
# one ulp below 0 (the smallest negative subnormal) goes to the histogram tests only: next to values of ~100 it is far below half
# an ulp, so the reference's fp64 Sobel sums keep or absorb it by their summation order, and a gradient component that is exactly
# 0 (the kernel's exact differences) comes out as -1.4e-45 there, which flips atan2 from +pi to -pi
TINY_NEG = np.nextafter(_F(0), _F(-1))


def _diamond(h, w, cy, cx, sy, sx):
    y, x = np.mgrid[:h, :w]
    d = (sy * np.abs(y - cy) + sx * np.abs(x - cx)).astype(np.float32)
    return d * np.float32(255.0 / max(float(d.max()), 1.0))


def sweep_triple(dist, h, w, n=1, seed=0):
    """(a, b, f) float32 [n,1,h,w] of distribution `dist` (SWEEP_DISTS); the same arguments always give the same arrays"""
    rng = np.random.default_rng([seed, h, w, n, SWEEP_DISTS.index(dist)])
    shp = (n, 1, h, w)
    frac = lambda: (rng.random(shp) * 255.0).astype(np.float32)
    ints = lambda: rng.integers(0, 256, shp).astype(np.float32)
    if dist == 'int':
        a, b = ints(), ints()
        f = fuse_int(a, b)
        f[..., :w // 2] = a[..., :w // 2]
        return a, b, f
    if dist == 'frac':
        a, b = frac(), frac()
        return a, b, (0.6 * a + 0.4 * b).astype(np.float32)
    if dist == 'ramp':
        a = _diamond(h, w, h // 2, w // 2, 3, 2)
        b = _diamond(h, w, h // 3, (2 * w) // 3, 1, 4)
        f = np.float32(255.0) - _diamond(h, w, (2 * h) // 3, w // 4, 2, 1)
        return tuple(np.broadcast_to(x, shp).copy() for x in (a, b, f))
    if dist == 'flat':
        a, b = frac(), frac()
        f = (0.5 * a + 0.5 * b).astype(np.float32)
        for x in (a, b, f):
            x[..., :h // 3, :w // 3] = 0.0
        f[..., h // 2:, w // 2:] = 0.0
        a[..., (2 * h) // 3:, :w // 3] = 0.0
        return a, b, f
    if dist == 'anti':
        a, b = frac(), ints()
        return a, b, np.float32(255.0) - a
    if dist == 'same':
        a = frac()
        return a, a.copy(), fuse_int(a, a)
    if dist == 'onebin':
        return tuple((100.0 + 0.99 * rng.random(shp)).astype(np.float32) for _ in range(3))
    if dist == 'edge':
        out = []
        for x in (frac(), frac(), frac()):
            m = rng.random(shp) < 0.25
            x[m] = rng.choice(EDGE_VALUES, int(m.sum()))
            out.append(x)
        return tuple(out)
    raise KeyError(dist)


def nonfinite_pair(h, w, n=1, seed=0):
    """(x, y) float32 [n,1,h,w]: the 'edge' values plus NaN, +-inf and TINY_NEG (only the exact-count histogram test takes these)"""
    x, _, y = sweep_triple('edge', h, w, n, seed)
    rng = np.random.default_rng([seed, h, w, n, 99])
    for t in (x, y):
        m = rng.random(t.shape) < 0.05
        t[m] = rng.choice(np.array([np.nan, np.inf, -np.inf, TINY_NEG], np.float32), int(m.sum()))
    return x, y


def mixed_batch(h, w, n, seed=0):
    """(a, b, f) float32 [n,1,h,w] whose sample i is SWEEP_DISTS[i % 8] (seed + i)"""
    parts = [sweep_triple(SWEEP_DISTS[i % len(SWEEP_DISTS)], h, w, 1, seed + i) for i in range(n)]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))
