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
