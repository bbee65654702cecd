"""Inputs and case tables of the loss sweep (tests/test_gpu_loss_sweep.py against the fp64 functions of oracle/fusion_oracle.py) and of
golden F20 (tests/golden/make_golden_losses.py, tests/test_loss_oracle_cpu.py).  Every builder is seeded and closed-form: the same
arguments give the same float32 bits on every machine, so fixtures hold results only.

Shapes come from the constants of csrc/loss.hip and csrc/loss_modes.hip: WIN = 11 (a one-row SSIM map at h = 11), ST = 32 (SSIM map
tiles: a map edge of 32 / 33 at h = 42 / 43), LT = 16 (Sobel tiles), MT_ = 16 (mode kernels), FF_CAP = 12288 (LDS staging of the fused
finish kernel) and the 2048-block cap of pixel_loss_kernel (more than 524,288 pixels per call)."""
import os

import numpy as np

from oracle import fusion_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F20 = os.path.join(GOLDEN, "f20_loss_modes.npz")
F20_MANIFEST = os.path.join(GOLDEN, "f20_manifest.json")

# name -> what it exercises
#   cf       closed_form_image at three phases (what goldens F2 / F9 use)
#   rand     uniform [0, 1)
#   dyadic   multiples of 1/64 in [0, 1]: every difference and every Sobel sum is exact in fp32 and in fp64, so every sgn() decision
#            agrees by construction; imgf = max(img1, img2) on the top third, = img1 on the left third, so d == 0 ties are frequent
#   flatsrc  img1 constant (the 1e-4 variance clamp of 'w-ssim' / 'msw-ssim'; mag_1 == 0)
#   same     img2 = img1 (golden F2 case d)
#   anti     imgf = 1 - img1 on large-scale structure, img2 independent (negative covariance on every pyramid level: the 1e-7 clamp of
#            'ms-ssim' for the first source)
#   anti2    anti with img2 = img1 (both sources clamped)
#   wide     values in [-0.5, 1.5] (negative mu products)
#   r255     0..255 (data_range = 255)
DISTS = ('cf', 'rand', 'dyadic', 'flatsrc', 'same', 'anti', 'anti2', 'wide', 'r255')
FLOAT_DISTS = ('cf', 'rand', 'flatsrc', 'same', 'anti', 'wide')     # the float distributions of the pixel / Sobel sweep
TAU = 1e-5          # near-tie margin of the l1 exclusion rule (values in [0, 1]; x 255 for 'r255')
CAP = 1e-3          # largest share of gradient pixels the rule may leave out; none on images of fewer than 1000 pixels


def _structured(rng, shp, sign=1.0):
    """large-scale 2-D pattern (periods 47 x 61 px: alive after four 2 x 2 poolings) plus a little noise, in [0.05, 0.95], rounded to
    multiples of 1/4096: 1 - v and every Sobel sum of v are then exact in fp32, so mag(1 - v) == mag(v) is an exact tie in the kernel and
    in the oracle alike instead of a difference of rounding errors"""
    n, _, h, w = shp
    y, x = np.mgrid[:h, :w].astype(np.float64)
    ph = rng.random((n, 2)) * 2.0 * np.pi
    base = np.sin(2.0 * np.pi * y[None] / 47.0 + ph[:, 0, None, None]) * np.sin(2.0 * np.pi * x[None] / 61.0 + ph[:, 1, None, None])
    v = 0.5 + sign * 0.35 * base + 0.1 * (rng.random((n, h, w)) - 0.5)
    return (np.round(v * 4096.0) / 4096.0).reshape(shp).astype(np.float32)


def triple(dist, h, w, n=1, seed=0):
    """(img1, img2, imgf) float32 [n,1,h,w] of distribution `dist`"""
    rng = np.random.default_rng([seed, h, w, n, DISTS.index(dist)])
    shp = (n, 1, h, w)
    u = lambda: rng.random(shp).astype(np.float32)
    if dist == 'cf':
        return tuple(O.closed_form_image(shp, p + 0.61 * seed) for p in (0.3, 1.7, 2.9))
    if dist == 'rand':
        return u(), u(), u()
    if dist == 'dyadic':
        a, b, f = (rng.integers(0, 65, shp).astype(np.float32) / np.float32(64.0) for _ in range(3))
        f[..., :h // 3, :] = np.maximum(a, b)[..., :h // 3, :]
        f[..., :, :w // 3] = a[..., :, :w // 3]
        return a, b, f
    if dist == 'flatsrc':
        return np.full(shp, 0.4, np.float32), u(), u()
    if dist == 'same':
        a = u()
        return a, a.copy(), u()
    if dist in ('anti', 'anti2'):
        a = _structured(rng, shp)
        b = a.copy() if dist == 'anti2' else _structured(rng, shp)
        return a, b, (np.float32(1.0) - a).astype(np.float32)
    if dist == 'wide':
        return tuple((2.0 * rng.random(shp) - 0.5).astype(np.float32) for _ in range(3))
    if dist == 'r255':
        return tuple((255.0 * rng.random(shp)).astype(np.float32) for _ in range(3))
    raise KeyError(dist)


MIX = ('rand', 'cf', 'dyadic', 'flatsrc', 'same', 'anti', 'wide', 'anti2')


def mixed_batch(h, w, n, seed=0):
    """(img1, img2, imgf) float32 [n,1,h,w] whose sample i is MIX[i % 8] with seed + i"""
    parts = [triple(MIX[i % len(MIX)], h, w, 1, seed + i) for i in range(n)]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def f64(*xs):
    return tuple(np.asarray(x, np.float64) for x in xs)


# ------------------------------------------------------------------ shapes and case tables
SSIM_SHAPES = [(11, 11), (11, 300), (300, 11), (12, 13), (26, 27), (42, 42), (42, 43), (43, 42), (33, 47), (64, 80), (97, 130), (256, 256)]
SMALL_SHAPES = [(2, 2), (2, 17), (17, 2), (3, 3), (3, 5), (15, 16), (16, 17)]      # pixel / Sobel / TV only
MS_SHAPES = [(161, 161), (161, 176), (176, 177), (322, 161)]
BIG = (1024, 1224)
WIN_SIZES = (3, 5, 7, 9, 11)
RAGGED = [(33, 47), (97, 130)]        # the two shapes of the 16-combination fused sweep


def _rot(seq, i):
    return seq[i % len(seq)]


def pixgrad_cases():
    """(dist, h, w, n, seed) of the PixelLoss / GradLoss sweep: every shape on 'dyadic' (nothing left out) and on two float
    distributions; batches 1, 2, 3 in rotation; 1024x1224 once per kind.  With seed 0 the oracle has no near-tie on any
    image of fewer than 1000 pixels and stays within CAP on the others (asserted by tests/test_loss_oracle_cpu.py)."""
    out = []
    for i, (h, w) in enumerate(SMALL_SHAPES + SSIM_SHAPES):
        n = 1 + i % 3
        out.append(('dyadic', h, w, n, 0))
        for k in range(2):
            dist = _rot(FLOAT_DISTS, 2 * i + k)
            out.append((dist, h, w, 1 + (n + k) % 3, 0))
    out += [('dyadic', *BIG, 1, 0), ('rand', *BIG, 1, 0)]
    return out


def ssim_cases():
    """(dist, h, w, n, seed) of the SSIMLoss('ssim') sweep at data_range 1"""
    dists = ('rand', 'cf', 'wide', 'same', 'flatsrc', 'anti', 'dyadic')
    out = [(_rot(dists, i), h, w, 1 + i % 3, 0) for i, (h, w) in enumerate(SSIM_SHAPES)]
    return out + [('rand', *BIG, 1, 0)]


def mode_cases(mode):
    """(dist, h, w, n, seed) of the 'w-ssim' / 'msw-ssim' / 'ms-ssim' sweeps"""
    if mode == 'ms-ssim':
        dists = ('rand', 'cf', 'anti', 'wide')
        out = [(_rot(dists, i), h, w, 1 + (i + 1) % 3, 0) for i, (h, w) in enumerate(MS_SHAPES)]
        return out + [('anti', 161, 161, 3, 1), ('cf', *BIG, 1, 0)]
    dists = ('flatsrc', 'rand', 'cf', 'wide', 'same', 'anti')
    out = [(_rot(dists, i), h, w, 1 + (i + 2) % 3, 0) for i, (h, w) in enumerate(SSIM_SHAPES)]
    return out + [('rand', *BIG, 1, 0)]


def tv_cases():
    out = []
    for i, (h, w) in enumerate(SMALL_SHAPES + [(11, 300), (33, 47), (97, 130), (256, 256)]):
        out += [('dyadic', h, w, 1 + i % 3, 0), ('rand', h, w, 1 + (i + 1) % 3, 0)]
    return out + [('rand', *BIG, 1, 0)]


def fused_train_cases():
    """(dist, h, w, n, seed) of the fused call in the train configuration: every SSIM-bearing shape, then the two direct-read cases
    (partial lists longer than FF_CAP) and B = 16 at 40x56"""
    dists = ('rand', 'dyadic', 'cf', 'wide')
    out = [(_rot(dists, i), h, w, 1 + i % 3, 0) for i, (h, w) in enumerate(SSIM_SHAPES)]
    return out + [('rand', 256, 256, 64, 0), ('rand', *BIG, 3, 0), ('mixed', 40, 56, 16, 0)]


def build(case):
    dist, h, w, n, seed = case
    return mixed_batch(h, w, n, seed) if dist == 'mixed' else triple(dist, h, w, n, seed)


def case_id(case):
    dist, h, w, n, seed = case
    return f"{dist}-{n}x{h}x{w}" + (f"-s{seed}" if seed else "")


# ------------------------------------------------------------------ the exclusion rule of the l1 Sobel gradient
def _near(q, tau):
    """near-tie: within tau of a sign change without being an exact zero.  Exact zeros of the fp64 oracle are structural on these inputs
    (gy on the first and last row and gx on the first and last column, where the reflect padding pairs equal pixels; a constant image;
    img2 = img1) and the kernel forms every such quantity from the same paired differences, which are exact zeros in fp32 too:
    sgn(0) = 0 on both sides, nothing to leave out."""
    return (np.abs(q) < tau) & (q != 0)


def sobel_l1_excluded(img1, img2, imgf, mode, tau=TAU):
    """bool [n,1,h,w]: the gradient pixels of GradLoss('l1', mode) that may be left out of the comparison -- those within the 3 x 3
    neighbourhood (the reflect fold maps row -1 onto row 1, which the 3 x 3 window already holds) of a pixel where the ORACLE's own
    decision margin is below tau: |gx|, |gy| of the fused image, and |mag_f - max(mag_1, mag_2)| ('max') or |mag_f - mag_i| ('avg')."""
    i1, i2, f = f64(img1, img2, imgf)
    m1, m2 = O._sobel(i1)[0], O._sobel(i2)[0]
    mf, gx, gy = O._sobel(f)
    near = _near(gx, tau) | _near(gy, tau)
    if mode == 'max':
        near |= _near(mf - np.maximum(m1, m2), tau)
    else:
        near |= _near(mf - m1, tau) | _near(mf - m2, tau)
    p = np.pad(near, ((0, 0), (0, 0), (1, 1), (1, 1)))
    h, w = near.shape[2:]
    out = np.zeros_like(near)
    for dy in range(3):
        for dx in range(3):
            out |= p[:, :, dy:dy + h, dx:dx + w]
    return out


def check_cap(excl, what=""):
    """the share of left-out pixels of one case stays within CAP; none on images of fewer than 1000 pixels"""
    px = excl.shape[2] * excl.shape[3]
    share = float(excl.mean())
    assert share <= (CAP if px >= 1000 else 0.0), f"{what}: the l1 exclusion rule leaves out {share:.2e} of the pixels ({int(excl.sum())})"
    return share


# ------------------------------------------------------------------ golden F20 (the reference's modules in float64)
def _parse(case):
    """'<dist>-<n>x<h>x<w>[-s<seed>]' -> (dist, h, w, n, seed)"""
    parts = case.split('-')
    n, h, w = (int(v) for v in parts[1].split('x'))
    return parts[0], h, w, n, int(parts[2][1:]) if len(parts) > 2 else 0


def f20_inputs(kind, case):
    """float32 inputs of one F20 case: (img1, img2, imgf), or (x,) of shape [2,3,h,w] for TVLoss.  A distribution name ending in '255' is
    that distribution times 255 (exact for 'dyadic')."""
    dist, h, w, n, seed = _parse(case)
    scale = np.float32(255.0 if dist.endswith('255') else 1.0)
    base = dist[:-3] if dist.endswith('255') else dist
    if kind == 'tv':
        return ((triple(base, h, w, 6, seed)[2] * scale).reshape(2, 3, h, w),)
    return tuple((x * scale).astype(np.float32) for x in triple(base, h, w, n, seed))


def f20_entries():
    """name -> {kind, args, cases}: what tests/golden/make_golden_losses.py evaluates on the reference and tests/test_loss_oracle_cpu.py
    on the fp64 oracle"""
    pg_cases = [f"{d}-{s}" for d in ('cf', 'dyadic') for s in ('1x33x47', '3x11x29', '3x2x3', '3x3x2', '1x3x3')]
    e = {}
    for kind, wt in (('pixel', 0.3), ('grad', 0.7)):
        for norm in ('l1', 'l2'):
            for mode in ('avg', 'max'):
                e[f"{kind}_{norm}_{mode}"] = dict(kind=kind, args=dict(norm=norm, mode=mode, weight=wt), cases=pg_cases)
    for mode in ('ssim', 'w-ssim', 'msw-ssim'):
        e[f"{mode}_255"] = dict(kind='ssim', args=dict(mode=mode, data_range=255.0, weight=0.7), cases=['cf255-3x33x47', 'dyadic255-1x33x47', 'cf255-1x11x29'])
    e["ms-ssim_anti"] = dict(kind='ssim', args=dict(mode='ms-ssim', data_range=1.0, weight=0.7), cases=['anti-1x161x176'])
    for norm in ('l1', 'l2'):
        e[f"tv_{norm}"] = dict(kind='tv', args=dict(norm=norm, weight=0.3), cases=[f"{d}-{s}" for d in ('cf', 'dyadic') for s in ('6x11x29', '6x2x3', '6x3x2', '6x3x3')])
    return e


def oracle_f20(entry, arrays):
    """(loss, gradient) of one F20 entry from the oracle, in the dtype of `arrays`"""
    kind, a = entry["kind"], entry["args"]
    if kind == 'pixel':
        return O.pixel_loss(*arrays, a["weight"], a["mode"], True, a["norm"])
    if kind == 'grad':
        return O.grad_loss(*arrays, a["weight"], a["mode"], True, a["norm"])
    if kind == 'tv':
        return O.tv_loss(arrays[0], a["norm"], a["weight"])
    if a["mode"] == 'ssim':
        return O.ssim_loss(*arrays, a["weight"], a["data_range"])
    return O.ssim_mode_loss(*arrays, a["mode"], a["weight"], a["data_range"])
