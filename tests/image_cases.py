"""Cases and fp64 definitions for the image-side layers (csrc/conv_image.hip, csrc/image_bwd.hip): the Cin == 1 first encoder conv and the
Cout == 1 last decoder conv, seven entry points, nine kernels; and the library's own answer to "which kernel does this call launch, on what
grid" (mmif_conv2d_image_plan, csrc/image_route.hpp).  No GPU needed: tests/test_image_oracle_cpu.py pins the definitions to torch's float64
autograd and the case list to the plan; tests/test_gpu_image_sweep.py runs every case on the device.

The definitions (all float64, on oracle.fusion_oracle; conventions of tests/conv_cases.py):

* image_in_fwd     y[:, :cout] = relu?(b + corr(reflect_pad(img, k//2), w)); lanes cout .. 8 cb - 1 of the view are written as ZERO
* image_out_fwd    img = relu?(b + sum_{c < cin} corr(reflect_pad(x_c), w_c)); lanes >= cin of the view never reach the result
* image_out_dgrad  on the whole stored domain of gx (halo >= k//2): the full scatter of g0 = gimg [y_img > 0] (zero outside the image) with
                   the flipped kernel; block i of accum_bits ADDS the old contents first; block i of mask_bits THEN multiplies by [x > 0],
                   taken at the reflected source for ring positions (a one-pixel axis has no other source than its pixel); lanes >= cin
                   hold the (masked) old value or zero
* image_in_wgrad / image_out_wgrad   dw, db of the definitions above; accumulate adds onto the previous contents; image_in_wgrad's gradient
                   is halo 0, halo 1 folded (zero ring) or halo 1 unfolded (k = 3: the padded-domain gradient, folded while loading)
* image_out_bwd    image_out_wgrad plus reflect_pad_adjoint(dgrad, padded) [x > 0] in the interior of gx; the ring stays as it was (zero)

Two data families per case.  'exact': small integers -- every partial sum in any order is an exactly representable integer, so the result
does not depend on summation order, tile walk or FMA grouping, and the comparison is BIT EQUALITY with the float64 result cast to the output
type; exact_condition() asserts what makes this true (sum |terms| < 2^24 for fp32 outputs, <= 256 for bf16 outputs) from the case's own data.
'real': seeded normal / uniform data, bf16-rounded where it enters a bf16 tensor, compared with the float64 definition on those operands
under the DERIVED per-element bound of bound(): with K terms summed in fp32 in any order, each of the K - 1 additions (an FMA rounds once)
errs by at most 2^-24 of a partial sum that sum |terms| bounds, so delta = K 2^-24 sum |terms|; fp32 outputs add the final 2^-24 |ref| of a
last rounding, bf16 outputs half a bf16 spacing at |ref| + delta.  Nothing here is calibrated on a device.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np
import torch

from conv_cases import FEW_BITS, cdiv
from oracle import fusion_oracle as O

POISON = 1.0e30          # unused channel lanes of 12- / 24-channel operands: large, finite, both signs; must not reach any output
FILL = 7.0               # the other blocks of a wider buffer
ENTRIES = ("in_fwd", "in_wgrad", "out_fwd", "out_dgrad", "out_wgrad", "out_bwd")

# the nine kernels, by the names the plan gives them, per dtype they exist for (tests/test_image_oracle_cpu.py: every one is reached)
REQUIRED_NAMES = ([f"{e}<{t},{k}>" for e in ("image_in_fwd", "image_in_wgrad", "image_out_fwd", "image_out_dgrad", "image_out_wgrad")
                   for t in ("bf16", "f32") for k in (1, 3)]
                  + ["image_out_fwd16", "image_out_fwd_tiled<f32>", "image_out_bwd16"])


def plan(entry, dtype, c, k, cb, n, h, w, halo=0):
    """what the library launches for the call (mmif.tensor.image_plan: name, G, slices, tiles), None where it would refuse"""
    from mmif import _lib as L
    from mmif import tensor as T
    return T.image_plan(entry, L.BF16 if dtype == "bf16" else L.F32, c, k, cb, n, h, w, halo)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    entry: str                  # in_fwd | in_wgrad | out_fwd | out_dgrad | out_wgrad | out_bwd
    family: str                 # exact | real
    dtype: str                  # bf16 | f32: the blocked tensors'
    c: int                      # cout of the image_in entries, cin of the image_out ones
    k: int
    n: int
    h: int
    w: int
    relu: bool = False          # forward: ReLU at the output; backward of image_out: y_img given
    bias: bool = True           # forward: bias given (else NULL)
    view: tuple = (0, 0)        # (block offset, blocks of the buffer) of the view; (0, 0): the exact tensor
    halo: int = 0               # out_dgrad: of gx; in_wgrad: of the gradient
    folded: bool = True         # in_wgrad, halo 1: zero ring + FOLDED flag; False: a padded-domain gradient
    bits: tuple = ((0, 0),)     # out_dgrad: (mask_bits, accum_bits) pairs run on the one set of operands
    accumulate: tuple = (0,)    # weight gradients: accumulate flags run
    note: str = ""

    @property
    def cb(self):
        return cdiv(self.c, 8)

    @property
    def cb_off(self):
        return self.view[0]

    @property
    def cb_total(self):
        return self.view[1] or self.cb

    @property
    def id(self):
        s = f"{self.entry}-{self.family}-{self.dtype}-c{self.c}k{self.k}-{self.n}x{self.h}x{self.w}"
        s += ("-relu" if self.relu else "") + ("" if self.bias else "-nobias")
        if self.view != (0, 0):
            s += f"-view{self.view[0]}of{self.view[1]}"
        if self.entry in ("out_dgrad", "in_wgrad"):
            s += f"-h{self.halo}" + ("" if self.folded or not self.halo else "raw")
        return s + (("-" + self.note) if self.note else "")

    def plan(self):
        return plan(self.entry, self.dtype, self.c, self.k, self.cb, self.n, self.h, self.w, self.halo)


MIN3 = [(1, 2, 2), (1, 2, 9), (1, 9, 2)]                                  # every row / column is a reflect source
MIN1 = [(1, 1, 1), (1, 1, 5)]
BWD_MIN = [(1, 4, 4), (1, 4, 5), (2, 5, 4)]                               # rows 1 and h - 2 are distinct fold targets from 4 on
T16 = [(1, 16, 16), (1, 14, 14), (2, 17, 33), (1, 15, 31), (1, 37, 53)]   # 16 x 16 tile seams (dgrad tiles the STORED domain h + 2)
T8X32 = [(1, 8, 32), (1, 9, 33), (2, 7, 31), (1, 16, 64), (1, 17, 65), (1, 23, 70)]
WALK = [(n, 8, 32) for n in (1, 7, 8, 9, 13, 17)]                         # n tiles of one image each: plain walk at 7, ragged XCD bands at 9, 13, 17
LONG = (31, 472, 33)                                                      # 3658 tiles of 8 x 32, 483 k pixels
CHANNELS = (8, 12, 24, 64)                                                # besides 16: one block, a half-filled pair, 1.5 pairs, four pairs
VIEWS = ((1, 4), (8, 16))
SWEEP3 = [(2, 17, 33), (1, 2, 9)]                                         # the shapes of the channel / view / flag sweeps
SWEEP1 = [(2, 17, 33), (1, 1, 5)]


def _cases():
    cs = []
    for fam in ("exact", "real"):
        for dt in ("bf16", "f32"):
            def add(entry, c, k, shape, **kw):
                cs.append(Case(entry, fam, dt, c, k, *shape, **kw))
            # ---- image_in_fwd
            for s in MIN3 + T16:
                add("in_fwd", 16, 3, s, relu=True)
            for s in MIN1 + T16[1:3]:
                add("in_fwd", 16, 1, s, relu=True)
            for relu, bias in ((0, 1), (0, 0), (1, 0)):
                add("in_fwd", 16, 3, T16[3], relu=bool(relu), bias=bool(bias), note="flags")
            for i, c in enumerate(CHANNELS):
                for k, shapes in ((3, SWEEP3), (1, SWEEP1)):
                    for j, s in enumerate(shapes):
                        add("in_fwd", c, k, s, relu=bool((i + j) & 1), bias=bool((i + j + k) & 2) or j == 0)
            for v in VIEWS:
                for c in (16, 12):
                    add("in_fwd", c, 3, SWEEP3[0], relu=True, view=v)
                add("in_fwd", 16, 1, SWEEP1[0], view=v)
            # ---- image_in_wgrad: halo 0 / halo 1 folded / halo 1 unfolded (k = 3)
            states = ((0, True), (1, True), (1, False))
            for s in MIN3 + [T16[0], T16[1], T16[2], T16[4]]:
                for halo, folded in states:
                    add("in_wgrad", 16, 3, s, halo=halo, folded=folded, accumulate=(0, 1))
            for s in MIN1 + [T16[2]]:
                for halo, folded in states[:2]:
                    add("in_wgrad", 16, 1, s, halo=halo, folded=folded, accumulate=(0, 1))
            for i, c in enumerate(CHANNELS):
                for j, s in enumerate(SWEEP3):
                    halo, folded = states[(i + j) % 3]
                    add("in_wgrad", c, 3, s, halo=halo, folded=folded, accumulate=(0, 1))
                add("in_wgrad", c, 1, SWEEP1[0], halo=i & 1, accumulate=(0, 1))
            for v in VIEWS:
                for (halo, folded), c in zip(states, (16, 12, 16)):
                    add("in_wgrad", c, 3, SWEEP3[0], halo=halo, folded=folded, accumulate=(0, 1), view=v)
            # ---- image_out_fwd: 16 channels 3x3 = the persistent kernel (bf16) / the tiled kernel (fp32); everything else the generic one
            for s in MIN3 + T16 + T8X32 + WALK[1:]:      # (WALK[0] is T8X32[0])
                add("out_fwd", 16, 3, s)
            for s in MIN1 + T16[:3]:
                add("out_fwd", 16, 1, s)
            for relu, bias in ((1, 1), (0, 0), (1, 0)):
                add("out_fwd", 16, 3, T8X32[1], relu=bool(relu), bias=bool(bias), note="flags")
            for i, c in enumerate(CHANNELS):
                for k, shapes in ((3, SWEEP3 + [T16[4]]), (1, SWEEP1)):
                    for j, s in enumerate(shapes):
                        add("out_fwd", c, k, s, relu=bool((i + j) & 1), bias=bool((i + j + k) & 2) or j == 0)
            for v in VIEWS:
                for c in (16, 12):
                    add("out_fwd", c, 3, SWEEP3[0], relu=True, view=v)
                add("out_fwd", 16, 1, SWEEP1[0], view=v)
            # ---- image_out_dgrad: the stored domain of gx, every few-bits combination, y_img given / NULL
            for s in MIN3 + T16:
                add("out_dgrad", 16, 3, s, halo=1, bits=FEW_BITS, relu=True)
            add("out_dgrad", 16, 3, T16[1], halo=1, bits=FEW_BITS, relu=False)
            for s in MIN1 + T16[:3]:
                for halo in (0, 1):
                    add("out_dgrad", 16, 1, s, halo=halo, bits=FEW_BITS, relu=bool(halo))
            for i, c in enumerate(CHANNELS):
                for j, s in enumerate(SWEEP3):
                    add("out_dgrad", c, 3, s, halo=1, bits=FEW_BITS, relu=bool((i + j) & 1))
                add("out_dgrad", c, 1, SWEEP1[0], halo=i & 1, bits=FEW_BITS, relu=bool(i & 2))
            for v in VIEWS:
                for c in (16, 12):
                    add("out_dgrad", c, 3, SWEEP3[0], halo=1, bits=FEW_BITS, relu=True, view=v)
                add("out_dgrad", 16, 1, SWEEP1[0], halo=0, bits=FEW_BITS, view=v)
            # ---- image_out_wgrad
            for s in MIN3 + [T16[0], T16[1], T16[2], T16[4]]:
                add("out_wgrad", 16, 3, s, relu=True, accumulate=(0, 1))
            add("out_wgrad", 16, 3, T16[3], relu=False, accumulate=(0, 1))
            for s in MIN1 + [T16[2]]:
                add("out_wgrad", 16, 1, s, relu=True, accumulate=(0, 1))
            for i, c in enumerate(CHANNELS):
                for j, s in enumerate(SWEEP3):
                    add("out_wgrad", c, 3, s, relu=bool((i + j) & 1), accumulate=(0, 1))
                add("out_wgrad", c, 1, SWEEP1[0], relu=bool(i & 1), accumulate=(0, 1))
            for v in VIEWS:
                for c in (16, 12):
                    add("out_wgrad", c, 3, SWEEP3[0], relu=True, accumulate=(0, 1), view=v)
            # ---- image_out_bwd (bf16, 16 channels, 3x3, h, w >= 4)
            if dt == "bf16":
                for i, s in enumerate(BWD_MIN + T8X32 + WALK[1:] + [T16[2], T16[4]]):
                    add("out_bwd", 16, 3, s, relu=bool(i & 1), accumulate=(0, 1))
                for v in VIEWS:
                    add("out_bwd", 16, 3, T8X32[1], relu=True, accumulate=(0, 1), view=v)
    # ---- the long walk, exact family, bf16, once per entry that has a persistent or grid-stride kernel: a bwd16 block owns 7 or 8 tiles (the
    # prefetch ring wraps twice), an fwd16 block 3 or 4, both weight-gradient kernels stride (483 k pixels over 512 x 256 threads)
    cs.append(Case("out_fwd", "exact", "bf16", 16, 3, *LONG, note="long"))
    cs.append(Case("out_bwd", "exact", "bf16", 16, 3, *LONG, relu=True, note="long"))
    cs.append(Case("out_wgrad", "exact", "bf16", 16, 3, *LONG, relu=True, note="long"))
    cs.append(Case("in_wgrad", "exact", "bf16", 16, 3, *LONG, halo=1, folded=False, note="long"))
    return cs


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"
# the fused backward against the three launches it replaces, bit for bit (exact family)
BWD_VS_THREE = [c for c in CASES if c.entry == "out_bwd" and c.family == "exact" and c.view == (0, 0)]


# ------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------
def rnd(a, dtype):
    """the values a tensor of the case's dtype holds, as float64"""
    a = np.asarray(a, np.float32)
    return (O.bf16_round(a) if dtype == "bf16" else a).astype(np.float64)


@dataclass
class Operands:
    img: np.ndarray = None       # in_*: the fp32 image [n, h, w]
    x: np.ndarray = None         # out_*: activations, every lane of the view [n, 8 cb, h, w] (lanes >= c: POISON)
    w: np.ndarray = None         # fp32 weights [cout, 1, k, k] / [1, cin, k, k]
    b: np.ndarray = None         # or None
    gp: np.ndarray = None        # in_wgrad: the stored gradient, every lane [n, 8 cb, h + 2 halo, w + 2 halo]
    gimg: np.ndarray = None      # out_*: dL/d(output image) [n, h, w]
    yimg: np.ndarray = None      # the layer's output where it has a ReLU, else None
    old: np.ndarray = None       # out_dgrad: previous contents of gx, every lane, stored extent
    dw_old: np.ndarray = None
    db_old: np.ndarray = None


_OPS = {}


def _keep(d, key, val, n=2):
    d[key] = val
    while len(d) > n:
        d.pop(next(iter(d)))
    return val


def _poison(a, c, rng):
    if a.shape[1] > c:
        a[:, c:] = POISON * rng.choice([-1.0, 1.0], size=a[:, c:].shape)
    return a


def operands(c: Case) -> Operands:
    key = (c.entry, c.family, c.dtype, c.c, c.k, c.n, c.h, c.w, c.relu, c.bias, c.halo, c.folded)
    if key in _OPS:
        return _OPS[key]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    ex = c.family == "exact"
    n, h, w, k, C = c.n, c.h, c.w, c.k, c.cb * 8
    o = Operands()

    def ints(lo, hi, shape):
        return rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    if c.entry.startswith("in_"):
        o.img = ints(0, 3, (n, h, w)) if ex else rng.random((n, h, w)).astype(np.float32).astype(np.float64)
        o.w = ints(-3, 3, (c.c, 1, k, k)) if ex else rnd(rng.standard_normal((c.c, 1, k, k)) * 0.3, "f32")
        o.b = (ints(-4, 4, (c.c,)) if ex else rnd(rng.standard_normal(c.c), "f32")) if c.bias else None
        hg = c.halo
        gp = ints(-2, 2, (n, C, h + 2 * hg, w + 2 * hg)) if ex else rnd(rng.standard_normal((n, C, h + 2 * hg, w + 2 * hg)), c.dtype)
        if hg and c.folded:
            gp = np.pad(gp[:, :, 1:-1, 1:-1], ((0, 0), (0, 0), (1, 1), (1, 1)))
        if n * h * w < 16:      # a tiny map random draws could blank: one pixel and its gradient let through
            o.img.flat[0] = max(o.img.flat[0], 1.0)
            gp[0, 0, hg, hg] = gp[0, 0, hg, hg] or 1.0
        o.gp = rnd(_poison(gp, c.c, rng), c.dtype)
        o.dw_old = ints(-8, 8, o.w.shape) if ex else rnd(rng.standard_normal(o.w.shape) * np.sqrt(n * h * w), "f32")
        o.db_old = ints(-8, 8, (c.c,)) if ex else rnd(rng.standard_normal(c.c) * np.sqrt(n * h * w), "f32")
    else:
        if ex:
            x = ints(1, 3, (n, C, h, w)) * (rng.random((n, C, h, w)) > 0.4)
        else:
            x = rnd(rng.standard_normal((n, C, h, w)), c.dtype) * (rng.random((n, C, h, w)) > 0.4)
        x[(x == 0) & (rng.random(x.shape) < 0.25)] = -0.0            # some of the zeros negative: [x > 0] is false, the products vanish
        o.x = rnd(_poison(x, c.c, rng), c.dtype)
        o.w = ints(-3, 3, (1, c.c, k, k)) if ex else rnd(rng.standard_normal((1, c.c, k, k)) * 0.2, "f32")
        o.b = (ints(-4, 4, (1,)) if ex else rnd(rng.standard_normal(1), "f32")) if c.bias else None
        o.gimg = ints(-2, 2, (n, h, w)) if ex else rnd(rng.standard_normal((n, h, w)), "f32")
        if c.relu:      # the layer's output as the backward sees it: negatives and exact zeros under the > 0 mask
            o.yimg = ints(-1, 2, (n, h, w)) if ex else rnd(rng.standard_normal((n, h, w)) * (rng.random((n, h, w)) > 0.2), "f32")
            if not (o.gimg * (o.yimg > 0)).any():      # a tiny map the mask would blank: let one pixel through
                o.yimg.flat[0], o.gimg.flat[0] = 1.0, 2.0
        hx = c.halo
        if c.entry == "out_dgrad":
            old = ints(-8, 8, (n, C, h + 2 * hx, w + 2 * hx)) if ex else rng.standard_normal((n, C, h + 2 * hx, w + 2 * hx))
            o.old = rnd(old, c.dtype)
        o.dw_old = ints(-8, 8, o.w.shape) if ex else rnd(rng.standard_normal(o.w.shape) * np.sqrt(n * h * w), "f32")
        o.db_old = ints(-8, 8, (1,)) if ex else rnd(rng.standard_normal(1) * np.sqrt(n * h * w), "f32")
        if c.entry == "out_fwd" and c.relu and conv_fwd(o.x[:, :c.c], o.w, o.b).max() <= 0:      # a tiny map the ReLU would blank: the other sign
            o.w, o.b = -o.w, (None if o.b is None else -o.b)
    return _keep(_OPS, key, o)


# ------------------------------------------------------------------------------------------------------------------------------
# definitions.  Small cases run oracle.fusion_oracle's numpy loops; from BIG elements on the same three operators run as one float64
# torch.nn.functional.conv2d each (exact for the integers of the long-walk case; tests/test_image_oracle_cpu.py holds both to autograd)
# ------------------------------------------------------------------------------------------------------------------------------
BIG = 1 << 20


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def reflect_pad(x, p):
    """O.reflect_pad with one-pixel axes allowed: their only source is the pixel itself (the kernels clamp the reflected index)"""
    if p == 0:
        return x
    iy = np.clip(O.reflect_index(np.arange(-p, x.shape[2] + p), x.shape[2]), 0, x.shape[2] - 1)
    ix = np.clip(O.reflect_index(np.arange(-p, x.shape[3] + p), x.shape[3]), 0, x.shape[3] - 1)
    return x[:, :, iy][:, :, :, ix]


def conv_fwd(x, w, b, big=None):
    """b + corr(reflect_pad(x), w), no activation"""
    if (x.size >= BIG) if big is None else big:
        xp = _t(reflect_pad(x, w.shape[2] // 2))
        return torch.nn.functional.conv2d(xp, _t(w), None if b is None else _t(b)).numpy()
    return O.conv2d_reflect_fwd(x, w, b, relu=False)


def conv_wgrad(x, w_shape, g, big=None):
    """dw[o, c, u, v] = sum g xpad, db[o] = sum g"""
    k = w_shape[2]
    if (x.size >= BIG) if big is None else big:
        xp, gt = _t(reflect_pad(x, k // 2)), _t(g)
        # the weight gradient as a correlation of the padded input with the gradient: channels <-> batch
        dw = torch.nn.functional.conv2d(xp.transpose(0, 1), gt.transpose(0, 1)).transpose(0, 1)
        return dw.numpy(), g.sum(axis=(0, 2, 3))
    _, gw, gb = O.conv2d_reflect_bwd(x, np.zeros(w_shape), None, g, relu=False, need_gx=False)
    return gw, gb


def conv_dgrad_padded(g, w, big=None):
    """the full scatter of g with w: [n, cin, h + 2p, w + 2p]"""
    p = w.shape[2] // 2
    if (g.size * w.shape[1] >= BIG) if big is None else big:
        gz = torch.nn.functional.pad(_t(g), (2 * p,) * 4)
        return torch.nn.functional.conv2d(gz, _t(w).flip(2, 3).transpose(0, 1)).numpy()
    return O.conv2d_reflect_dgrad_padded(g, w)


def g0_of(o: Operands):
    """the gradient at the layer's pre-activation: gimg [y_img > 0]"""
    g = o.gimg if o.yimg is None else o.gimg * (o.yimg > 0)
    return g[:, None] + 0.0


def def_in_fwd(c: Case):
    """(y on every lane of the view [n, 8 cb, h, w], S = the same sum on |operands|, K terms)"""
    o = operands(c)
    y = np.zeros((c.n, c.cb * 8, c.h, c.w))
    S = np.zeros_like(y)
    y[:, :c.c] = conv_fwd(o.img[:, None], o.w, o.b)
    S[:, :c.c] = conv_fwd(np.abs(o.img[:, None]), np.abs(o.w), None if o.b is None else np.abs(o.b))
    if c.relu:
        y = np.maximum(y, 0)
    return y, S, c.k * c.k + 1


def def_out_fwd(c: Case):
    """(img [n, h, w], S, K)"""
    o = operands(c)
    y = conv_fwd(o.x[:, :c.c], o.w, o.b)[:, 0]
    S = conv_fwd(np.abs(o.x[:, :c.c]), np.abs(o.w), None if o.b is None else np.abs(o.b))[:, 0]
    return (np.maximum(y, 0) if c.relu else y), S, c.c * c.k * c.k + 1


def _embed(a, halo, p):
    """a padded-domain array [.., h + 2p, w + 2p] inside the stored domain of halo >= p (zero beyond: nothing is scattered there)"""
    d = halo - p
    return np.pad(a, ((0, 0), (0, 0), (d, d), (d, d))) if d else a


def apply_bits(val, old, x, mask_bits, accum_bits):
    """[n, C, ., .] arrays: block i of accum_bits ADDS old FIRST, block i of mask_bits THEN multiplies by [x > 0]"""
    C = val.shape[1]
    am = np.array([(accum_bits >> (ch // 8)) & 1 for ch in range(C)], np.float64)[None, :, None, None]
    mm = np.array([(mask_bits >> (ch // 8)) & 1 for ch in range(C)], np.float64)[None, :, None, None]
    out = val + am * old
    if mask_bits:
        out = out * (1 - mm + mm * (x > 0))
    return out + 0.0


def def_out_dgrad(c: Case, mask_bits, accum_bits):
    """(gx on every lane of the view and the whole stored domain, S, K)"""
    o = operands(c)
    p, C = c.k // 2, c.cb * 8
    g0 = g0_of(o)
    ref = np.zeros((c.n, C, c.h + 2 * c.halo, c.w + 2 * c.halo))
    S = np.zeros_like(ref)
    ref[:, :c.c] = _embed(conv_dgrad_padded(g0, o.w), c.halo, p)
    S[:, :c.c] = _embed(conv_dgrad_padded(np.abs(g0), np.abs(o.w)), c.halo, p)
    xs = reflect_pad(o.x, c.halo)                            # the mask's source: reflected on the ring
    return apply_bits(ref, o.old, xs, mask_bits, accum_bits), apply_bits(S, np.abs(o.old), None, 0, accum_bits), c.k * c.k + 1


def def_out_wgrad(c: Case, accumulate):
    """(dw, db, Sw, Sb, K)"""
    o = operands(c)
    g0 = g0_of(o)
    dw, db = conv_wgrad(o.x[:, :c.c], o.w.shape, g0)
    Sw, Sb = conv_wgrad(np.abs(o.x[:, :c.c]), o.w.shape, np.abs(g0))
    K = c.n * c.h * c.w
    if accumulate:
        dw, db, Sw, Sb, K = dw + o.dw_old, db + o.db_old, Sw + np.abs(o.dw_old), Sb + np.abs(o.db_old), K + 1
    return dw + 0.0, db + 0.0, Sw, Sb, K


def in_wgrad_gradient(c: Case):
    """(g, |g| bound): the logical gradient [n, cout, h, w] image_in_wgrad sums -- the interior of a halo-0 / folded tensor, the fold of an
    unfolded one (summed in fp32 while loading: K counts its padded positions)"""
    o = operands(c)
    gp = o.gp[:, :c.c]
    if c.halo and not c.folded:
        return O.reflect_pad_adjoint(gp, 1), O.reflect_pad_adjoint(np.abs(gp), 1)
    g = gp[:, :, 1:-1, 1:-1] if c.halo else gp
    return g, np.abs(g)


def def_in_wgrad(c: Case, accumulate):
    """(dw, db, Sw, Sb, K)"""
    o = operands(c)
    g, ga = in_wgrad_gradient(c)
    dw, db = conv_wgrad(o.img[:, None], o.w.shape, g)
    Sw, Sb = conv_wgrad(np.abs(o.img[:, None]), o.w.shape, ga)
    K = c.n * ((c.h + 2) * (c.w + 2) if (c.halo and not c.folded) else c.h * c.w)
    if accumulate:
        dw, db, Sw, Sb, K = dw + o.dw_old, db + o.db_old, Sw + np.abs(o.dw_old), Sb + np.abs(o.db_old), K + 1
    return dw + 0.0, db + 0.0, Sw, Sb, K


def def_out_bwd(c: Case, accumulate):
    """(gx on the stored domain [n, 16, h + 2, w + 2] with a zero ring, Sx, Kx per element, then def_out_wgrad's five)"""
    o = operands(c)
    g0 = g0_of(o)
    gx = np.zeros((c.n, 16, c.h + 2, c.w + 2))
    Sx = np.zeros_like(gx)
    Kx = np.zeros_like(gx)
    gx[:, :, 1:-1, 1:-1] = O.reflect_pad_adjoint(conv_dgrad_padded(g0, o.w), 1) * (o.x > 0)
    Sx[:, :, 1:-1, 1:-1] = O.reflect_pad_adjoint(conv_dgrad_padded(np.abs(g0), np.abs(o.w)), 1)
    # terms of an element: nine per padded position that reflects onto it (1, 2 or 4)
    Kx[:, :, 1:-1, 1:-1] = O.reflect_pad_adjoint(np.full((1, 1, c.h + 2, c.w + 2), 9.0), 1)
    return (gx + 0.0, Sx, Kx) + def_out_wgrad(c, accumulate)


def references(c: Case):
    """every comparison the sweep makes for the case, in its order: (what, ref, S, K, output dtype, allow_zero) -- allow_zero: a bias sum or
    a masked map of a few pixels may vanish; every other reference must not (0 == 0 would pin nothing)"""
    if c.entry == "in_fwd":
        yield ("y",) + def_in_fwd(c) + (c.dtype, False)
    elif c.entry == "out_fwd":
        yield ("img",) + def_out_fwd(c) + ("f32", False)
    elif c.entry == "out_dgrad":
        for m, a in c.bits:
            m, a = m & ((1 << c.cb) - 1), a & ((1 << c.cb) - 1)      # restricted to the view's blocks
            yield (f"gx(mask={m:#x},accum={a:#x})",) + def_out_dgrad(c, m, a) + (c.dtype, m != 0)
    else:
        for acc in c.accumulate:
            if c.entry == "out_bwd":
                gx, Sx, Kx, dw, db, Sw, Sb, K = def_out_bwd(c, acc)
                yield (f"gx(accumulate={acc})", gx, Sx, Kx, "bf16", False)
            else:
                dw, db, Sw, Sb, K = (def_in_wgrad if c.entry == "in_wgrad" else def_out_wgrad)(c, acc)
            yield (f"dw(accumulate={acc})", dw, Sw, K, "f32", False)
            yield (f"db(accumulate={acc})", db, Sb, K, "f32", True)


# ------------------------------------------------------------------------------------------------------------------------------
# the two comparisons
# ------------------------------------------------------------------------------------------------------------------------------
def exact_condition(S, out_dtype, what=""):
    """what makes the exact family exact: every |term| of an output element sums to less than 2^24 (fp32 output: every partial sum in any
    order is an integer fp32 holds) / to at most 256 (bf16 output: the integers a bf16 holds without gaps)"""
    m = float(np.max(S)) if np.size(S) else 0.0
    assert (m <= 256.0) if out_dtype == "bf16" else (m < 2.0 ** 24), f"{what}: sum |terms| = {m} leaves the exact range of {out_dtype}"


def half_spacing_bf16(v):
    """half the distance between neighbouring bf16 values at magnitude v (8 significant bits)"""
    _, e = np.frexp(np.asarray(v, np.float64))          # v = m 2^e, 0.5 <= m < 1: spacing 2^(e - 8)
    return np.where(np.asarray(v) > 0, np.ldexp(1.0, e - 9), 0.0)


def bound(ref, S, K, out_dtype):
    """the derived per-element bound of the real-valued family (module docstring)"""
    delta = np.asarray(K, np.float64) * 2.0 ** -24 * S
    if out_dtype == "bf16":
        return delta + half_spacing_bf16(np.abs(ref) + delta)
    return delta + 2.0 ** -24 * np.abs(ref)
