"""Cases and fp64 definitions for the hierarchical depth-wise chain kernels of csrc/res2dw.hip (mmif_res2dw_fwd / _dgrad / _wgrad and the
workspace query).  numpy only: tests/test_res2dw_oracle_cpu.py pins the definitions to torch's float64 autograd and proves that the table covers
what it claims and tells every listed wrong definition from the true one; tests/test_gpu_res2dw_sweep.py runs every case on the device.

Definitions (include/mmif.h is the contract; float64 on the stored fp32 operands).  A tensor has nseg * c channels, segment i = channels
[i c, (i + 1) c); the weights are one packed buffer, segment 0 at 0 as [c], segment i >= 1 at float offset c + 9 c (i - 1) as [c][3][3].
 fwd    in_0 = x_0, in_1 = x_1, in_i = y_{i-1} + x_i (i >= 2);  y_0 = b_0 + w_0 in_0,  y_i = b_i + sum_{u,v} w_i[u][v] pad(in_i)[yy + u][xx + v]
        (padding 1 on each stage's own input: reflect without edge repeat, or zeros)
 dgrad  G_{S-1} = gy_{S-1}, G_i = gy_i + dx_{i+1} (1 <= i <= S - 2), G_0 = gy_0;  dx_0 = w_0 G_0, dx_i = the scatter of G_i w_i onto the padded
        domain, then the padding's adjoint: every reflect image summed (fold), or the crop
 wgrad  dw_i[ch][u][v] = sum_{n, pixels} G_i pad(in_i)[yy + u][xx + v], db_i = sum G_i, with G_i and in_i formed from the OPERANDS x, y, gy, dx
        (y the output of fwd for x, dx the output of dgrad for gy)

Bounds (u = 2^-24), derived from the kernel source, never fitted.  A chain of T fp32 FMAs or additions has an error of at most
T u / (1 - T u) <= (T + 1) u times the sum A of the magnitudes of its terms; A is the same definition evaluated on the operands' magnitudes.
 stage-wise   y_i against the fp64 stage on the device's own y_{i-1} and x_i; dx_i against the fp64 adjoint on gy_i + the device's own dx_{i+1}.
              Valid because a block's recomputed halo values are the bits its neighbour stores (one instruction sequence per output).
   fwd    segment 0: one FMA onto the bias (T = 1); segment 1: r2_fwd_strip's 9 FMAs onto the bias (T = 9); segment >= 2: the add that
          forms in_i, then the 9 FMAs (T = 10)                                                                       (T + 1) u A
   dgrad  segment 0: one product (T = 1); r2_dgrad_strip: 9 FMAs from 0 (zero padding: T = 9); reflect: up to 8 mirror images with 16 taps
          in ONE more chain from 0, added last (no term passes more than 16 + 1 roundings: T = 17); + 1 where G_i is a sum  (T + 1) u A
 end to end   y and dx against the full fp64 chain: e_i = (stage bound)_i + |w_i| (*) pad(e_{i-1}) (dgrad: the adjoint, from e_{i+1}), the
              stage bound on the magnitude chain M_{i-1} + e_{i-1} >= |the device's y_{i-1}|, all in fp64
 wgrad  the two operand sums (2); r2_wgrad_tile: per thread one product and 3 FMAs over its strip of 4 (4), the wave butterfly (6), the 4 waves
        in order (3); res2dw_wgrad_reduce: each of 16 chains adds every 16th of the E = n * tiles partials (ceil(E / 16)), then the 16 chains
        in order (15): T = 30 + ceil(E / 16); db has 3 additions instead of the 4 strip operations: the same T covers it   (T + 1) u A
Measured on an MI355X (the report of tests/test_gpu_res2dw_sweep.py over all cases; max err / bound, max err):
 y stage 0.499, 1.4e-06   y chain 0.499, 1.3e-06   dx stage 0.498, 5.1e-07   dx chain 0.498, 5.3e-07   dw 0.058, 8.8e-05   db 0.041, 2.3e-05
(0.499 is the one FMA / product of segment 0 against its bound of two roundings; the sums' worst-case bounds grow with the chain length,
rounding errors of random sign with its root.)
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
SENT = -1024.0
TH, TW = 32, 64                 # csrc/res2dw.hip R2_TH, R2_TW: the chain kernels' tile
WTH, WTW = 16, 64               # R2_WTH, R2_WTW: the weight gradient's tile
SMAX = 8                        # R2_SMAX
MAX_BLOCKS = 4096               # R2_MAX_BLOCKS: the cap of every launcher's walk
SLOTS = 10                      # R2_SLOTS: workspace floats per (sample, tile, channel)
SUBS = 16                       # R2_SUBS: interleaved chains of the reduce
EINVAL, EWORKSPACE = -1, -3


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Case:
    n: int
    c: int
    nseg: int
    h: int
    w: int
    reflect: bool
    bias: bool = True           # False: NULL bias (fwd) / NULL db (wgrad)
    guard: int = 4              # sentinel floats before and after every output (3: the outputs start off a 16-byte boundary)

    @property
    def id(self):
        return f"{self.n}x{self.nseg}x{self.c}x{self.h}x{self.w}-{'refl' if self.reflect else 'zero'}-{'b' if self.bias else 'nob'}-g{self.guard}"

    @property
    def tiles(self):
        return cdiv(self.h, TH) * cdiv(self.w, TW)

    @property
    def wtiles(self):
        return cdiv(self.h, WTH) * cdiv(self.w, WTW)

    @property
    def workspace_bytes(self):
        return self.n * self.nseg * self.c * self.wtiles * SLOTS * 4

    @property
    def packed(self):
        return self.c + 9 * self.c * (self.nseg - 1)

    @property
    def numel(self):
        return self.n * self.nseg * self.c * self.h * self.w


def operands(c: Case) -> dict:
    """x, gy [n][nseg c][h][w], the packed weights, the bias: fp32, signed, from a seed that is the case's id.  (3 x 3 weights of deviation 1 / 6:
    sum |w| is about 1.2 per stage, so that the magnitude chain of 7 stages, and with it every bound, stays near the outputs' own scale.)"""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    shape = (c.n, c.nseg * c.c, c.h, c.w)
    o = dict(x=rng.standard_normal(shape).astype(np.float32), gy=rng.standard_normal(shape).astype(np.float32))
    o["w"] = np.concatenate([rng.standard_normal(c.c).astype(np.float32)] + [(rng.standard_normal(c.c * 9) / 6).astype(np.float32) for _ in range(c.nseg - 1)])
    o["bias"] = rng.standard_normal(c.nseg * c.c).astype(np.float32) if c.bias else None
    return o


def unpack(c: Case, w, mut=None):
    """[c], then nseg - 1 times [c][3][3]"""
    w = np.asarray(w)
    out = [w[:c.c]]
    if mut == "woff_9c":        # every segment's offset computed as if segment 0 had 9 c weights too (what lies behind the buffer reads as 0)
        w = np.concatenate([w, np.zeros(9 * c.c * c.nseg - w.size)])
    for i in range(1, c.nseg):
        off = 9 * c.c * i if mut == "woff_9c" else c.c + 9 * c.c * (i - 1)
        out.append(w[off:off + 9 * c.c].reshape(c.c, 3, 3))
    return out


def refl(t, L, repeat=False):
    """the in-plane index of padded-domain coordinate t: F.pad(mode='reflect'), or with the edge repeated ('symmetric')"""
    if repeat:
        return -t - 1 if t < 0 else (2 * L - 1 - t if t >= L else t)
    return -t if t < 0 else (2 * (L - 1) - t if t >= L else t)


def pad1(a, mode):
    """[n][c][h][w] -> [n][c][h + 2][w + 2]"""
    if mode == "zero":
        return np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))
    h, w = a.shape[2:]
    iy = [refl(t, h, mode == "repeat") for t in range(-1, h + 1)]
    ix = [refl(t, w, mode == "repeat") for t in range(-1, w + 1)]
    return a[:, :, iy][:, :, :, ix]


def fold_mat(L, mode):
    """[L][L + 2]: the adjoint of padding one axis by 1"""
    m = np.zeros((L, L + 2))
    for t in range(-1, L + 1):
        if mode in ("reflect", "repeat"):
            m[refl(t, L, mode == "repeat"), t + 1] = 1.0
        elif 0 <= t < L:            # zero padding, and the mutation that drops the mirror terms: the crop
            m[t, t + 1] = 1.0
    return m


def conv3(inp, w, mode):
    h, wd = inp.shape[2:]
    xp = pad1(inp, mode)
    acc = np.zeros_like(inp)
    for u in range(3):
        for v in range(3):
            acc += w[None, :, u, v, None, None] * xp[:, :, u:u + h, v:v + wd]
    return acc


def adj3(G, w, mode):
    h, wd = G.shape[2:]
    z = np.zeros(G.shape[:2] + (h + 2, wd + 2))
    for u in range(3):
        for v in range(3):
            z[:, :, u:u + h, v:v + wd] += w[None, :, u, v, None, None] * G
    return fold_mat(h, mode) @ z @ fold_mat(wd, mode).T


def _mode(c: Case, mut):
    if mut == "edge_repeat" and c.reflect:
        return "repeat"
    return "reflect" if c.reflect else "zero"


def _seg(t, c, i):
    return t[:, i * c.c:(i + 1) * c.c]


def _a(mag):
    return (lambda t: np.abs(t)) if mag else (lambda t: t)


def _fwd_extended(c: Case, x, ws, b):
    """the wrong definition `the conv continued past the edge`: x padded ONCE by nseg - 1, every stage a valid conv on the shrinking extended
    domain, the plane cropped out of each stage"""
    H = c.nseg - 1
    xp = np.pad(x, ((0, 0), (0, 0), (H, H), (H, H)), mode="reflect" if c.reflect else "constant")
    y = np.zeros_like(x)
    _seg(y, c, 0)[...] = ws[0][None, :, None, None] * _seg(x, c, 0)
    prev = None
    for i in range(1, c.nseg):
        g = c.nseg - i                      # this stage's input lives on the plane grown by g
        xi = _seg(xp, c, i)[:, :, H - g:H + c.h + g, H - g:H + c.w + g]
        inp = xi if i == 1 else prev + xi
        out = np.zeros(inp.shape[:2] + (inp.shape[2] - 2, inp.shape[3] - 2))
        for u in range(3):
            for v in range(3):
                out += ws[i][None, :, u, v, None, None] * inp[:, :, u:u + out.shape[2], v:v + out.shape[3]]
        if b is not None:
            out += _seg(b[None, :, None, None], c, i)
        _seg(y, c, i)[...] = out[:, :, g - 1:g - 1 + c.h, g - 1:g - 1 + c.w]
        prev = out
    if b is not None:
        _seg(y, c, 0)[...] += _seg(b[None, :, None, None], c, 0)
    return y


def fwd(c: Case, o, mut=None, mag=False, prev=None):
    """y.  prev: a y whose segment i - 1 feeds in_i instead of the chain's own (the stage-wise comparison)"""
    a = _a(mag)
    x, ws = a(f32(o["x"])), unpack(c, a(f32(o["w"])), mut)
    b = a(f32(o["bias"])) if o["bias"] is not None else None
    if mut == "extended_domain" and c.nseg > 1 and min(c.h, c.w) > c.nseg - 1:
        return _fwd_extended(c, x, ws, b)
    mode = _mode(c, mut)
    y = np.zeros_like(x)
    for i in range(c.nseg):
        inp = _seg(x, c, i)
        if i >= 2 or (i == 1 and mut == "add_from_1"):
            inp = inp + _seg(y if prev is None else a(np.asarray(prev, np.float64)), c, i - 1)
        yi = ws[0][None, :, None, None] * inp if i == 0 else conv3(inp, ws[i], mode)
        if b is not None:
            yi = yi + _seg(b[None, :, None, None], c, i)
        _seg(y, c, i)[...] = yi
    return y


def dgrad(c: Case, o, mut=None, mag=False, nxt=None):
    """dx.  nxt: a dx whose segment i + 1 enters G_i instead of the chain's own (the stage-wise comparison)"""
    a = _a(mag)
    g, ws = a(f32(o["gy"])), unpack(c, a(f32(o["w"])), mut)
    mode = "zero" if mut == "no_mirror" else _mode(c, mut)
    dx = np.zeros_like(g)
    for i in range(c.nseg - 1, -1, -1):
        G = _seg(g, c, i)
        if 1 <= i <= c.nseg - 2 or (i == 0 and c.nseg >= 2 and mut == "add_from_1"):
            G = G + _seg(dx if nxt is None else a(np.asarray(nxt, np.float64)), c, i + 1)
        _seg(dx, c, i)[...] = ws[0][None, :, None, None] * G if i == 0 else adj3(G, ws[i], mode)
    return dx


def wgrad(c: Case, o, y, dx, mut=None, mag=False):
    """(dw packed, db) from the operands x, y, gy, dx"""
    a = _a(mag)
    x, g, y, dx = a(f32(o["x"])), a(f32(o["gy"])), a(np.asarray(y, np.float64)), a(np.asarray(dx, np.float64))
    mode = _mode(c, mut)
    parts, db = [], np.zeros(c.nseg * c.c)
    for i in range(c.nseg):
        A, B = _seg(g, c, i), _seg(x, c, i)
        if (1 <= i <= c.nseg - 2 and mut != "G_without_dx") or (i == 0 and c.nseg >= 2 and mut == "y0_feeds_in1"):
            A = A + _seg(dx, c, i + 1)
        if (i >= 2 and mut != "in_without_y") or (i == 1 and mut == "y0_feeds_in1"):
            B = B + _seg(y, c, i - 1)
        db[i * c.c:(i + 1) * c.c] = A.sum(axis=(0, 2, 3))
        if i == 0:
            parts.append(np.einsum("nchw,nchw->c", A, B))
            continue
        Bp = pad1(B, mode)
        dw = np.zeros((c.c, 3, 3))
        for u in range(3):
            for v in range(3):
                dw[:, u, v] = np.einsum("nchw,nchw->c", A, Bp[:, :, u:u + c.h, v:v + c.w])
        parts.append(dw.reshape(-1))
    return np.concatenate(parts), db


def _seg_factor(c: Case, t):
    """[1][nseg c][1][1] from one factor per segment"""
    return np.repeat(np.asarray(t, np.float64), c.c)[None, :, None, None]


def _t_fwd(c: Case):
    return [1 if i == 0 else (9 if i == 1 else 10) for i in range(c.nseg)]


def _t_dgrad(c: Case):
    return [1 if i == 0 else (17 if c.reflect else 9) + (1 if 1 <= i <= c.nseg - 2 else 0) for i in range(c.nseg)]


def stage_bounds(c: Case, o, y_dev, dx_dev) -> dict:
    """per-element bounds of y_i / dx_i against the fp64 stage on the device's own y_{i-1} / dx_{i+1}"""
    return dict(y=(_seg_factor(c, _t_fwd(c)) + 1) * U * fwd(c, o, mag=True, prev=y_dev),
                dx=(_seg_factor(c, _t_dgrad(c)) + 1) * U * dgrad(c, o, mag=True, nxt=dx_dev))


def stage_define(c: Case, o, y_dev, dx_dev) -> dict:
    return dict(y=fwd(c, o, prev=y_dev), dx=dgrad(c, o, nxt=dx_dev))


def _chain_bound(c: Case, o, which):
    """e of the end-to-end recursion (module docstring)"""
    mode = "reflect" if c.reflect else "zero"
    ws = unpack(c, np.abs(f32(o["w"])))
    e = np.zeros((c.n, c.nseg * c.c, c.h, c.w))
    if which == "y":
        T, M, x = _t_fwd(c), fwd(c, o, mag=True), np.abs(f32(o["x"]))       # M_i >= |y_i|, so M_{i-1} + e_{i-1} >= |the device's y_{i-1}|
        b = np.abs(f32(o["bias"])) if o["bias"] is not None else np.zeros(c.nseg * c.c)
        for i in range(c.nseg):
            inp = _seg(x, c, i) + (_seg(M, c, i - 1) + _seg(e, c, i - 1) if i >= 2 else 0.0)
            A = (ws[0][None, :, None, None] * inp if i == 0 else conv3(inp, ws[i], mode)) + _seg(b[None, :, None, None], c, i)
            _seg(e, c, i)[...] = (T[i] + 1) * U * A + (conv3(_seg(e, c, i - 1), ws[i], mode) if i >= 2 else 0.0)
    else:
        T, M, g = _t_dgrad(c), dgrad(c, o, mag=True), np.abs(f32(o["gy"]))
        for i in range(c.nseg - 1, -1, -1):
            chained = 1 <= i <= c.nseg - 2
            G = _seg(g, c, i) + (_seg(M, c, i + 1) + _seg(e, c, i + 1) if chained else 0.0)
            A = ws[0][None, :, None, None] * G if i == 0 else adj3(G, ws[i], mode)
            _seg(e, c, i)[...] = (T[i] + 1) * U * A + (adj3(_seg(e, c, i + 1), ws[i], mode) if chained else 0.0)
    return e


def bounds(c: Case, o) -> dict:
    """end-to-end bounds of y and dx (against the full fp64 chain)"""
    return dict(y=_chain_bound(c, o, "y"), dx=_chain_bound(c, o, "dx"))


def wgrad_bounds(c: Case, o, y, dx) -> dict:
    T = 30 + cdiv(c.n * c.wtiles, SUBS)
    adw, adb = wgrad(c, o, y, dx, mag=True)
    return dict(dw=(T + 1) * U * adw, db=(T + 1) * U * adb)


def define(c: Case, o, mut=None) -> dict:
    """the four outputs; the weight gradient's operands y and dx are the TRUE chain's (a mutation of wgrad changes how it forms G_i and in_i)"""
    y, dx = fwd(c, o, mut), dgrad(c, o, mut)
    dw, db = wgrad(c, o, fwd(c, o), dgrad(c, o), mut)
    return dict(y=y, dx=dx, dw=dw, db=db)


# which outputs a planted wrong definition changes
MUTATIONS = {
    "add_from_1": ("y", "dx"),          # the add starting at i >= 1 instead of i >= 2 (and its adjoint: G_0 = gy_0 + dx_1)
    "y0_feeds_in1": ("dw", "db"),       # the weight gradient's operands formed as if y_0 fed in_1: in_1 = x_1 + y_0, G_0 = gy_0 + dx_1
    "edge_repeat": ("y", "dx", "dw"),   # padding by edge repeat
    "extended_domain": ("y", ),         # a stage evaluated on the un-reflected extended domain: the conv continued past the edge
    "no_mirror": ("dx", ),              # dgrad without the mirror images
    "G_without_dx": ("dw", "db"),       # G_i without dx_{i+1}
    "in_without_y": ("dw", ),           # in_i without y_{i-1}
    "woff_9c": ("y", "dx"),             # the packed weight offsets computed with 9 c for segment 0
}

NSEGS = (1, 2, 3, 4, 8)
EXT_H = (TH - 1, TH, TH + 1, 2 * TH + 1)
EXT_W = (TW - 1, TW, TW + 1, 2 * TW + 1)
EXT_WH = (WTH - 1, WTH, WTH + 1, 2 * WTH + 1)
SMALL_REFLECT = ((2, 2), (2, 5), (3, 3), (7, 4))


def _cases():
    cs = []
    for i, nseg in enumerate(NSEGS):
        for j in range(4):
            cs.append(Case(n=(1, 2, 3)[(i + j) % 3], c=(3, 1, 3, 1)[j], nseg=nseg, h=EXT_H[j], w=EXT_W[(j + 1 + i) % 4], reflect=(i + j) % 2 == 0,
                           bias=((i + j) // 2) % 2 == 0, guard=(4, 3)[j % 2]))
    # the weight gradient's own tile heights (its widths are the chain kernels')
    for j, hh in enumerate(EXT_WH):
        cs.append(Case(n=2, c=3, nseg=(3, 4, 2, 8)[j], h=hh, w=EXT_W[(j + 2) % 4], reflect=j % 2 == 1, bias=j < 2, guard=(3, 4)[j % 2]))
    # reflect planes smaller than the halo of an 8-segment chain: every mirror of an axis meets
    for j, (hh, ww) in enumerate(SMALL_REFLECT):
        cs.append(Case(n=(1, 2, 3, 1)[j], c=(3, 1, 3, 1)[j], nseg=8, h=hh, w=ww, reflect=True, bias=j % 2 == 0, guard=(3, 4)[j % 2]))
    cs.append(Case(n=1, c=1, nseg=8, h=1, w=1, reflect=False))                          # zero padding has no smallest plane
    cs.append(Case(n=2, c=3, nseg=4, h=1, w=9, reflect=False, bias=False, guard=3))
    # the channel counts of Res2Fusion's two blocks
    cs.append(Case(n=2, c=16, nseg=4, h=9, w=10, reflect=True, bias=False))
    cs.append(Case(n=1, c=48, nseg=8, h=6, w=11, reflect=True, guard=3))
    cs.append(Case(n=3, c=16, nseg=3, h=5, w=4, reflect=False))
    # more (column, tile) and (plane, tile) pairs than the walks have blocks: 3 x 1400 = 4200 columns, 8400 planes > 4096
    cs.append(Case(n=3, c=1400, nseg=2, h=2, w=3, reflect=True, guard=3))
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


CASES = _cases()

# one (n, c, nseg, h, w, reflect) per class of illegal arguments, with a piece of the message
ILLEGAL = (
    ((1, 1, 0, 8, 8, 0), b"nseg must be 1..8"), ((1, 1, 9, 8, 8, 0), b"nseg must be 1..8"), ((1, 1, -1, 8, 8, 1), b"nseg must be 1..8"),
    ((0, 1, 1, 8, 8, 0), b"bad arguments"), ((1, 0, 1, 8, 8, 0), b"bad arguments"), ((1, 1, 1, 0, 8, 0), b"bad arguments"),
    ((1, 1, 1, 8, 0, 0), b"bad arguments"),
    ((1, 1, 2, 1, 8, 1), b"reflect padding needs h,w >= 2"), ((1, 1, 8, 8, 1, 1), b"reflect padding needs h,w >= 2"),
    ((4096, 64, 8, 32, 32, 0), b"too many elements"), ((1, 8192, 8, 2, 2, 0), b"too many elements"),
)
