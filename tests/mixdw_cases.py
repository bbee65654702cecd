"""Cases and fp64 definitions for the mixed depth-wise kernels of csrc/mixdw.hip (mmif_mixdw_fwd / _dgrad / _wgrad and the workspace query).
numpy only: tests/test_mixdw_oracle_cpu.py pins the definitions to torch's float64 autograd and proves that the table covers what it claims
and tells every listed wrong definition from the true one; tests/test_gpu_mixdw_sweep.py runs every case on the device.

Definitions (include/mmif.h is the contract; float64 on the stored fp32 operands).  A tensor has nseg * c channels, segment i = channels
[i c, (i + 1) c) with kernel k_i = k0 + 2 i, stride 1, padding p_i = k_i / 2 (reflect without edge repeat, or zeros); the weights are one packed
buffer, segment i at float offset c sum_{j<i} k_j^2 with layout [c][k_i][k_i].
 fwd    y = bias + sum_{u,v} w[u][v] xpad[yy + u][xx + v]
 dgrad  the scatter of gy w onto the padded domain, then the padding's adjoint: every reflect image summed (fold), or the crop
 wgrad  dw[ch][u][v] = sum_{n, pixels} gy xpad[yy + u][xx + v], db = sum gy

Bounds (u = 2^-24), derived from the kernel source, never fitted.  A chain of T fp32 FMAs or additions has an error of at most
T u / (1 - T u) <= (T + 1) u times the sum A of the magnitudes of its terms; A is the same definition evaluated on the operands' magnitudes.
 fwd    md_fwd_tile: k k FMAs onto the bias                                                                            (k k + 1) u A
 dgrad  md_dgrad_tile: the in-plane image is k k FMAs from 0; zero padding has nothing else                             (k k + 1) u A
        reflect: up to 8 mirror images (3 x 3 - 1), k k FMAs each, in ONE chain from 0 (<= 8 k k), which is then added to the in-plane
        sum (+ 1): no term passes more than 8 k k + 1 roundings                                                        (8 k k + 2) u A
 wgrad  md_wgrad_tile: per thread one product and 3 FMAs over its strip of 4 (4), the wave butterfly (6), the 4 waves in order (3);
        mixdw_wgrad_reduce: each wave adds every fourth of the E = n * tiles partials (ceil(E / 4)), then the 4 waves (3):
        T = 16 + ceil(E / 4); db has 3 additions instead of the 4 strip operations: the same T covers it                (T + 1) u A
Measured on an MI355X (the report of tests/test_gpu_mixdw_sweep.py over all cases; max err / bound, max err):
 y 0.499, 2.6e-06   dx 0.499, 1.4e-06   dw 0.062, 1.8e-04   db 0.023, 1.3e-04
(0.499 is the one product of a k = 1 segment against its bound of two roundings; the sums' worst-case bounds grow with the chain length,
rounding errors of random sign with its root.)
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
SENT = -1024.0
TH, TW = 16, 64                 # csrc/mixdw.hip MD_TH, MD_TW
MAX_BLOCKS = 4096               # MD_MAX_BLOCKS: the cap of the (plane, tile) walk of every launcher
SLOTS = 50                      # MD_SLOTS: workspace floats per (sample, tile, channel)
LEGAL = tuple((k0, nseg) for k0 in (1, 3, 5, 7) for nseg in (1, 2, 3, 4) if k0 + 2 * (nseg - 1) <= 7)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Case:
    n: int
    c: int
    nseg: int
    k0: int
    h: int
    w: int
    reflect: bool
    bias: bool = True           # False: NULL bias (fwd) / NULL db (wgrad)
    guard: int = 4              # sentinel floats before and after every output (3: the outputs start off a 16-byte boundary)

    @property
    def id(self):
        return f"{self.n}x{self.nseg}x{self.c}x{self.h}x{self.w}-k{self.k0}-{'refl' if self.reflect else 'zero'}-{'b' if self.bias else 'nob'}-g{self.guard}"

    @property
    def ks(self):
        return [self.k0 + 2 * i for i in range(self.nseg)]

    @property
    def tiles(self):
        return cdiv(self.h, TH) * cdiv(self.w, TW)

    @property
    def workspace_bytes(self):
        return self.n * self.nseg * self.c * self.tiles * SLOTS * 4

    @property
    def packed(self):
        return self.c * sum(k * k for k in self.ks)


def operands(c: Case) -> dict:
    """x, gy [n][nseg c][h][w], the packed weights, the bias: fp32, signed, from a seed that is the case's id"""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    shape = (c.n, c.nseg * c.c, c.h, c.w)
    o = dict(x=rng.standard_normal(shape).astype(np.float32), gy=rng.standard_normal(shape).astype(np.float32))
    o["w"] = np.concatenate([(rng.standard_normal(c.c * k * k) / k).astype(np.float32) for k in c.ks])
    o["bias"] = rng.standard_normal(c.nseg * c.c).astype(np.float32) if c.bias else None
    return o


def unpack(c: Case, w):
    out, off = [], 0
    for k in c.ks:
        out.append(np.asarray(w[off:off + c.c * k * k]).reshape(c.c, k, k))
        off += c.c * k * k
    return out


def refl(t, L, repeat=False):
    """the in-plane index of padded-domain coordinate t: F.pad(mode='reflect'), or with the edge repeated ('symmetric')"""
    if repeat:
        return -t - 1 if t < 0 else (2 * L - 1 - t if t >= L else t)
    return -t if t < 0 else (2 * (L - 1) - t if t >= L else t)


def pad2(x, p, mode):
    if p == 0:
        return x
    return np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect" if mode == "reflect" else "constant")


def fold_mat(L, p, mode):
    """[L][L + 2 p]: the adjoint of padding one axis by p"""
    m = np.zeros((L, L + 2 * p))
    for t in range(-p, L + p):
        if mode == "reflect":
            m[refl(t, L), t + p] = 1.0
        elif mode == "repeat":
            m[refl(t, L, True), t + p] = 1.0
        elif 0 <= t < L:            # zero padding, and the mutation that drops the mirror terms: the crop
            m[t, t + p] = 1.0
    return m


def _segments(c: Case, w, mut):
    """per segment (kernel size, weights [c][k][k]) under a mutation of the weight lookup"""
    ws = unpack(c, w)
    segs = []
    for i, k in enumerate(c.ks):
        if mut == "swap_k":
            j = c.nseg - 1 - i
            segs.append((c.ks[j], ws[j]))
        elif mut == "seg0_weights":
            e = np.zeros((c.c, k, k))
            o = (k - c.k0) // 2
            e[:, o:o + c.k0, o:o + c.k0] = ws[0]
            segs.append((k, e))
        else:
            segs.append((k, ws[i]))
    return segs


def _mode(c: Case, mut):
    mode = "reflect" if c.reflect else "zero"
    if mut == "pad_mode" and (c.reflect or min(c.h, c.w) >= c.ks[-1] // 2 + 1):     # (a plane too small to reflect keeps its zeros)
        mode = "zero" if c.reflect else "reflect"
    return mode


def fwd(c: Case, o, mut=None, mag=False):
    a = (lambda t: np.abs(t)) if mag else (lambda t: t)
    x = a(f32(o["x"]))
    y = np.zeros_like(x)
    mode = _mode(c, mut)
    for i, (k, w) in enumerate(_segments(c, a(f32(o["w"])), mut)):
        p = k // 2
        xs = x[:, i * c.c:(i + 1) * c.c]
        acc = np.zeros_like(xs)
        if mut == "no_halo":
            for y0 in range(0, c.h, TH):
                for x0 in range(0, c.w, TW):
                    t = np.pad(xs[:, :, y0:y0 + TH, x0:x0 + TW], ((0, 0), (0, 0), (p, p), (p, p)))
                    th, tw = t.shape[2] - 2 * p, t.shape[3] - 2 * p
                    for u in range(k):
                        for v in range(k):
                            acc[:, :, y0:y0 + th, x0:x0 + tw] += w[None, :, u, v, None, None] * t[:, :, u:u + th, v:v + tw]
        else:
            xp = pad2(xs, p, mode)
            for u in range(k):
                for v in range(k):
                    acc += w[None, :, u, v, None, None] * xp[:, :, u:u + c.h, v:v + c.w]
        y[:, i * c.c:(i + 1) * c.c] = acc
    if o["bias"] is not None:
        y += a(f32(o["bias"]))[None, :, None, None]
    return y


def dgrad(c: Case, o, mut=None, mag=False):
    a = (lambda t: np.abs(t)) if mag else (lambda t: t)
    g = a(f32(o["gy"]))
    dx = np.zeros_like(g)
    mode = _mode(c, mut)
    if mut == "no_mirror":
        mode = "zero"
    elif mut == "edge_repeat" and c.reflect:
        mode = "repeat"
    for i, (k, w) in enumerate(_segments(c, a(f32(o["w"])), mut)):
        p = k // 2
        gs = g[:, i * c.c:(i + 1) * c.c]
        z = np.zeros(gs.shape[:2] + (c.h + 2 * p, c.w + 2 * p))
        for u in range(k):
            for v in range(k):
                z[:, :, u:u + c.h, v:v + c.w] += w[None, :, u, v, None, None] * gs
        dx[:, i * c.c:(i + 1) * c.c] = fold_mat(c.h, p, mode) @ z @ fold_mat(c.w, p, mode).T
    return dx


def wgrad(c: Case, o, mut=None, mag=False):
    """(dw packed, db)"""
    a = (lambda t: np.abs(t)) if mag else (lambda t: t)
    x, g = a(f32(o["x"])), a(f32(o["gy"]))
    mode = _mode(c, mut)
    parts = []
    for i, k in enumerate(c.ks):
        j = c.nseg - 1 - i if mut == "swap_k" else i
        kk = c.ks[j]
        p = kk // 2
        xp = pad2(x[:, i * c.c:(i + 1) * c.c], p, mode)
        gs = g[:, i * c.c:(i + 1) * c.c]
        dw = np.zeros((c.c, kk, kk))
        for u in range(kk):
            for v in range(kk):
                dw[:, u, v] = np.einsum("nchw,nchw->c", gs, xp[:, :, u:u + c.h, v:v + c.w])
        parts.append(dw.reshape(-1))
    return np.concatenate(parts), g.sum(axis=(0, 2, 3))


def _per_channel_k(c: Case):
    return np.repeat(np.asarray(c.ks), c.c)


def bounds(c: Case, o) -> dict:
    """per-element bounds of y, dx, dw, db (module docstring)"""
    kc = _per_channel_k(c).astype(np.float64)[None, :, None, None]
    b = {"y": (kc * kc + 1) * U * fwd(c, o, mag=True)}
    b["dx"] = ((8 * kc * kc + 2) if c.reflect else (kc * kc + 1)) * U * dgrad(c, o, mag=True)
    T = 16 + cdiv(c.n * c.tiles, 4)
    adw, adb = wgrad(c, o, mag=True)
    b["dw"], b["db"] = (T + 1) * U * adw, (T + 1) * U * adb
    return b


def define(c: Case, o, mut=None) -> dict:
    dw, db = wgrad(c, o, mut)
    return dict(y=fwd(c, o, mut), dx=dgrad(c, o, mut), dw=dw, db=db)


# which outputs a planted wrong definition changes
MUTATIONS = {"swap_k": ("y", "dx"), "seg0_weights": ("y", "dx"), "pad_mode": ("y", "dx", "dw"), "no_mirror": ("dx", ), "edge_repeat": ("dx", ),
             "no_halo": ("y", )}

EXT_H = (TH - 1, TH, TH + 1, 2 * TH + 1)
EXT_W = (TW - 1, TW, TW + 1, 2 * TW + 1)


def _cases():
    cs = []
    for i, (k0, nseg) in enumerate(LEGAL):
        for j in range(4):
            cs.append(Case(n=(1, 3)[(i + j) % 2], c=(1, 3, 8)[(i + j) % 3], nseg=nseg, k0=k0, h=EXT_H[j], w=EXT_W[(j + 1 + i) % 4],
                           reflect=(i + j) % 2 == 0, bias=((i + j) // 2) % 2 == 0, guard=(4, 3)[j % 2]))
    # the smallest reflect plane (p + 1)^2 of every kernel size, alone and as the largest kernel of a mix: both mirrors of an axis meet
    for k in (1, 3, 5, 7):
        cs.append(Case(n=1, c=3, nseg=1, k0=k, h=k // 2 + 1, w=k // 2 + 1, reflect=True, bias=k % 4 == 1, guard=3))
        cs.append(Case(n=3, c=1, nseg=(k + 1) // 2, k0=1, h=k // 2 + 1, w=k // 2 + 1, reflect=True, bias=k % 4 == 3))
    cs.append(Case(n=1, c=1, nseg=1, k0=7, h=1, w=1, reflect=False))                    # zero padding has no smallest plane
    cs.append(Case(n=1, c=3, nseg=4, k0=1, h=4, w=2 * TW + 1, reflect=True, bias=False))
    # more (plane, tile) pairs than the walk has blocks: 96 planes x 48 tiles = 4608 > 4096
    cs.append(Case(n=3, c=8, nseg=4, k0=1, h=7 * TH + 1, w=5 * TW + 1, reflect=True, guard=3))
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


CASES = _cases()
