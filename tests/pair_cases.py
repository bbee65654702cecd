"""Cases and fp64 definitions for the pair-conv kernels of PFNetv2's self-learned fusion (csrc/pair.hip: pairconv_fwd_kernel,
pairconv_fwd_strip_kernel, pairconv_dgrad_kernel, pairconv_wgrad_kernel + pairconv_wgrad_reduce, pairconv_bwd_kernel behind mmif_pairconv_fwd /
_dgrad / _wgrad / _bwd).  No GPU needed: tests/test_pair_oracle_cpu.py pins the definitions to torch's float64 autograd, proves every case
discriminating and the table complete; tests/test_gpu_pair_sweep.py runs every case on the device.

Every channel c of the operands a, b [n, C, h, w] is an independent 2-channel image with shared weights w[nout][2][3][3]; the definitions stack
the pairs as [n*C, 2, h, w] and are float64 numpy on oracle.fusion_oracle:

* forward     oa[c] = act(bias[0] + corr(reflect_pad(a[c]), w[0][0]) + corr(reflect_pad(b[c]), w[0][1])) (+ res1 + res2 AFTER the activation);
              ob with w[1], bias[1], when nout = 2 (no residual)
* gx          padded domain [h+2][w+2]: gx_c[p] = sum_o sum_tap w[o][c][tap] g_o[p - tap + 1], g zero outside the image; + `add` at interior
              positions only (an unfolded halo-1 `add`: its fold); then, on the channel blocks in mask_bits, * [x_c(R(p)) > 0], R = the reflect
              source, so that folding afterwards equals masking the folded gradient
* dw, db      dw[o][c][tap] = sum_{n, channel, p} g_o[p] reflect_pad(x_c)[p + tap - 1], db[o] = sum g_o; accumulate adds onto the old values; an
              unfolded halo-1 g means its fold
* fused       gx and dw / db of one call

bf16 cases evaluate the definitions on the bf16-rounded values the kernel reads: the mask [x > 0] is then exact and no case excludes anything.

Bounds (u = 2^-24, ULP = 2^-8), derived, never fitted:
* forward, gx:  |got - want| <= T u S (+ ULP |want| when the store is bf16), S = the definition on absolute values, T = its number of terms
* dw, db:       |got - want| <= D u sum|g x|, D = the longest chain of dependent additions a term passes through (wgrad_depth below)
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle import fusion_oracle as O

U = 2.0 ** -24
ULP = 2.0 ** -8
PT = 16                 # pair.hip PT: tile edge of pairconv_fwd_kernel / _wgrad_kernel (image domain), _dgrad_kernel / _bwd_kernel (stored domain)
FT = 32                 # pair.hip FT: tile edge of pairconv_fwd_strip_kernel, 4-wide strips
PERSISTENT_BLOCKS = 2048    # pair.hip PAIR_WG_BLOCKS = PAIR_BWD_BLOCKS

MUTATIONS = ("taps_transposed", "inputs_swapped", "outputs_swapped", "zero_padding", "clamped_ring_mask", "add_in_ring", "residual_before_act")


def cdiv(a, b):
    return (a + b - 1) // b


def bits(*i):
    return sum(1 << k for k in i)


ALT = 0x5a5a5a5a5a5a5a5a


@dataclass(frozen=True)
class Case:
    op: str                   # fwd | dgrad | wgrad | bwd
    dtype: str                # bf16 | f32
    n: int
    cb: int                   # channel blocks per operand
    h: int
    w: int
    nout: int = 2
    relu: bool = True         # fwd
    bias: bool = True         # fwd
    res: str = "none"         # fwd: none | ops (the operands themselves) | other
    strip: int = 1            # fwd, bf16: $MMIF_PAIR_STRIP
    mask: str = "none"        # dgrad, bwd: none | all | b67 | alt
    add: str = "none"         # dgrad, bwd: none | h0 | folded | raw (halo 1, unfolded: dgrad only)
    g: str = "folded"         # dgrad, wgrad, bwd: h0 | folded | raw (halo 1, unfolded: wgrad only)
    pair: bool = True         # a and b are views of ONE tensor at a non-zero cb_off (the engine's layout); False: two tensors at cb_off 0
    accumulate: tuple = (0, 1)   # wgrad, bwd
    note: str = ""

    @property
    def id(self):
        s = f"{self.op}-{self.dtype}-{self.n}x{self.cb}cbx{self.h}x{self.w}-o{self.nout}"
        if self.op == "fwd":
            s += f"-{'relu' if self.relu else 'lin'}-{'b' if self.bias else 'nob'}-res_{self.res}" + (f"-strip{self.strip}" if self.dtype == "bf16" else "")
        else:
            s += f"-g_{self.g}"
        if self.op in ("dgrad", "bwd"):
            s += f"-m_{self.mask}-add_{self.add}"
        return s + ("" if self.pair else "-own") + (("-" + self.note) if self.note else "")

    @property
    def C(self):
        return 8 * self.cb

    @property
    def mask_bits(self):
        full = (1 << self.cb) - 1
        return {"none": 0, "all": full, "b67": bits(6, 7), "alt": ALT & full}[self.mask]

    @property
    def has_gx(self):
        return self.op in ("dgrad", "bwd")

    @property
    def has_dw(self):
        return self.op in ("wgrad", "bwd")

    # ---- what the kernels make of the shape (read from the host code of pair.hip)
    @property
    def tiles(self):
        """tiles the launch walks: 16x16 of the image (fwd, wgrad) or of gx's stored [h+2][w+2] (dgrad, bwd); the bf16 strip forward 32x32"""
        if self.op == "fwd" and self.dtype == "bf16" and self.strip:
            return self.n * self.cb * cdiv(self.h, FT) * cdiv(self.w, FT)
        e = 2 if self.has_gx else 0
        return self.n * self.cb * cdiv(self.h + e, PT) * cdiv(self.w + e, PT)

    @property
    def tiles_per_block(self):
        """persistent kernels: G = min(tiles, 2048) blocks, block b walks tiles b, b + G, ..."""
        return cdiv(self.tiles, min(self.tiles, PERSISTENT_BLOCKS))

    def terms(self, which):
        """T: terms summed into one element of the forward output (`oa`, `ob`) or of gx"""
        if which == "oa":
            return 18 + int(self.bias) + (2 if self.res != "none" else 0)
        if which == "ob":
            return 18 + int(self.bias)
        return 9 * self.nout + {"none": 0, "h0": 1, "folded": 1, "raw": 4}[self.add]     # raw: load_grad_fold sums up to 4 stored values in fp32

    def wgrad_depth(self, which="dw"):
        """D: the longest chain of dependent fp32 additions one product g x (or one g, for db) passes through, read from pair.hip.
        pairconv_wgrad_kernel, and pairconv_bwd_kernel on fp32 storage: a thread's accumulator of one tap is an f32x2 that takes 4 pk_fma per
          tile (granule pairs k = 0..3; an fma rounds once) -> 4 per tile; db: (g0 + g1) + (g2 + g3), then += -> 3 per tile.
        pairconv_bwd_kernel on bf16 storage: dot8_bf16 = 4 chained fdot2 steps per tile, two roundings each -> 8 per tile, dw and db alike.
        A block walks tiles_per_block tiles.  Then: the two halves of the f32x2 (1; the bf16 fused kernel's accumulator is scalar: 0), 6 steps
        of the 64-lane shuffle tree, (red[0] + red[1]) + (red[2] + red[3]) = 2.  pairconv_wgrad_reduce: each of 256 threads chains
        ceil(G / 256) partials, block_sum = 6 shuffle steps + 4 waves added in turn.  An unfolded halo-1 g: load_grad_fold adds up to 4 stored values
        (0 + first is exact) -> + 3.  (accumulate: `*dst + tot` rounds the final value once more; def_wgrad adds that term on its own.)"""
        G = min(self.tiles, PERSISTENT_BLOCKS)
        fused_bf16 = self.op == "bwd" and self.dtype == "bf16"
        per_tile = 8 if fused_bf16 else (4 if which == "dw" else 3)
        return (per_tile * self.tiles_per_block + (0 if fused_bf16 else 1) + 6 + 2 + cdiv(G, 256) + 6 + 4 + (3 if self.g == "raw" else 0))

    def mutations(self):
        """the wrong definitions that can show on this case"""
        m = ["taps_transposed", "inputs_swapped"]
        if self.nout == 2:
            m.append("outputs_swapped")
        if self.op == "fwd" or self.has_dw:
            m.append("zero_padding")
        if self.has_gx and self.mask_bits:
            m.append("clamped_ring_mask")
        if self.has_gx and self.add != "none":
            m.append("add_in_ring")
        if self.op == "fwd" and self.res != "none" and self.relu:
            m.append("residual_before_act")
        return m


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
TILE_EDGES = (2, 3, 14, 15, 16, 17, 30, 31)                  # h or w at an edge of the 16x16 tiles, in the image domain or in [h+2][w+2]
STRIP_EDGES = (2, 3, 5, 6, 7, 31, 32, 33, 34, 65)            # w at an edge of the strip forward's 32x32 tiles / 4-wide strips
# every TILE_EDGES value as h and as w; 2-row and 2-column images; one tall-thin and one wide-flat shape
EDGE_SHAPES = [(2, 2), (3, 3), (13, 13), (2, 19), (19, 2), (14, 15), (15, 16), (16, 17), (17, 14), (30, 31), (31, 30), (70, 3), (3, 70)]
STRIP_SHAPES = [(4, 5), (3, 6), (5, 7), (33, 32), (32, 33), (2, 34), (3, 65)]
BIG = (65, 8, 17, 17)          # 65 * 8 planes of 2 x 2 tiles in both domains = 2080 tiles: blocks 0..31 walk two tiles, the others one

FWD_VARIANTS = [(nout, relu, bias, res) for nout in (1, 2) for relu in (True, False) for bias in (True, False) for res in ("none", "ops", "other")]
GX_VARIANTS = [(nout, mask, add, g) for nout in (1, 2) for mask in ("none", "all", "alt") for add in ("none", "h0", "folded", "raw") for g in ("h0", "folded")]
WG_VARIANTS = [(nout, g) for nout in (1, 2) for g in ("h0", "folded", "raw")]
DTYPES = ("bf16", "f32")


def _strips(dtype):
    return (1, 0) if dtype == "bf16" else (1,)


def _cases():
    cs = []
    k = 0      # walks the variant lists, so that every edge shape meets a different combination
    for dtype in DTYPES:
        # ---- every edge shape, a few variants each
        for i, (h, w) in enumerate(EDGE_SHAPES + STRIP_SHAPES):
            cb = (1, 3)[i % 2]
            for strip in _strips(dtype):
                for j in range(2):
                    nout, relu, bias, res = FWD_VARIANTS[(5 * k + 7 * j) % len(FWD_VARIANTS)]
                    cs.append(Case("fwd", dtype, 2, cb, h, w, nout, relu=relu, bias=bias, res=res, strip=strip, pair=bool((i + j) % 2)))
                k += 1
        for i, (h, w) in enumerate(EDGE_SHAPES):
            cb = (3, 1)[i % 2]
            for j in range(2):
                nout, mask, add, g = GX_VARIANTS[(11 * k + 13 * j) % len(GX_VARIANTS)]
                mask = "all" if (cb == 1 and mask == "alt") else mask
                cs.append(Case("dgrad", dtype, 2, cb, h, w, nout, mask=mask, add=add, g=g, pair=bool((i + j) % 2)))
                cs.append(Case("bwd", dtype, 2, cb, h, w, nout, mask=mask, add=("folded" if add == "raw" else add), g=g, pair=bool((i + j + 1) % 2)))
                nout, g = WG_VARIANTS[(k + j) % len(WG_VARIANTS)]
                cs.append(Case("wgrad", dtype, 2, cb, h, w, nout, g=g, pair=bool((i + j) % 2)))
                k += 1
        # ---- every variant, at one shape with ragged tiles in both domains and more than one tile per plane
        for strip in _strips(dtype):
            for nout, relu, bias, res in FWD_VARIANTS:
                cs.append(Case("fwd", dtype, 2, 3, 17, 35, nout, relu=relu, bias=bias, res=res, strip=strip, note="all"))
        for nout, mask, add, g in GX_VARIANTS:
            cs.append(Case("dgrad", dtype, 2, 3, 17, 18, nout, mask=mask, add=add, g=g, note="all"))
            if add != "raw":
                cs.append(Case("bwd", dtype, 2, 3, 17, 18, nout, mask=mask, add=add, g=g, note="all"))
        for nout, g in WG_VARIANTS:
            cs.append(Case("wgrad", dtype, 2, 3, 17, 18, nout, g=g, note="all"))
        # ---- the engine's geometry: 8 channel blocks per operand, both as views of one 16-block tensor; mask_bits = bits(6, 7) / all / alternating
        for strip in _strips(dtype):
            cs.append(Case("fwd", dtype, 1, 8, 15, 33, 2, strip=strip, note="engine"))
            cs.append(Case("fwd", dtype, 1, 8, 15, 33, 1, relu=False, res="ops", strip=strip, note="engine"))
            cs.append(Case("fwd", dtype, 1, 8, 15, 33, 1, relu=False, res="other", strip=strip, note="engine"))
        for mask in ("b67", "all", "alt", "none"):
            add = {"b67": "folded", "all": "h0", "alt": "raw", "none": "none"}[mask]
            cs.append(Case("dgrad", dtype, 1, 8, 15, 16, 2, mask=mask, add=add, note="engine"))
            cs.append(Case("bwd", dtype, 1, 8, 15, 16, 2, mask=mask, add=("folded" if add == "raw" else add), note="engine"))
        cs.append(Case("bwd", dtype, 1, 8, 15, 16, 1, mask="b67", add="none", note="engine"))
        cs.append(Case("wgrad", dtype, 1, 8, 15, 16, 2, g="folded", note="engine"))
        cs.append(Case("wgrad", dtype, 1, 8, 15, 16, 1, g="raw", note="engine"))
        # ---- more tiles than persistent blocks: some blocks walk two tiles, the others one
        n, cb, h, w = BIG
        cs.append(Case("wgrad", dtype, n, cb, h, w, 2, g="folded", note="persistent"))
        cs.append(Case("bwd", dtype, n, cb, h, w, 2, mask="b67", add="folded", note="persistent"))
        cs.append(Case("dgrad", dtype, n, cb, h, w, 2, mask="b67", add="raw", note="persistent"))
        for strip in _strips(dtype):
            cs.append(Case("fwd", dtype, n, cb, h, w, 2, strip=strip, note="persistent"))
    return cs


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


# ------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------
def rnd(a, dtype):
    """the values a tensor of the case's dtype holds, as float64"""
    a = np.asarray(a, np.float32)
    return (O.bf16_round(a) if dtype == "bf16" else a).astype(np.float64)


def fold(gp):
    """adjoint of reflect padding by 1 of a stored halo-1 tensor [.., h+2, w+2] -> [.., h, w]"""
    return O.reflect_pad_adjoint(gp, 1)


def pad0(a):
    return np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))


def ring_zero(a):
    a = a.copy()
    a[:, :, 0] = 0
    a[:, :, -1] = 0
    a[:, :, :, 0] = 0
    a[:, :, :, -1] = 0
    return a


def _stored(rng, shape, kind, dtype):
    """a gradient as the tensor stores it: h0 [n, C, h, w]; folded / raw [n, C, h+2, w+2], ring zero / ring alive"""
    n, C, h, w = shape
    if kind == "h0":
        return rnd(rng.standard_normal(shape), dtype)
    gp = rnd(rng.standard_normal((n, C, h + 2, w + 2)), dtype)
    return ring_zero(gp) if kind == "folded" else gp


def logical(stored, kind, absolute=False):
    """the gradient the call means ([n, C, h, w]): the stored interior, or the fp64 fold of an unfolded halo-1 tensor (the kernels fold in
    fp32 without storing); absolute: the same on |stored values|, for the bounds"""
    s = np.abs(stored) if absolute else stored
    return s if kind == "h0" else (s[:, :, 1:-1, 1:-1] if kind == "folded" else fold(s))


@dataclass
class Operands:
    a: np.ndarray
    b: np.ndarray
    w: np.ndarray          # [nout, 2, 3, 3], fp32 values
    bias: np.ndarray       # [nout] (zeros when the case passes NULL)
    r1: np.ndarray
    r2: np.ndarray
    g: list                # stored upstream gradients, one per output
    add: np.ndarray        # stored residual gradient (None: absent)
    dw_old: np.ndarray
    db_old: np.ndarray


_OPS = {}


def operands(c: Case) -> Operands:
    key = (c.dtype, c.n, c.cb, c.h, c.w, c.nout, c.bias, c.res, c.add, c.g)
    if key in _OPS:
        return _OPS[key]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    shape = (c.n, c.C, c.h, c.w)
    a, b = rnd(rng.standard_normal(shape), c.dtype), rnd(rng.standard_normal(shape), c.dtype)
    w = (rng.standard_normal((c.nout, 2, 3, 3)) * 0.3).astype(np.float32).astype(np.float64)
    bias = (rng.standard_normal(c.nout) * 0.25).astype(np.float32).astype(np.float64) if c.bias else np.zeros(c.nout)
    if c.res == "ops":
        r1, r2 = a, b
    elif c.res == "other":
        r1, r2 = rnd(rng.standard_normal(shape), c.dtype), rnd(rng.standard_normal(shape), c.dtype)
    else:
        r1 = r2 = None
    g = [_stored(rng, shape, c.g, c.dtype) for _ in range(c.nout)]
    add = _stored(rng, shape, c.add, c.dtype) if c.add != "none" else None
    scale = np.sqrt(c.n * c.C * c.h * c.w)
    dw_old = (rng.standard_normal(w.shape) * scale).astype(np.float32).astype(np.float64)
    db_old = (rng.standard_normal(c.nout) * scale).astype(np.float32).astype(np.float64)
    o = Operands(a, b, w, bias, r1, r2, g, add, dw_old, db_old)
    _OPS[key] = o
    while len(_OPS) > 4:
        _OPS.pop(next(iter(_OPS)))
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# definitions (mut: one of MUTATIONS, a deliberately wrong definition for tests/test_pair_oracle_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------------
def stack_pairs(a, b):
    """[n, C, h, w] x 2 -> [n*C, 2, h, w]: every channel an independent 2-channel image"""
    return np.ascontiguousarray(np.stack([a, b], axis=2).reshape(-1, 2, a.shape[2], a.shape[3]))


def stack_list(gs):
    return np.ascontiguousarray(np.stack(gs, axis=2).reshape(-1, len(gs), gs[0].shape[2], gs[0].shape[3]))


def unstack(y, n, C):
    return [np.ascontiguousarray(y[:, i].reshape(n, C, y.shape[2], y.shape[3])) for i in range(y.shape[1])]


def _mut_w(w, mut):
    if mut == "taps_transposed":
        return np.ascontiguousarray(w.transpose(0, 1, 3, 2))
    if mut == "inputs_swapped":
        return np.ascontiguousarray(w[:, ::-1])
    if mut == "outputs_swapped":
        return np.ascontiguousarray(w[::-1])
    return w


def fwd_on(a, b, w, bias, relu, r1, r2, mut=None):
    """[oa, ob?] of the forward on explicit arrays"""
    X = stack_pairs(a, b)
    w = _mut_w(w, mut)
    if mut == "zero_padding":
        z = O.conv2d_general_fwd(X, w, bias, 1, 1, False, False)
    else:
        z = O.conv2d_reflect_fwd(X, w, bias, relu=False)
    out = unstack(z, a.shape[0], a.shape[1])
    if mut == "residual_before_act" and r1 is not None:
        out[0] = out[0] + r1 + r2
    if relu:
        out = [np.maximum(y, 0) for y in out]
    if mut != "residual_before_act" and r1 is not None:
        out[0] = out[0] + r1 + r2          # pair.hip: `+ feat1 + feat2 ... added to output 0`, after the activation
    return out


def def_fwd(c: Case, mut=None):
    """(outs, bounds): [oa, ob?] and the per-element bound of each"""
    o = operands(c)
    outs = fwd_on(o.a, o.b, o.w, o.bias, c.relu, o.r1, o.r2, mut)
    ab = (lambda x: None if x is None else np.abs(x))
    S = fwd_on(np.abs(o.a), np.abs(o.b), np.abs(o.w), np.abs(o.bias), False, ab(o.r1), ab(o.r2))
    bounds = [c.terms(k) * U * s + (ULP * np.abs(y) if c.dtype == "bf16" else 0.0) for k, s, y in zip(("oa", "ob"), S, outs)]
    return outs, bounds


def block_mask(mask_bits, C):
    return np.array([(mask_bits >> (ch // 8)) & 1 for ch in range(C)], np.float64)[None, :, None, None]


def gx_on(gs, w, a, b, mask_bits, add, mut=None, absolute=False):
    """[gxa, gxb] on the stored domain [n, C, h+2, w+2]; gs: logical gradients, add: logical residual gradient or None"""
    n, C = a.shape[:2]
    gxp = unstack(O.conv2d_reflect_dgrad_padded(stack_list(gs), _mut_w(w, mut)), n, C)
    out = []
    for x, gx in zip((a, b), gxp):
        if add is not None:
            gx = gx + (np.pad(add, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge") if mut == "add_in_ring" else pad0(add))
        pos = (x > 0).astype(np.float64)
        posp = np.pad(pos, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge") if mut == "clamped_ring_mask" else O.reflect_pad(pos, 1)
        mm = block_mask(mask_bits, C)
        out.append(gx * (1 - mm + mm * posp))
    return out


def def_gx(c: Case, mut=None):
    """(outs, bounds): [gxa, gxb] and the per-element bound of each (zero where the mask zeroes: such an element must be exactly 0)"""
    o = operands(c)
    gs = [logical(g, c.g) for g in o.g]
    add = logical(o.add, c.add) if o.add is not None else None
    outs = gx_on(gs, o.w, o.a, o.b, c.mask_bits, add, mut)
    gabs = [logical(g, c.g, True) for g in o.g]
    addabs = logical(o.add, c.add, True) if o.add is not None else None
    S = gx_on(gabs, np.abs(o.w), o.a, o.b, c.mask_bits, addabs)
    bounds = [c.terms("gx") * U * s + (ULP * np.abs(y) if c.dtype == "bf16" else 0.0) for s, y in zip(S, outs)]
    return outs, bounds


def wgrad_on(a, b, gs, mut=None):
    X, G = stack_pairs(a, b), stack_list(gs)
    w0 = np.zeros((len(gs), 2, 3, 3))
    if mut == "zero_padding":
        _, dw, db = O.conv2d_general_bwd(X, w0, None, G, 1, 1, False, False)
    else:
        _, dw, db = O.conv2d_reflect_bwd(X, w0, None, G, relu=False, need_gx=False)
    if mut == "outputs_swapped":
        db = db[::-1]
    return _mut_w(dw, mut), np.ascontiguousarray(db)


def def_wgrad(c: Case, accumulate=0, mut=None):
    """(dw, db, bound_dw, bound_db).  accumulate: old + fresh; the bound then has the final addition's own rounding, u (|old| + sum|g x|)"""
    o = operands(c)
    dw, db = wgrad_on(o.a, o.b, [logical(g, c.g) for g in o.g], mut)
    Sdw, Sdb = wgrad_on(np.abs(o.a), np.abs(o.b), [logical(g, c.g, True) for g in o.g])
    bdw, bdb = c.wgrad_depth("dw") * U * Sdw, c.wgrad_depth("db") * U * Sdb
    if accumulate:
        return dw + o.dw_old, db + o.db_old, bdw + U * (np.abs(o.dw_old) + Sdw), bdb + U * (np.abs(o.db_old) + Sdb)
    return dw, db, bdw, bdb
