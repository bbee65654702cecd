"""Cases and fp64 definitions for the blocked-layout glue kernels that mmif/nest_engine.py and mmif/engine.py launch between convolutions
(csrc/nest.hip: 2x2 max-pool, nearest-x2 up-sampling + reflect pad, in-place ReLU mask, attention fusion; csrc/misc.hip: element fusion, the
two layout conversions, mmif_zero).  No GPU needed: tests/test_nest_oracle_cpu.py pins the definitions to torch's float64 autograd and to
tests/golden/f4_blocks.npz, proves the table complete, well conditioned and able to tell every listed wrong definition from the true one;
tests/test_gpu_nest_sweep.py runs every case on the device.

Every definition is a float64 numpy function of LOGICAL operands on oracle.fusion_oracle.  A gradient is stored in one of three kinds:
  h0      a halo-0 tensor: the logical gradient itself
  folded  halo 1, MMIF_T_FOLDED set, the halo full of garbage that must be ignored: the logical gradient is the interior
  raw     halo 1, no flag, a live halo: the logical gradient is the reflect-pad adjoint (`fold`) of the stored array.  An axis of extent 1 has
          no reflect source: the halo along it means nothing and is dropped
The two stored-domain kernels (relu_mask, fuse_elem_bwd) are defined on the stored array: position (ys, xs) uses the activation at
(R(ys - halo), R(xs - halo)); the result stays in the input's halo state.  bf16 cases evaluate the definitions on the bf16-rounded operands;
the final store rounding is part of the bound.

Bounds (u = 2^-24, ULP = 2^-8), derived, never fitted: selection and copy kernels are exact (bound 0); everything else
|got - want| <= K u A (+ ULP |want| for a bf16 store), A = the definition with every term replaced by its absolute value and the true
denominators, K = Case.K(): the fp32 roundings that feed one output, counted from the kernel source; accumulate adds u (|old| + A).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle import fusion_oracle as O

U = 2.0 ** -24
ULP = 2.0 ** -8
EPS = O.EPS
SENT = -1024.0                 # bf16-exact, far from every reference value: pre-fills every output and guard block
GRID_CAP_ITEMS = 8192 * 256    # nest.hip grid_for(): at most 8192 blocks of 256 threads (misc.hip: 4096); past this a thread takes a second trip
PS_SLICES, PS_THREADS = 32, 256   # nest.hip plane_sums_kernel: 32 slices of 256 threads per (n, channel block)
STRIDE_HW = (1449, 1448)       # 2 098 152 items at n = cb = 1: the smallest near-square plane past GRID_CAP_ITEMS
DTYPES = ("bf16", "f32")
KINDS = ("h0", "folded", "raw")
ATTN_MODES = ("sa", "ca", "sca")
ELEM_MODES = ("sum", "mean", "max")
KERNELS = ("pool_fwd", "pool_bwd", "up_fwd", "up_bwd", "relu_mask", "attn_fwd", "attn_bwd", "elem_fwd", "elem_bwd", "to_blocked", "to_nchw", "zero")
CONV_CHANNELS = (1, 3, 8, 9, 20)

MUTATIONS = ("last_max_tie", "ceil_mode", "mask_ge_zero", "raw_halo_dropped", "folded_halo_folded", "accumulate_ignores_old",
             "pad_split_reversed", "edge_replication", "source_grid_reflection", "weights_constant", "clamp_always_passes", "sign_zero_is_one",
             "sca_is_sum", "pool_without_abs", "max_tie_one_zero", "clamped_halo_mask")


def cdiv(a, b):
    return (a + b - 1) // b


def fold_roundings(h, w):
    """load_grad_fold on an unfolded halo-1 tensor sums the interior value and its mirrored halo values in fp32, starting from 0 (0 + first is
    exact): per axis 1 source (extent 1), 2 (row 1 or h-2), or 3 (extent 3: row 1 is both) -> sources - 1 additions at the worst pixel"""
    per = lambda e: 1 if e == 1 else (3 if e == 3 else 2)
    return per(h) * per(w) - 1


@dataclass(frozen=True)
class Case:
    k: str                    # one of KERNELS
    dtype: str                # bf16 | f32
    n: int
    cb: int                   # channel blocks of every operand
    h: int                    # pool: the input x; up: the SOURCE; everything else: the tensor
    w: int
    g: str = "h0"             # kind of the incoming gradient (relu_mask, elem_bwd: of the tensor walked; to_blocked, zero: h0 = halo 0, folded = halo 1)
    acc: int = 0              # accumulate onto the outgoing gradient's old interior
    mask: int = 0             # ReLU mask riding in the backward
    mode: str = ""            # attention: sa | ca | sca; element fusion: sum | mean | max
    dh: int = 0               # up: target height = 2 h + dh
    dw: int = 0
    view: bool = True         # operands are views at cb_off 1 / 2 of wider tensors between sentinel guard blocks (False: own tensors, cb_off 0)
    inputs: str = "relu"      # attention: relu (exact zeros, all-zero pixels, one all-zero channel) | signed (offset + one clearly negative channel)
    cached: bool = False      # attn_bwd: _bwd_cached directly after the forward on the same workspace
    same: bool = False        # element fusion: a and b are the same tensor
    c: int = 0                # the conversions: logical channel count
    stride: bool = False      # more items than GRID_CAP_ITEMS: small-integer operands, one state, no mutation run
    note: str = ""

    @property
    def id(self):
        s = f"{self.k}-{self.dtype}-{self.n}x{self.cb}cbx{self.h}x{self.w}"
        if self.k in ("up_fwd", "up_bwd"):
            s += f"+{self.dh}+{self.dw}"
        if self.mode:
            s += f"-{self.mode}"
        if self.k in ("attn_fwd", "attn_bwd"):
            s += f"-{self.inputs}"
        if self.k in ("pool_bwd", "up_bwd", "relu_mask", "attn_bwd", "elem_bwd", "to_nchw", "to_blocked", "zero"):
            s += f"-g_{self.g}"
        if self.k in ("pool_bwd", "up_bwd", "attn_bwd"):
            s += f"-acc{self.acc}"
        if self.k in ("pool_bwd", "up_bwd", "elem_bwd"):
            s += f"-m{self.mask}"
        if self.c:
            s += f"-c{self.c}"
        return s + ("-cached" if self.cached else "") + ("-same" if self.same else "") + ("" if self.view else "-own") + \
            ("-stride" if self.stride else "") + (("-" + self.note) if self.note else "")

    @property
    def C(self):
        return 8 * self.cb

    @property
    def halo(self):
        return 0 if self.g == "h0" else 1

    @property
    def target(self):
        """up: the larger tensor's extent"""
        return 2 * self.h + self.dh, 2 * self.w + self.dw

    @property
    def ghw(self):
        """logical extent of the incoming gradient"""
        if self.k.startswith("pool"):
            return self.h // 2, self.w // 2
        if self.k.startswith("up"):
            return self.target
        return self.h, self.w

    @property
    def items(self):
        """what the kernel's grid-stride loop walks"""
        nc = self.n * self.cb
        if self.k == "pool_fwd":
            return nc * (self.h // 2) * (self.w // 2)
        if self.k == "up_fwd":
            return nc * self.target[0] * self.target[1]
        if self.k in ("attn_fwd", "attn_bwd"):
            return self.n * self.h * self.w
        if self.k in ("relu_mask", "elem_bwd", "zero"):
            return nc * (self.h + 2 * self.halo) * (self.w + 2 * self.halo)
        return nc * self.h * self.w

    @property
    def exact(self):
        if self.k in ("pool_fwd", "up_fwd", "relu_mask", "zero", "to_blocked"):
            return True
        if self.k == "elem_fwd":
            return self.mode == "max"
        if self.k in ("pool_bwd", "to_nchw"):
            return self.g != "raw" and not self.acc
        return False

    def K(self):
        """fp32 roundings that feed one output element, read from nest.hip / misc.hip / common.hpp (C = 8 cb channels; T = ceil(hw / 8192)
        pixels per thread of plane_sums_kernel; F = fold_roundings of a raw gradient, else 0; `accumulate` is bounded on its own)."""
        F = fold_roundings(*self.ghw) if self.g == "raw" else 0
        C, T = self.C, cdiv(self.h * self.w, PS_SLICES * PS_THREADS)
        # one plane sum: a thread's strided partial (T additions, 0 + first exact: counted anyway), block_sum = 6 shuffle steps + 4 waves added
        # in turn, plane_sums_finish = 32 slices in turn
        SUM = T + 6 + 4 + PS_SLICES
        if self.exact:
            return 0
        if self.k in ("pool_bwd", "to_nchw"):
            return F                                   # the selected / copied value is the fp32 fold
        if self.k == "up_bwd":
            return F                                   # + (candidates - 1) additions per source pixel: added element-wise by def_up_bwd
        if self.k == "elem_fwd":
            return 1                                   # a + b (the * 0.5 of 'mean' is exact)
        if self.k == "elem_bwd":
            return 1                                   # g * d, d in {0, 0.5, 1}
        # attention.  spatial weight: s1, s2 = chains of C additions each (2 (C - 1)), s1 + s2 (1), s1 / d (1);
        # channel weight: two plane sums (2 SUM), 1 / hw (1, shared), sum * inv_hw (2), m1 + m2 (1), m1 / dc (1)
        WS, WC = 2 * (C - 1) + 2, 2 * SUM + 5
        if self.k == "attn_fwd":
            sa = WS + 4                                # 1 - ws, two products, their sum
            ca = WC + 4
            return {"sa": sa, "ca": ca, "sca": sa + ca + 1}[self.mode]      # sca: r += the second branch (1); * 0.5 exact
        if self.k == "attn_bwd":
            # spatial: gw = chain of C terms g (a - b): subtraction, product, addition each (3 C) on a folded g (F); gs1 = gw (1 / d - s1 / (d d)):
            # 1 / d, d d, s1 / (d d), the difference, the product (5); ra = gk ws + gs1 sign: product, sum (2)
            sa = WS + 3 * C + F + 5 + 2
            # channel: gsum = a plane sum of g (a - b): 3 roundings per term (3 T + 42) on a folded g (F); coefficient (1 / dc - m1 / (dc dc)) inv_hw
            # (5); ra = gk wc + gwc coef: two products, sum (3)
            ca = WC + (3 * T + 6 + 4 + PS_SLICES) + F + 5 + 3
            return {"sa": sa, "ca": ca, "sca": sa + ca + 1}[self.mode]
        raise AssertionError(self.k)

    def mutations(self):
        """the wrong definitions that can show on this case"""
        if self.stride:
            return []
        m = []
        k = self.k
        if k == "pool_bwd":
            m.append("last_max_tie")
            if self.h % 2 or self.w % 2:
                m.append("ceil_mode")
        if k in ("pool_bwd", "up_bwd", "elem_bwd") and self.mask or k == "relu_mask":
            m.append("mask_ge_zero")
        if k in ("pool_bwd", "up_bwd", "attn_bwd", "to_nchw") and max(self.ghw) >= 2:      # (an axis of extent 1 has no halo to fold)
            if self.g == "raw":
                m.append("raw_halo_dropped")
            if self.g == "folded":
                m.append("folded_halo_folded")
        if k in ("pool_bwd", "up_bwd", "attn_bwd") and self.acc:
            m.append("accumulate_ignores_old")
        if k in ("up_fwd", "up_bwd"):
            if (self.dh % 2 and self.h > 1) or (self.dw % 2 and self.w > 1):
                m.append("pad_split_reversed")
            if self.dh == 3 or self.dw == 3:
                m.append("edge_replication")
            if (self.dh and self.h > 1) or (self.dw and self.w > 1):
                m.append("source_grid_reflection")
        if k in ("attn_fwd", "attn_bwd"):
            if self.mode == "sca":
                m.append("sca_is_sum")
            if self.mode != "ca" and self.inputs == "signed":
                m.append("pool_without_abs")
        if k == "attn_bwd":
            m.append("weights_constant")
            if self.mode != "sa" and self.inputs == "signed" and self.C > 1:
                m.append("clamp_always_passes")
            if self.mode != "ca" and self.inputs == "relu":
                m.append("sign_zero_is_one")
        if k == "elem_bwd" and self.mode == "max":
            m.append("max_tie_one_zero")
        if k in ("relu_mask", "elem_bwd") and self.halo and (self.mask or k == "relu_mask"):
            m.append("clamped_halo_mask")
        return m


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 2), (3, 3), (4, 4), (5, 5), (9, 9), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6), (9, 4), (2, 70), (70, 3)]
UP_SOURCES = [(1, 1), (2, 2), (3, 3), (4, 4), (6, 6), (1, 4), (4, 1), (2, 6), (6, 2), (3, 4)]
UP_FULL = [(2, 2), (3, 4), (6, 2)]          # every admissible (dh, dw) at these sources
ATTN_SHAPES = [(1, 1), (3, 85), (16, 16), (1, 257), (1, 8191), (64, 128), (3, 2731), (5, 3277), (4, 6), (5, 7), (2, 2)]
ELEM_SHAPES = [(2, 2), (3, 5), (4, 4), (7, 6), (2, 9)]
BWD_VARIANTS = [(g, acc, mask) for g in KINDS for acc in (0, 1) for mask in (0, 1)]
NCB = [(1, 1), (2, 3), (3, 2), (1, 2), (2, 1), (3, 3), (1, 3), (3, 1), (2, 2)]


def _diffs(h, w):
    return [(dh, dw) for dh in range(4) for dw in range(4) if dh < 2 * h and dw < 2 * w]


def _cases():
    cs = []
    for dtype in DTYPES:
        k = 0
        # ---- pool: every shape forward; backward: two rotating variants per shape, and the full cross product at three shapes
        for i, (h, w) in enumerate(POOL_SHAPES):
            n, cb = NCB[i % len(NCB)]
            cs.append(Case("pool_fwd", dtype, n, cb, h, w, view=bool(i % 2)))
            for j in range(2):
                g, acc, mask = BWD_VARIANTS[(5 * k + 7 * j) % 12]
                cs.append(Case("pool_bwd", dtype, n, cb, h, w, g=g, acc=acc, mask=mask, view=bool((i + j) % 2)))
            k += 1
        for (h, w), (n, cb) in (((5, 9), (2, 2)), ((3, 7), (1, 3)), ((4, 2), (3, 1))):          # g: 2 x 4, 1 x 3, 2 x 1
            for g, acc, mask in BWD_VARIANTS:
                cs.append(Case("pool_bwd", dtype, n, cb, h, w, g=g, acc=acc, mask=mask, note="all"))
        # ---- up: every source with every admissible target forward; backward rotating, and the full cross product at diff (3, 3) and (1, 2)
        for i, (h, w) in enumerate(UP_SOURCES):
            n, cb = NCB[(i + 3) % len(NCB)]
            ds = _diffs(h, w)
            if (h, w) not in UP_FULL:          # elsewhere: four of the admissible targets, the largest among them
                ds = sorted({ds[(3 * i) % len(ds)], ds[(3 * i + 5) % len(ds)], ds[(7 * i + 2) % len(ds)], ds[-1]})
            for j, (dh, dw) in enumerate(ds):
                cs.append(Case("up_fwd", dtype, n, cb, h, w, dh=dh, dw=dw, view=bool((i + j) % 2)))
                g, acc, mask = BWD_VARIANTS[(5 * k) % 12]
                cs.append(Case("up_bwd", dtype, n, cb, h, w, dh=dh, dw=dw, g=g, acc=acc, mask=mask, view=bool((i + j + 1) % 2)))
                k += 1
        for (h, w, dh, dw), (n, cb) in (((3, 4, 3, 3), (2, 2)), ((2, 3, 1, 2), (1, 3))):
            for g, acc, mask in BWD_VARIANTS:
                cs.append(Case("up_bwd", dtype, n, cb, h, w, dh=dh, dw=dw, g=g, acc=acc, mask=mask, note="all"))
        # ---- relu mask: in place on each kind of stored tensor
        for i, (h, w) in enumerate(ELEM_SHAPES):
            n, cb = NCB[(i + 5) % len(NCB)]
            for g in KINDS:
                cs.append(Case("relu_mask", dtype, n, cb, h, w, g=g, view=bool((i + KINDS.index(g)) % 2)))
        # ---- attention: every plane size (one forward, one backward, rotating variants), and every state at one small shape
        for i, (h, w) in enumerate(ATTN_SHAPES):
            small = h * w <= 64
            n, cb = NCB[(i + 2) % len(NCB)] if small else (1, 1)
            if h * w == 1:
                n = max(n, 2)
            for j, inputs in enumerate(("relu", "signed")):
                mode = ATTN_MODES[(i + j) % 3]
                cs.append(Case("attn_fwd", dtype, n, cb, h, w, mode=mode, inputs=inputs, view=bool((i + j) % 2)))
                g, acc, _ = BWD_VARIANTS[(5 * k) % 12]
                cs.append(Case("attn_bwd", dtype, n, cb, h, w, mode=ATTN_MODES[(i + j + 1) % 3], inputs=inputs, g=g, acc=acc, cached=bool((i + j) % 2),
                               view=bool((i + j + 1) % 2)))
                k += 1
        for inputs in ("relu", "signed"):
            for mode in ATTN_MODES:
                cs.append(Case("attn_fwd", dtype, 2, 2, 5, 7, mode=mode, inputs=inputs, note="all"))
                cs.append(Case("attn_fwd", dtype, 2, 3, 3, 4, mode=mode, inputs=inputs, view=False, note="all"))
                for g in KINDS:
                    for acc in (0, 1):
                        cs.append(Case("attn_bwd", dtype, 2, 2, 5, 7, mode=mode, inputs=inputs, g=g, acc=acc, cached=bool(acc), note="all"))
                        cs.append(Case("attn_bwd", dtype, 2, 3, 3, 4, mode=mode, inputs=inputs, g=g, acc=acc, cached=not acc, view=False, note="all"))
        # ---- element fusion
        for i, (h, w) in enumerate(ELEM_SHAPES):
            n, cb = NCB[(i + 1) % len(NCB)]
            for j, mode in enumerate(ELEM_MODES):
                cs.append(Case("elem_fwd", dtype, n, cb, h, w, mode=mode, view=bool((i + j) % 2), same=(i == 1)))
                for g in KINDS:
                    for mask in (0, 1):
                        cs.append(Case("elem_bwd", dtype, n, cb, h, w, mode=mode, g=g, mask=mask, view=bool((i + j + mask) % 2), same=(i == 1)))
        # ---- the two conversions and mmif_zero
        for i, c in enumerate(CONV_CHANNELS):
            h, w = ELEM_SHAPES[i]
            n = (1, 2, 3)[i % 3]
            for j, g in enumerate(KINDS):
                cs.append(Case("to_nchw", dtype, n, cdiv(c, 8), h, w, g=g, c=c, view=bool((i + j) % 2)))
            for j, g in enumerate(("h0", "folded")):
                cs.append(Case("to_blocked", dtype, n, cdiv(c, 8), h, w, g=g, c=c, view=bool((i + j + 1) % 2)))
                cs.append(Case("zero", dtype, n, cdiv(c, 8), h, w, g=g, view=bool((i + j) % 2)))
        cs.append(Case("to_blocked", dtype, 2, 2, 3, 5, g="folded", c=3, note="wide"))          # a view wider than the channels need: zeros beyond c
        cs.append(Case("to_nchw", dtype, 2, 2, 3, 5, g="raw", c=3, note="wide"))
    # ---- stride: one per kernel, one dtype, one state.  pool_fwd and up_bwd are indexed over the SMALLER tensor (the partner is four times as
    # large): bf16 only
    h, w = STRIDE_HW
    st = dict(n=1, cb=1, view=False, stride=True)
    cs += [Case("pool_fwd", "bf16", h=2 * h, w=2 * w, **st), Case("up_bwd", "bf16", h=h, w=w, g="h0", **st),
           Case("pool_bwd", "f32", h=h, w=w, g="h0", **st), Case("up_fwd", "bf16", h=725, w=724, dh=0, dw=0, **st),
           Case("relu_mask", "bf16", h=h, w=w, g="h0", **st), Case("attn_fwd", "f32", h=h, w=w, mode="sa", **st),
           Case("attn_bwd", "bf16", h=h, w=w, mode="sa", g="h0", **st), Case("elem_fwd", "f32", h=h, w=w, mode="sum", **st),
           Case("elem_bwd", "bf16", h=h, w=w, mode="max", g="h0", mask=1, **st), Case("to_blocked", "bf16", h=h, w=w, c=8, **st),
           Case("to_nchw", "f32", h=h, w=w, c=8, g="h0", **st), Case("zero", "f32", h=h, w=w, **st)]
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
    """adjoint of reflect padding by 1 of a stored halo-1 array [.., h+2, w+2] -> [.., h, w]; an axis of extent 1 drops its halo"""
    h, w = gp.shape[2] - 2, gp.shape[3] - 2
    if h >= 2 and w >= 2:
        return O.reflect_pad_adjoint(gp, 1)
    t = gp[:, :, 1:-1].copy()
    if h >= 2:
        t[:, :, 1] += gp[:, :, 0]
        t[:, :, h - 2] += gp[:, :, h + 1]
    out = t[:, :, :, 1:-1].copy()
    if w >= 2:
        out[:, :, :, 1] += t[:, :, :, 0]
        out[:, :, :, w - 2] += t[:, :, :, w + 1]
    return out


def interior(s):
    return s[:, :, 1:-1, 1:-1]


def logical(stored, kind, absolute=False, mut=None):
    """the gradient the call means ([n, C, h, w]); absolute: the same on |stored values|, for the bounds"""
    s = np.abs(stored) if absolute else stored
    if kind == "h0":
        return s
    if kind == "folded":
        return fold(s) if mut == "folded_halo_folded" else interior(s)
    return interior(s) if mut == "raw_halo_dropped" else fold(s)


def embed(a, halo=1):
    """an interior-only write into a sentinel-filled halo-1 buffer"""
    return a if halo == 0 else np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)), constant_values=SENT)


def stored_grad(rng, shape, kind, dtype):
    """a gradient as the tensor stores it: h0 [n, C, h, w]; folded [n, C, h+2, w+2] with a garbage ring; raw: the ring is part of the value"""
    n, C, h, w = shape
    if kind == "h0":
        return rnd(rng.standard_normal(shape), dtype)
    gp = rnd(rng.standard_normal((n, C, h + 2, w + 2)), dtype)
    if kind == "folded":
        ring = np.ones(gp.shape, bool)
        ring[:, :, 1:-1, 1:-1] = False
        gp[ring] = rnd(300.0 + 50.0 * rng.standard_normal(int(ring.sum())), dtype)
    return gp


def relu_act(rng, shape, dtype):
    """a ReLU output on a grid of 0.5: about half exact zeros, equal non-zero neighbours, so 2-, 3- and 4-way ties of a 2x2 window occur"""
    return rnd(np.round(np.maximum(rng.standard_normal(shape), 0) * 2) / 2, dtype)


def attn_inputs(rng, c):
    """a, b of an attention case, conditioned so that every denominator is clearly in or clearly out of the clamp regime (see
    conditioning()).  relu: non-zero values >= 1/64, about a tenth of the pixels zero in every channel of both, channel 2 all-zero in both.
    signed: N(0.5, 1) with |x| >= 1/64, channel 1 shifted down by 2.5 in both (mean sum about -4)."""
    shape = (c.n, c.C, c.h, c.w)
    out = []
    dead = rng.random((c.n, 1, c.h, c.w)) < 0.1
    if c.n * c.h * c.w > 1:
        dead[0, 0, 0, 0] = True
        dead[-1, 0, -1, -1] = False
    for _ in range(2):
        v = rng.standard_normal(shape)
        if c.inputs == "relu":
            x = np.where(v > 0.3, v + 1.0 / 64, 0.0)
            x = np.where(dead, 0.0, x)
            x[:, 2] = 0.0
        else:
            x = v + 0.5
            x = np.where(np.abs(x) < 1.0 / 64, 1.0 / 64, x)
            x[:, 1] -= 2.5
        out.append(rnd(x, c.dtype))
    a, b = out
    # planes whose sum is neither clearly negative nor clearly positive (small planes of signed values): made positive
    s, sa = (a + b).sum((2, 3)), (np.abs(a) + np.abs(b)).sum((2, 3))
    bad = ~((s == 0) & (sa == 0)) & ~(s <= -0.1 * sa) & ~((s >= 0.25 * sa) & (s >= 2.0 ** 10 * EPS * c.h * c.w))
    a[bad], b[bad] = np.abs(a[bad]) + 0.5, np.abs(b[bad])
    return rnd(a, c.dtype), b


def _int_pattern(shape, mul, mod, sub):
    """small integers, exact in bf16 and in every sum the kernels form: the stride cases compare bit for bit and cost no random numbers"""
    n, C, h, w = shape
    y, x, ch = np.arange(h, dtype=np.int32)[:, None, None], np.arange(w, dtype=np.int32)[None, :, None], np.arange(C, dtype=np.int32)[None, None, :]
    v = ((y * mul[0] + x * mul[1] + ch * mul[2]) % mod - sub).astype(np.float32)       # [h, w, C]
    return np.broadcast_to(v.transpose(2, 0, 1)[None], shape).copy()


_OPS = {}


def operands(c: Case) -> dict:
    key = (c.k if c.k.startswith("to_") else c.k.split("_")[0], c.dtype, c.n, c.cb, c.h, c.w, c.dh, c.dw, c.g, c.inputs, c.c, c.stride, c.same)
    if key in _OPS:
        return _OPS[key]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    shape = (c.n, c.C, c.h, c.w)
    gh, gw = c.ghw
    o = {}
    if c.stride:
        act = lambda sh, s: np.maximum(_int_pattern(sh, (31, 17, 7), 13, 5 + s), 0)
        grd = lambda sh: _int_pattern(sh, (5, 3, 11), 9, 4)
        if c.k.startswith("pool") or c.k == "relu_mask":
            o["x"] = act(shape, 0)
        if c.k.startswith("up"):
            o["x"] = act(shape, 0)
            o["xm"] = o["x"]
        if c.k.startswith(("attn", "elem")):
            o["a"] = act(shape, 0) + 1
            o["b"] = np.maximum(_int_pattern(shape, (13, 29, 3), 11, 4), 0) if c.k.startswith("elem") else act(shape, 2) + 1
        if c.k in ("pool_bwd", "up_bwd", "relu_mask", "attn_bwd", "elem_bwd", "to_nchw"):
            o["g"] = grd((c.n, c.C, gh, gw))
        if c.k == "to_blocked":
            o["src"] = grd((c.n, c.c, c.h, c.w))
        for name in ("old", "old_a", "old_b"):
            o[name] = None
        _OPS[key] = o
        while len(_OPS) > 2:
            _OPS.pop(next(iter(_OPS)))
        return o
    if c.k.startswith("pool"):
        x = relu_act(rng, shape, c.dtype)
        if (c.h // 2) * (c.w // 2) >= 2:       # a four-way tie of zeros of both signs in the first window of every plane
            x[:, :, 0, 0], x[:, :, 0, 1], x[:, :, 1, 0], x[:, :, 1, 1] = -0.0, 0.0, -0.0, 0.0
        o["x"] = x
    elif c.k.startswith("up"):
        o["x"] = relu_act(rng, shape, c.dtype)
        o["xm"] = relu_act(rng, shape, c.dtype)
    elif c.k == "relu_mask":
        o["x"] = relu_act(rng, shape, c.dtype)
    elif c.k.startswith("attn"):
        o["a"], o["b"] = attn_inputs(rng, c)
    elif c.k.startswith("elem"):
        # half of the elements on the 0.5 grid (ties for 'max': equal non-zero values, both zero), half free ReLU values (sums that round)
        a, b = (np.where(rng.random(shape) < 0.5, relu_act(rng, shape, c.dtype), rnd(np.maximum(rng.standard_normal(shape), 0), c.dtype)) for _ in range(2))
        o["a"], o["b"] = (a, a) if c.same else (a, b)
    if c.k.split("_")[0] in ("pool", "up", "relu", "attn", "elem") or c.k == "to_nchw":
        o["g"] = stored_grad(rng, (c.n, c.C, gh, gw), c.g, c.dtype)
    if c.k == "to_nchw":
        o["g"][:, c.c:] = 77.0          # channels beyond c hold garbage that must not reach the output
    if c.k == "to_blocked":
        o["src"] = (rng.standard_normal((c.n, c.c, c.h, c.w)) * 1.37).astype(np.float32).astype(np.float64)      # fp32 values, not bf16-exact
    o["old"] = rnd(rng.standard_normal(shape) * 2, c.dtype)
    o["old_a"], o["old_b"] = rnd(rng.standard_normal(shape) * 2, c.dtype), rnd(rng.standard_normal(shape) * 2, c.dtype)
    _OPS[key] = o
    while len(_OPS) > 6:
        _OPS.pop(next(iter(_OPS)))
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# definitions (mut: one of MUTATIONS, a deliberately wrong definition for tests/test_nest_oracle_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------------
def relu_keep(x, mut=None):
    return (x >= 0) if mut == "mask_ge_zero" else (x > 0)


def pool_windows(x):
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :, :Ho * 2, :Wo * 2].reshape(N, C, Ho, 2, Wo, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)


def pool_tie_counts(x):
    """windows whose maximum is attained 2, 3, 4 times; the same among windows with a non-zero maximum; windows tying -0.0 with +0.0"""
    xv = pool_windows(x)
    m = xv.max(-1, keepdims=True)
    k = (xv == m).sum(-1)
    nz = m[..., 0] != 0
    signs = np.signbit(xv) & (xv == 0)
    mixed = ((m[..., 0] == 0) & signs.any(-1) & (~signs & (xv == 0)).any(-1)).sum()
    return {j: int((k == j).sum()) for j in (2, 3, 4)}, {j: int(((k == j) & nz).sum()) for j in (2, 3, 4)}, int(mixed)


def pool_bwd_on(x, g, mut=None):
    """gradient of nn.MaxPool2d(2, 2): the FIRST maximum of each window takes the cell's gradient; an odd last row / column takes none"""
    if mut == "ceil_mode":          # the odd last row / column pooled as a window of its own, with the neighbouring cell's gradient
        ph, pw = x.shape[2] % 2, x.shape[3] % 2
        xp = np.pad(x, ((0, 0), (0, 0), (0, ph), (0, pw)), constant_values=-np.inf)
        gp = np.pad(g, ((0, 0), (0, 0), (0, ph), (0, pw)), mode="edge")
        return pool_bwd_on(xp, gp)[:, :, :x.shape[2], :x.shape[3]]
    if mut == "last_max_tie":
        idx = 3 - pool_windows(x)[..., ::-1].argmax(-1)
    else:
        _, idx = O.maxpool2x2_fwd(x)
    return O.maxpool2x2_bwd(g, idx, x.shape)


def up_map(L, src, diff, mut=None):
    """source index of every target position along one axis: nearest x2, then ReflectionPad2d with diff // 2 in front"""
    lo = diff - diff // 2 if mut == "pad_split_reversed" else diff // 2
    t = np.arange(L) - lo                      # position on the doubled grid, before padding
    if mut == "edge_replication":
        return np.clip(t, 0, 2 * src - 1) // 2
    if mut == "source_grid_reflection":
        return np.clip(O.reflect_index(np.floor_divide(t, 2), src), 0, src - 1)
    return O.reflect_index(t, 2 * src) // 2


def up_onehot(L, src, diff, mut=None):
    m = np.zeros((L, src))
    m[np.arange(L), up_map(L, src, diff, mut)] = 1
    return m


def up_fwd_on(x, H, W, mut=None):
    if mut is None:
        return O.upsample_nearest2x_fwd(x, (H, W))
    return x[:, :, up_map(H, x.shape[2], H - 2 * x.shape[2], mut)][:, :, :, up_map(W, x.shape[3], W - 2 * x.shape[3], mut)]


def up_bwd_on(g, h, w, mut=None):
    if mut is None:
        return O.upsample_nearest2x_bwd(g, (g.shape[0], g.shape[1], h, w))
    H, W = g.shape[2:]
    return np.einsum("nchw,hi,wj->ncij", g, up_onehot(H, h, H - 2 * h, mut), up_onehot(W, w, W - 2 * w, mut))


def up_candidates(c):
    """[h, w]: target positions that read each source pixel = terms upsample_bwd_kernel sums there"""
    H, W = c.target
    return np.outer(up_onehot(H, c.h, c.dh).sum(0), up_onehot(W, c.w, c.dw).sum(0))


def attn_terms(a, b, mode, mut=None, absolute=False):
    """weights of the two branches and what the backward needs; absolute: numerators on |values|, denominators the true ones"""
    hw = a.shape[2] * a.shape[3]
    t = {}
    ab = np.abs
    s1, s2 = (a.sum(1, keepdims=True), b.sum(1, keepdims=True)) if mut == "pool_without_abs" else (ab(a).sum(1, keepdims=True), ab(b).sum(1, keepdims=True))
    m1, m2 = a.mean((2, 3), keepdims=True), b.mean((2, 3), keepdims=True)
    for name, p1, p2, p1abs in (("s", s1, s2, ab(a).sum(1, keepdims=True)), ("c", m1, m2, ab(a).mean((2, 3), keepdims=True))):
        ssum = p1 + p2
        d = np.maximum(ssum, EPS)
        passes = np.ones_like(d) if mut == "clamp_always_passes" else (ssum >= EPS).astype(np.float64)
        num = p1abs if absolute else p1
        t[name] = dict(w=num / d, d1=(1.0 / d + num / (d * d) * passes) if absolute else (1.0 / d - p1 / (d * d) * passes),
                       d2=(num / (d * d) * passes) if absolute else (-p1 / (d * d) * passes))
    t["scale"] = 0.5 if (mode == "sca" and mut != "sca_is_sum") else 1.0
    t["hw"] = hw
    return t


def attn_fwd_on(a, b, mode, mut=None, absolute=False):
    t = attn_terms(a, b, mode, mut, absolute)
    A, B = (np.abs(a), np.abs(b)) if absolute else (a, b)
    r = 0.0
    for br, on in (("s", mode != "ca"), ("c", mode != "sa")):
        if on:
            wgt = t[br]["w"]
            r = r + wgt * A + ((1.0 + wgt) if absolute else (1.0 - wgt)) * B
    return r * t["scale"]


def attn_bwd_on(a, b, g, mode, mut=None, absolute=False):
    """(ga, gb) of attention_fusion (spatial 'l1', channel 'avg', clamp(min=eps)); derivation: oracle.fusion_oracle._attn_branch_bwd"""
    t = attn_terms(a, b, mode, mut, absolute)
    if absolute:
        G, diff = np.abs(g), np.abs(a) + np.abs(b)
    else:
        G, diff = g, a - b
    sgn = (lambda x: np.where(x >= 0, 1.0, -1.0)) if mut == "sign_zero_is_one" else np.sign
    if mut == "pool_without_abs":
        sgn = np.ones_like
    ga = gb = 0.0
    for br, on in (("s", mode != "ca"), ("c", mode != "sa")):
        if not on:
            continue
        wgt = t[br]["w"]
        gk = G * t["scale"]
        ga = ga + gk * wgt
        gb = gb + gk * ((1.0 + wgt) if absolute else (1.0 - wgt))
        if mut == "weights_constant":
            continue
        if br == "s":
            gw = (G * diff).sum(1, keepdims=True) * t["scale"]
            da, db = np.abs(sgn(a)), np.abs(sgn(b))
            if not absolute:
                da, db = sgn(a), sgn(b)
        else:
            gw = (G * diff).sum((2, 3), keepdims=True) * t["scale"]
            da = db = 1.0 / t["hw"]
        ga = ga + gw * t[br]["d1"] * da
        gb = gb + gw * t[br]["d2"] * db
    return ga + 0 * a, gb + 0 * a


def conditioning(a, b):
    """every denominator of the attention weights with its sum of absolute terms: [(sum, sum of |terms|, eps threshold)], spatial per pixel,
    channel per (n, channel) on the MEANS"""
    hw = a.shape[2] * a.shape[3]
    sp = (np.abs(a) + np.abs(b)).sum(1)
    ch, cha = (a + b).sum((2, 3)) / hw, (np.abs(a) + np.abs(b)).sum((2, 3)) / hw
    return (sp.ravel(), sp.ravel()), (ch.ravel(), cha.ravel())


def elem_weights(a, b, mode, mask, mut=None):
    """d out / d a, d out / d b of element fusion, times the ReLU masks of a and b"""
    if mode == "max":
        da = (a > b) + (1.0 if mut == "max_tie_one_zero" else 0.5) * (a == b)
        db = 1.0 - da
    else:
        da = db = np.full(a.shape, 1.0 if mode == "sum" else 0.5)
    if mask:
        da, db = da * relu_keep(a, mut), db * relu_keep(b, mut)
    return da, db


def halo_src(x, halo, mut=None):
    """the activation seen from every stored position of a halo-`halo` tensor"""
    if halo == 0:
        return x
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge" if mut == "clamped_halo_mask" else "reflect")


@dataclass
class Out:
    name: str
    want: np.ndarray          # the output buffer's stored domain; SENT where the call must leave the buffer alone
    bound: np.ndarray


def _bounded(c, want, A, K, old=None):
    b = K * U * A + (ULP * np.abs(want) if c.dtype == "bf16" else 0.0)
    if old is not None:
        b = b + U * (np.abs(old) + A)
    return b


def _grad_out(c, fresh, A, K, old, keep, mut):
    """an outgoing halo-1 gradient: interior = (old +) fresh, masked; the halo stays as it was"""
    use_old = c.acc and mut != "accumulate_ignores_old"
    want = (fresh + old if use_old else fresh) * keep
    exact = c.exact or (np.ndim(K) == 0 and K == 0 and not c.acc)
    bound = np.zeros_like(want) if exact else _bounded(c, want, A, K, old if c.acc else None) * keep
    return embed(want), np.pad(bound, ((0, 0), (0, 0), (1, 1), (1, 1)))


def define(c: Case, mut=None):
    """[Out] of everything the case's call writes, per output buffer"""
    o = operands(c)
    f64 = np.float64
    if c.k == "pool_fwd":
        y, _ = O.maxpool2x2_fwd(o["x"])
        return [Out("y", y, np.zeros(y.shape))]
    if c.k == "up_fwd":
        y = up_fwd_on(o["x"], *c.target, mut)
        return [Out("y", y, np.zeros(y.shape))]
    if c.k in ("pool_bwd", "up_bwd") and c.stride:          # small integers: every sum is exact; no bound to form
        fresh = pool_bwd_on(o["x"], o["g"]) if c.k == "pool_bwd" else up_bwd_on(o["g"], c.h, c.w)
        want = embed(fresh)
        return [Out("gx", want, np.zeros(want.shape))]
    if c.k in ("pool_bwd", "up_bwd"):
        g, gabs = logical(o["g"], c.g, mut=mut), logical(o["g"], c.g, True)
        if c.k == "pool_bwd":
            fresh, A, K = pool_bwd_on(o["x"], g, mut), pool_bwd_on(o["x"], gabs), c.K()
            keep = relu_keep(o["x"], mut) if c.mask else np.ones(fresh.shape)
        else:
            fresh, A = up_bwd_on(g, c.h, c.w, mut), up_bwd_on(gabs, c.h, c.w)
            K = c.K() + up_candidates(c)[None, None] - 1
            keep = relu_keep(o["xm"], mut) if c.mask else np.ones(fresh.shape)
        old = o["old"] if c.acc else None
        want, bound = _grad_out(c, fresh, A, K, old, keep, mut)
        return [Out("gx", want, bound)]
    if c.k == "relu_mask":
        want = o["g"] * relu_keep(halo_src(o["x"], c.halo, mut), mut)
        return [Out("g", want, np.zeros(want.shape))]
    if c.k == "attn_fwd":
        y, A = attn_fwd_on(o["a"].astype(f64), o["b"].astype(f64), c.mode, mut), attn_fwd_on(o["a"].astype(f64), o["b"].astype(f64), c.mode, None, True)
        return [Out("out", y, _bounded(c, y, A, c.K()))]
    if c.k == "attn_bwd":
        a, b = o["a"].astype(f64), o["b"].astype(f64)
        g, gabs = logical(o["g"], c.g, mut=mut).astype(f64), logical(o["g"], c.g, True).astype(f64)
        fa, fb = attn_bwd_on(a, b, g, c.mode, mut)
        Aa, Ab = attn_bwd_on(a, b, gabs, c.mode, None, True)
        one = np.ones(fa.shape)
        return [Out(nm, *_grad_out(c, f, A, c.K(), (old if c.acc else None), one, mut))
                for nm, f, A, old in (("ga", fa, Aa, o["old_a"]), ("gb", fb, Ab, o["old_b"]))]
    if c.k == "elem_fwd":
        y = O.element_fusion(o["a"], o["b"], c.mode)
        A = O.element_fusion(np.abs(o["a"]), np.abs(o["b"]), "sum" if c.mode == "max" else c.mode)
        return [Out("out", y, np.zeros(y.shape) if c.exact or c.stride else _bounded(c, y, A, c.K()))]
    if c.k == "elem_bwd":
        da, db = elem_weights(halo_src(o["a"], c.halo, mut), halo_src(o["b"], c.halo, mut), c.mode, c.mask, mut)
        outs = []
        for nm, d in (("ga", da), ("gb", db)):
            want = o["g"] * d
            outs.append(Out(nm, want, np.zeros(want.shape) if c.stride else _bounded(c, want, np.abs(want), c.K())))
        return outs
    if c.k == "to_blocked":
        v = np.zeros((c.n, c.C, c.h, c.w))
        v[:, :c.c] = rnd(o["src"], c.dtype)
        return [Out("dst", embed(v, c.halo), np.zeros((c.n, c.C, c.h + 2 * c.halo, c.w + 2 * c.halo)))]
    if c.k == "to_nchw":
        want, A = logical(o["g"], c.g, mut=mut)[:, :c.c], logical(o["g"], c.g, True)[:, :c.c]
        return [Out("dst", want, c.K() * U * A)]
    if c.k == "zero":
        z = np.zeros((c.n, c.C, c.h + 2 * c.halo, c.w + 2 * c.halo))
        return [Out("t", z, z.copy())]
    raise AssertionError(c.k)
