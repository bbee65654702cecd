"""Cases and fp64 definitions for the generic 3x3 / 1x1 ConvLayer kernels (csrc/conv_mfma.hip, csrc/conv_x3.hip, csrc/conv_valu.hip,
csrc/conv1x1.hip; dispatch in csrc/conv_route.hpp and csrc/conv_api.hip), and the library's own answer to "which kernel does this call
launch" (mmif_conv2d_route).  No GPU needed: tests/test_conv_oracle_cpu.py pins the definitions to torch's float64 autograd and the case list
to the dispatch; tests/test_gpu_conv_sweep.py runs every case on the device.

The definitions (all float64, on oracle.fusion_oracle):

* forward            y = relu?(b + corr(reflect_pad(x), w))
* dgrad, padded      gxp[n, c, 0:h+2, 0:w+2] = full scatter of g w  (O.conv2d_reflect_dgrad_padded)
* dgrad, folded      reflect_pad_adjoint(gxp, 1) in the interior, the ring at zero
* accumulate bits    bit i of accum_bits ADDS the old contents of channel block i (channels 8i..8i+7) -- gx's own, or gx_old's for
                     mmif_conv2d_reflect_dgrad_folded_onto
* mask bits          bit i of mask_bits THEN multiplies block i by [x > 0] (conv_epilogue: `c += old` precedes the mask; conv_api.hip:147
                     "fold(dgrad(gy)) + gx_old on the blocks in accum_bits, masked by mask_bits").  In the padded domain the mask of a ring
                     pixel is that of its reflected source, so that folding afterwards equals masking the folded gradient.
* wgrad              dw[o, c, u, v] = sum g xpad, db[o] = sum g; accumulate adds onto the previous values

bf16 families evaluate the definition on the bf16-rounded x, w, g (and old values) the kernel reads, so the ReLU mask has no near-zero ambiguity.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle import fusion_oracle as O

ALL = (1 << 64) - 1
M5A = 0x5a5a5a5a5a5a5a5a
M33 = 0x3333333333333333
BIT_SETS = (0, ALL, M5A, M33)
ALL_BITS = tuple((m, a) for m in BIT_SETS for a in BIT_SETS)          # every combination of mask_bits / accum_bits
FEW_BITS = ((M5A, M33), (ALL, ALL), (0, 0), (M33, 0))


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch, ASKED: mmif_conv2d_route (csrc/conv_api.hip) answers from the route functions the launches themselves go through
# (csrc/conv_route.hpp), on descriptors without data -- no GPU needed when num_cus is given
# ------------------------------------------------------------------------------------------------------------------------------
DEFAULT_SWITCHES = {"conv_dma": 1, "thin_wide": 1, "conv1x1_stream": 1, "wgrad_dma_blocks": 256}     # the mmif_debug_set_* switches


def pick_mf(n_out):
    return min(cdiv(n_out, 16), 4)


def pick_mfw(cout):
    return 1 if cout <= 16 else (2 if cout <= 32 else 4)


def pick_icf(ks, cin, cout):
    return (4 if cin > 32 else (2 if cin > 16 else 1)) if (ks == 1 and pick_mfw(cout) == 4) else 1


class switches:
    """the library's mmif_debug_set_* switches set to sw inside the block, back to their defaults after it"""

    def __init__(self, sw):
        self.sw = sw

    def _set(self, values):
        from mmif._lib import lib
        for k in self.sw:
            getattr(lib, "mmif_debug_set_" + k)(values[k])

    def __enter__(self):
        self._set(self.sw)

    def __exit__(self, *a):
        self._set(DEFAULT_SWITCHES)


def route(op, dtype, cin, cout, n, h, w, gy_folded=True, fold=False, mask_bits=0, accum_bits=0, num_cus=256, switches_=None, k=3, impl="auto",
          gy_halo=1, gx_halo=1):
    """What the library launches for the call (mmif.tensor.conv_route: name, G, slices, tiles, org), None where it would refuse.  op: 'fwd',
    'dgrad' (fold = the folded call), 'dgrad_onto', 'dgrad_dup', 'wgrad', 'bwd_pair', 'bwd_wide'.  dtype 'bf16' / 'f32'; impl 'auto' / 'mfma' /
    'x3' / 'valu'; num_cus = 0: the current device's."""
    from mmif import _lib as L
    from mmif import tensor as T

    def t(c, halo, folded=False):
        return L.MmifTensor(None, L.BF16 if dtype == "bf16" else L.F32, n, h, w, halo, cdiv(c, 8), 0, cdiv(c, 8), L.T_FOLDED if (halo and folded) else 0)
    if op == "fwd":
        a, b = t(cin, 0), t(cout, 0)
    elif op.startswith("dgrad"):
        a, b = t(cout, gy_halo, gy_folded), t(cin, gx_halo)
    else:
        a, b = t(cin, 0), t(cout, gy_halo, gy_folded)
    code = {"auto": L.IMPL_AUTO, "mfma": L.IMPL_MFMA, "x3": L.IMPL_X3, "valu": L.IMPL_VALU}[impl]
    with switches(switches_ or {}):
        return T.conv_route(op, a, b, cin, cout, k, mask_bits, accum_bits, fold, code, num_cus)


def expected_kernel(op, dtype, cin, cout, n, h, w, gy_folded=True, fold=False, mask_bits=0, accum_bits=0, num_cus=256, switches=None, k=3,
                    impl="auto", gy_halo=1, gx_halo=1):
    """Name of the kernel the library launches ('none': it would refuse the call); for 'bwd_wide' the input-gradient half (its
    weight-gradient half is always wgrad_dma)."""
    r = route(op, dtype, cin, cout, n, h, w, gy_folded, fold, mask_bits, accum_bits, num_cus, switches, k, impl, gy_halo, gx_halo)
    return r.name if r is not None else "none"


# The fp32 split-operand family (csrc/conv_x3.hip), one name per code object.  Forward kernels exist per operand format (h16: two scaled fp16
# pieces, b3 / b2: three / two bf16 pieces -- mmif_set_x3_forward_pieces(16 | 3 | 2)); the input gradient always reads two bf16 pieces.
X3_FORMATS = (16, 3, 2)
X3_LABELS = (["x3<%d,mb%d,%s>" % (k, mb, f) for k in (1, 3) for mb in (2, 1) for f in ("h16", "b3", "b2") if (k, mb, f) != (3, 1, "b3")]
             + ["x3<3,mb1,b3,rj4>"] + ["x3<3,mb1,%s,nw4%s>" % (f, m) for f in ("h16", "b2") for m in ("", ",m16")]
             + ["x3_dgrad<1,mb2>", "x3_dgrad<1,mb1>", "x3_dgrad<3,mb2>", "x3_dgrad<3,mb1>", "x3_dgrad<3,mb1,nw4>", "x3_dgrad<3,mb1,nw4,m16>"]
             + ["x3_wgrad<1>", "x3_wgrad<3>"] + ["x3_wgrad_thin<%d>" % c for c in (2, 4, 6)])
# No legal call reaches it on a part with <= 256 compute units (every gfx950 part): the route takes wgrad_x3_kernel<16,6,2,3> only where the
# thin kernel's partials (up to 5 blocks per CU x 6976 floats) outgrow the workspace of 256 partials of 36928 floats, i.e. past 270
# compute units.  tests/test_conv_oracle_cpu.py proves both halves on a grid of shapes.
UNREACHABLE = {"x3_wgrad_thin16"}

# every kernel name the sweep must reach (tests/test_conv_oracle_cpu.py fails on an unreached one)
REQUIRED_LABELS = (["mfma<3,%d>" % m for m in (1, 2, 3, 4)] + ["mfma<1,%d>" % m for m in (2, 3, 4)] + ["conv1x1_stream"]
                   + ["conv_dma<L0,org0>", "conv_dma<L0,org1>", "conv_dma<L1,org0>", "conv_dma<L1,org1>", "conv_dma<L2,org1>", "conv_dma<L0,org1,dup>"]
                   + ["thin_async<1>", "thin_async<2>", "thin_async<3>", "thin_wide", "wgrad_dma", "wgrad_taprow"]
                   + ["wgrad_mfma<3,%d>" % m for m in (1, 2, 4)] + ["wgrad_mfma<1,4,2,%d>" % i for i in (1, 2, 4)] + ["bwd_pair", "valu"] + X3_LABELS)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    label: str            # the kernel the case is meant to reach at num_cus = 256 (x3 forward: in the default operand format, h16)
    op: str               # fwd | dgrad | dgrad_onto | wgrad | bwd_pair | bwd_wide | dgrad_dup
    cin: int
    cout: int
    n: int
    h: int
    w: int
    k: int = 3
    dtype: str = "bf16"
    impl: str = "mfma"
    fold: bool = False                # dgrad: the folded call
    gy_folded: bool = True            # gy is a folded halo-1 gradient (zero ring); False: a padded-domain gradient the kernel folds on load
    gy_halo: int = 1
    gx_halo: int = 1
    bits: tuple = ((0, 0),)           # (mask_bits, accum_bits) pairs run on the one set of operands
    accumulate: tuple = (0,)          # wgrad family: accumulate flags run
    relu: bool = True
    slot: tuple = (0, 0)              # channel blocks before / after the output view inside a wider buffer
    switches: tuple = ()              # (name, value) pairs of mmif_debug_set_* switches
    phases: bool = False              # bwd_wide: the two halves as two calls as well
    note: str = ""

    @property
    def id(self):
        head = "x3" if self.impl == "x3" else self.label      # (the x3 ids name the family: they predate the per-kernel labels)
        s = f"{head}-{self.op}{'F' if self.fold else ''}-{self.dtype}-{self.cin}to{self.cout}k{self.k}-{self.n}x{self.h}x{self.w}"
        if not self.gy_folded:
            s += "-gyraw"
        if self.gy_halo == 0:
            s += "-gyh0"
        if self.switches:
            s += "-" + "_".join(f"{a}{b}" for a, b in self.switches)
        return s + (("-" + self.note) if self.note else "")

    @property
    def sw(self):
        return dict(self.switches)

    def route(self, num_cus=256, mask_bits=None, accum_bits=None):
        """what the library launches for this case under its switches (see route())"""
        m, a = self.bits[0] if mask_bits is None else (mask_bits, accum_bits)
        cbm = (1 << cdiv(self.cin, 8)) - 1
        return route(self.op, self.dtype, self.cin, self.cout, self.n, self.h, self.w, self.gy_folded, self.fold, m & cbm, a & cbm, num_cus, self.sw,
                     self.k, self.impl, self.gy_halo, self.gx_halo)

    def expected(self, num_cus=256, mask_bits=None, accum_bits=None):
        r = self.route(num_cus, mask_bits, accum_bits)
        return r.name if r is not None else "none"

    def x3_forward_labels(self, num_cus=256):
        """{operand format: kernel} of an x3 forward case: the sweep runs it in each of the three (the process mode is put back afterwards)"""
        from mmif._lib import lib
        prev = lib.mmif_get_x3_forward_pieces()
        try:
            out = {}
            for pieces in X3_FORMATS:
                lib.mmif_set_x3_forward_pieces(pieces)
                out[pieces] = self.expected(num_cus)
            return out
        finally:
            lib.mmif_set_x3_forward_pieces(prev)


NO_DMA = (("conv_dma", 0),)
REG_MAPS = [(33, 40), (16, 16), (17, 17), (15, 31), (2, 9), (9, 2), (3, 3), (4, 4), (5, 7)]
REG_CH = [(16, 16), (24, 24), (40, 40), (72, 72), (20, 12), (13, 21)]     # (cin, cout): MF 1..4 both ways + ragged last channel blocks


def _cases():
    cs = []
    # ---- register-staged conv_mfma_kernel<3, MF>: forward, padded-domain dgrad, folded call (dgrad + stand-alone fold kernel)
    for cin, cout in REG_CH:
        for h, w in REG_MAPS:
            cs.append(Case(f"mfma<3,{pick_mf(cout)}>", "fwd", cin, cout, 3, h, w, switches=NO_DMA))
            for fold in (False, True):
                cs.append(Case(f"mfma<3,{pick_mf(cin)}>", "dgrad", cin, cout, 3, h, w, fold=fold, bits=ALL_BITS, switches=NO_DMA))
        # a padded-domain gy (non-zero ring): the kernel folds it while loading
        cs.append(Case(f"mfma<3,{pick_mf(cin)}>", "dgrad", cin, cout, 3, 33, 40, gy_folded=False, bits=FEW_BITS, switches=NO_DMA))
        cs.append(Case(f"mfma<3,{pick_mf(cin)}>", "dgrad", cin, cout, 2, 5, 7, gy_halo=0, bits=FEW_BITS, switches=NO_DMA))
    # ---- conv_dma_kernel (16 x 32 tiles)
    dma_maps = [(1, 32, 16), (3, 33, 17), (1, 31, 15), (1, 64, 48), (3, 4, 4), (1, 5, 7)]
    for cin, cout in [(8, 64), (32, 72), (40, 136), (72, 64)]:
        for n, h, w in dma_maps:
            cs.append(Case("conv_dma<L0,org0>", "fwd", cin, cout, n, h, w))
    for n, h, w in dma_maps:
        cs.append(Case("conv_dma<L0,org1>", "dgrad", 72, 64, n, h, w, fold=True, bits=((0, M33), (0, 0), (0, ALL)), note="nomask"))
        cs.append(Case("conv_dma<L1,org1>", "dgrad", 64, 72, n, h, w, fold=True, bits=((M5A, M33), (ALL, 0), (M33, ALL))))
        cs.append(Case("conv_dma<L1,org1>", "dgrad", 136, 40, n, h, w, fold=True, bits=((M5A, M33), (ALL, ALL))))
        cs.append(Case("conv_dma<L0,org1>", "dgrad", 64, 32, n, h, w, fold=True, bits=((M5A, M33), (ALL, 0)), note="consumers-fetch-mask"))
        cs.append(Case("conv_dma<L0,org1>", "dgrad", 72, 8, n, h, w, fold=True, bits=((M5A, M33), (ALL, ALL)), note="consumers-fetch-mask"))
    for n, h, w in [(3, 33, 17), (1, 5, 7), (2, 3, 5), (2, 5, 3)]:      # org 0: the unfolded call, and the folded call at h = 3 / w = 3
        fold = h == 3 or w == 3
        cs.append(Case("conv_dma<L0,org0>", "dgrad", 72, 64, n, h, w, fold=fold, bits=((0, M33), (0, 0))))
        cs.append(Case("conv_dma<L1,org0>", "dgrad", 64, 72, n, h, w, fold=fold, bits=((M5A, M33), (ALL, 0))))
        cs.append(Case("conv_dma<L0,org0>", "dgrad", 64, 32, n, h, w, fold=fold, bits=((M5A, M33),), note="consumers-fetch-mask"))
    # ---- thin_conv_async_kernel: >= 2 * 256 tiles.  8x128x128 = exactly 512; 9x105x131 = 567 (odd: a short last round, tiles of different
    # images in one block); 2x256x257 = 544; 73x16x112 = 511 tiles stays on the register-staged kernel
    for cin, cout, n, h, w in [(40, 24, 8, 128, 128), (40, 32, 9, 105, 131), (8, 32, 2, 256, 257), (32, 40, 8, 128, 128), (32, 48, 9, 105, 131),
                               (24, 40, 9, 121, 125)]:
        cs.append(Case(f"thin_async<{pick_mf(cout)}>", "fwd", cin, cout, n, h, w))
    cs.append(Case("mfma<3,2>", "fwd", 40, 24, 73, 16, 112, note="511tiles"))
    cs.append(Case("mfma<3,3>", "dgrad", 40, 32, 73, 16, 112, fold=True, bits=((M5A, M33),), note="511tiles"))
    for cin, cout, n, h, w in [(16, 48, 8, 128, 128), (24, 40, 9, 105, 131), (40, 32, 2, 256, 257), (40, 32, 8, 128, 128), (16, 16, 9, 121, 125)]:
        cs.append(Case(f"thin_async<{pick_mf(cin)}>", "dgrad", cin, cout, n, h, w, fold=True, bits=((M5A, M33), (ALL, 0))))
        cs.append(Case(f"thin_async<{pick_mf(cin)}>", "dgrad_onto", cin, cout, n, h, w, fold=True, bits=((M5A, M33), (0, ALL))))
    cs.append(Case("thin_async<2>", "dgrad", 24, 40, 8, 128, 128, fold=False, bits=((M5A, M33),), note="padded-domain"))   # org 0: 9x9 tiles of the 130x130 stored map
    # ---- the wide 64 -> 32 forward geometry, output slot inside a wider buffer
    cs.append(Case("thin_wide", "fwd", 64, 32, 8, 128, 128, slot=(1, 1)))
    cs.append(Case("thin_wide", "fwd", 56, 24, 3, 250, 180, slot=(1, 2)))
    # ---- weight gradients
    for acc in ((0, 1),):
        for cin, cout, n, h, w in [(64, 136, 3, 33, 17), (304, 152, 2, 33, 40), (304, 152, 1, 16, 16), (64, 64, 1, 16, 16), (128, 64, 1, 64, 48)]:
            cs.append(Case("wgrad_dma", "wgrad", cin, cout, n, h, w, accumulate=acc))
        cs.append(Case("wgrad_dma", "wgrad", 64, 136, 3, 33, 17, accumulate=acc, switches=(("wgrad_dma_blocks", 64),)))
        cs.append(Case("wgrad_dma", "wgrad", 128, 64, 1, 64, 48, accumulate=acc, switches=(("wgrad_dma_blocks", 64),)))
        for cin, cout in [(16, 16), (48, 16), (32, 32), (64, 32)]:
            for n, h, w in [(3, 33, 40), (1, 16, 16), (2, 5, 7)]:
                cs.append(Case("wgrad_taprow", "wgrad", cin, cout, n, h, w, accumulate=acc))
        for cin, cout in [(20, 12), (13, 21), (72, 64), (40, 40)]:
            for n, h, w in [(3, 33, 40), (1, 16, 16), (2, 2, 9), (3, 17, 17)]:
                cs.append(Case(f"wgrad_mfma<3,{pick_mfw(cout)}>", "wgrad", cin, cout, n, h, w, accumulate=acc))
        for cin, cout in [(8, 64), (24, 40), (88, 64)]:
            for n, h, w in [(3, 33, 40), (1, 16, 16)]:
                cs.append(Case(f"wgrad_mfma<1,4,2,{pick_icf(1, cin, cout)}>", "wgrad", cin, cout, n, h, w, k=1, accumulate=acc))
    # ---- one-launch backward of a thin layer / of a wide layer, straight against the definition
    for cin, cout in [(64, 32), (32, 16)]:
        for n, h, w in [(3, 33, 40), (1, 4, 4), (1, 64, 48)]:
            cs.append(Case("bwd_pair", "bwd_pair", cin, cout, n, h, w, bits=((ALL, 0),), accumulate=(0, 1)))
    for cin, cout in [(64, 64), (128, 64), (64, 128)]:
        for n, h, w in [(3, 33, 17), (1, 4, 4), (1, 64, 48)]:
            cs.append(Case("conv_dma<L2,org1>", "bwd_wide", cin, cout, n, h, w, bits=((ALL, 0), (M5A, 0)), accumulate=(0, 1), phases=(h == 33)))
    cs.append(Case("conv_dma<L0,org1>", "bwd_wide", 64, 64, 3, 33, 17, bits=((0, 0),), note="nomask"))
    for n, h, w in [(2, 33, 40), (1, 4, 4), (1, 64, 48)]:
        cs.append(Case("conv_dma<L0,org1,dup>", "dgrad_dup", 64, 64, n, h, w, fold=True))
    # ---- fp32 tensors: the split-operand (x3) and the fp32 FMA (valu) kernels; one map per tile-edge class
    x3 = {(16, 16): ("x3<3,mb1,h16,nw4,m16>", "x3_dgrad<3,mb1,nw4,m16>", "x3_wgrad_thin<2>"), (48, 16): ("x3<3,mb1,h16,nw4,m16>", "x3_dgrad<3,mb2>", "x3_wgrad_thin<6>"),
          (72, 64): ("x3<3,mb2,h16>", "x3_dgrad<3,mb2>", "x3_wgrad<3>"), (13, 21): ("x3<3,mb1,h16,nw4>", "x3_dgrad<3,mb1,nw4,m16>", "x3_wgrad<3>")}
    for impl in ("x3", "valu"):
        for cin, cout in [(16, 16), (48, 16), (72, 64), (13, 21)]:
            lf, ld, lw = x3[cin, cout] if impl == "x3" else (impl,) * 3
            for n, h, w in [(2, 33, 40), (1, 16, 16), (2, 17, 17), (2, 2, 9), (1, 3, 3), (2, 5, 7)]:
                cs.append(Case(lf, "fwd", cin, cout, n, h, w, dtype="f32", impl=impl))
                cs.append(Case(ld, "dgrad", cin, cout, n, h, w, dtype="f32", impl=impl, fold=True, bits=FEW_BITS))
                cs.append(Case(lw, "wgrad", cin, cout, n, h, w, dtype="f32", impl=impl, accumulate=(0, 1)))
            cs.append(Case(ld, "dgrad", cin, cout, 2, 33, 40, dtype="f32", impl=impl, fold=False, bits=FEW_BITS))
    for cin, cout in [(72, 64), (13, 21)]:      # x3 dgrad masked by the sign map its weight gradient leaves
        cs.append(Case(x3[cin, cout][1], "bwd_wide", cin, cout, 2, 33, 40, dtype="f32", impl="x3", bits=((ALL, 0), (M5A, 0)), accumulate=(0, 1)))
    # ---- 1x1 layers
    for cin, cout in [(8, 64), (88, 64), (24, 40)]:
        for n, h, w in [(3, 33, 40), (1, 16, 16), (2, 5, 7)]:
            cs.append(Case("conv1x1_stream", "fwd", cin, cout, n, h, w, k=1))
            cs.append(Case("conv1x1_stream", "dgrad", cin, cout, n, h, w, k=1, gy_halo=0, gx_halo=0, bits=((M5A, 0), (0, 0))))
            # accumulate bits: the streaming kernel declines, conv_mfma_kernel<1, MF> runs
            cs.append(Case(f"mfma<1,{pick_mf(cin)}>", "dgrad", cin, cout, n, h, w, k=1, gy_halo=0, gx_halo=0, bits=((M5A, M33), (0, ALL))))
    for cin, cout in [(40, 24), (24, 40), (88, 64)]:
        cs.append(Case(f"mfma<1,{pick_mf(cout)}>", "fwd", cin, cout, 3, 33, 40, k=1, switches=(("conv1x1_stream", 0),)))
    # ---- the x3 kernels the four fp32 layers above do not reach (last: the cases before them keep their places), on the tile-edge maps (1x3x3: the folded dgrad below h = 4 leaves the fold to the
    # stand-alone kernel): eight-wave blocks at <= 32 outputs (> 64 inputs), the four-wave dgrad at 17..32 outputs, the 17..32-input thin
    # weight gradient, and every 1x1 kernel
    f32 = dict(dtype="f32", impl="x3")
    for n, h, w in [(2, 33, 40), (2, 5, 7)]:
        cs.append(Case("x3<3,mb1,h16>", "fwd", 72, 24, n, h, w, **f32))
        cs.append(Case("x3_wgrad_thin<4>", "wgrad", 24, 12, n, h, w, accumulate=(0, 1), **f32))
    for n, h, w in [(2, 33, 40), (2, 5, 7), (1, 3, 3)]:
        cs.append(Case("x3_dgrad<3,mb1>", "dgrad", 24, 72, n, h, w, fold=True, bits=FEW_BITS, **f32))
        cs.append(Case("x3_dgrad<3,mb1,nw4>", "dgrad", 24, 40, n, h, w, fold=True, bits=FEW_BITS, **f32))
    for n, h, w in [(2, 33, 40), (2, 5, 7)]:
        for cin, cout in [(24, 40), (88, 64)]:
            cs.append(Case("x3<1,mb2,h16>", "fwd", cin, cout, n, h, w, k=1, **f32))
            cs.append(Case(f"x3_dgrad<1,mb{2 if cin > 32 else 1}>", "dgrad", cin, cout, n, h, w, k=1, gy_halo=0, gx_halo=0, bits=FEW_BITS, **f32))
            cs.append(Case("x3_wgrad<1>", "wgrad", cin, cout, n, h, w, k=1, accumulate=(0, 1), **f32))
        cs.append(Case("x3<1,mb1,h16>", "fwd", 40, 24, n, h, w, k=1, **f32))
    return cs


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


# ------------------------------------------------------------------------------------------------------------------------------
# operands and definitions
# ------------------------------------------------------------------------------------------------------------------------------
def rnd(a, dtype):
    """the values a tensor of the case's dtype holds, as float64"""
    a = np.asarray(a, np.float32)
    return (O.bf16_round(a) if dtype == "bf16" else a).astype(np.float64)


@dataclass
class Operands:
    x: np.ndarray
    w: np.ndarray         # what the kernel multiplies with: bf16-rounded for the bf16 families (packed operand images are bf16)
    w32: np.ndarray       # the fp32 master weights handed to the library
    b: np.ndarray
    g: np.ndarray         # upstream gradient, logical [n, cout, h, w] (for gy_folded=False cases: the fold of gp)
    gp: np.ndarray        # stored gradient [n, cout, h+2*halo, w+2*halo]
    old: np.ndarray       # previous contents of gx (stored extent)
    dw_old: np.ndarray
    db_old: np.ndarray
    F: np.ndarray = None  # dgrad_dup: the 128-channel activations whose blocks 6, 7 / 14, 15 mask the copies
    key: tuple = ()


_OPS = {}      # the last few operand sets / definitions only: cases that share one are neighbours in CASES
_KEEP = 3


def _put(d, key, val):
    d[key] = val
    while len(d) > _KEEP * (1 if d is _OPS else 4):
        d.pop(next(iter(d)))
    return val


def operands(c: Case) -> Operands:
    key = (c.dtype, c.cin, c.cout, c.k, c.n, c.h, c.w, c.gy_folded, c.gy_halo, c.gx_halo, c.op == "dgrad_dup")
    if key in _OPS:
        return _OPS[key]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    x = rnd(rng.standard_normal((c.n, c.cin, c.h, c.w)), c.dtype)
    w32 = (rng.standard_normal((c.cout, c.cin, c.k, c.k)) * 0.05).astype(np.float32)
    w = rnd(w32, c.dtype)
    b = rng.standard_normal(c.cout).astype(np.float32).astype(np.float64)
    hg = c.gy_halo
    gp = rnd(rng.standard_normal((c.n, c.cout, c.h + 2 * hg, c.w + 2 * hg)), c.dtype)
    if hg and c.gy_folded:
        ring = np.ones(gp.shape[2:], bool)
        ring[1:-1, 1:-1] = False
        gp[:, :, ring] = 0.0
    if hg and not c.gy_folded:      # the kernel folds a padded-domain gy while loading: "fp32 fold, rounded once" (csrc/conv_mfma.hip load_in_gradfold)
        g = rnd(O.reflect_pad_adjoint(gp, 1), c.dtype)
    else:
        g = gp[:, :, 1:-1, 1:-1] if hg else gp
    hx = c.gx_halo
    old = rnd(rng.standard_normal((c.n, c.cin, c.h + 2 * hx, c.w + 2 * hx)), c.dtype)
    dw_old = (rng.standard_normal(w.shape) * np.sqrt(c.n * c.h * c.w)).astype(np.float32).astype(np.float64)
    db_old = (rng.standard_normal(c.cout) * np.sqrt(c.n * c.h * c.w)).astype(np.float32).astype(np.float64)
    F = rnd(rng.standard_normal((c.n, 128, c.h, c.w)), c.dtype) if c.op == "dgrad_dup" else None
    return _put(_OPS, key, Operands(x, w, w32, b, np.ascontiguousarray(g), gp, old, dw_old, db_old, F, key))


def block_mask(bits, channels):
    """per-channel 0/1 vector of a 64-bit channel-block set"""
    return np.array([(bits >> (ch // 8)) & 1 for ch in range(channels)], np.float64)


def ring_zero(a):
    a = a.copy()
    a[:, :, 0] = 0
    a[:, :, -1] = 0
    a[:, :, :, 0] = 0
    a[:, :, :, -1] = 0
    return a


_DEF = {}


def _cached(key, fn):
    if key not in _DEF:
        _put(_DEF, key, fn())
    return _DEF[key]


def def_fwd(c: Case):
    """(y, S): the definition and the same sum on |operands| (the scale of the fp32 accumulation error)"""
    o = operands(c)

    def go():
        y = O.conv2d_reflect_fwd(o.x, o.w, o.b, c.relu)
        S = O.conv2d_reflect_fwd(np.abs(o.x), np.abs(o.w), np.abs(o.b), False)
        return y, S
    return _cached(("fwd", o.key, c.relu), go)


def def_dgrad_padded(c: Case):
    """(gxp, Sp) on the stored extent of gx: padded domain for k = 3 with a halo, the plain map for halo 0 / 1x1 inside its ring"""
    o = operands(c)

    def go():
        gxp = O.conv2d_reflect_dgrad_padded(o.g, o.w)
        Sp = O.conv2d_reflect_dgrad_padded(np.abs(o.g), np.abs(o.w))
        return gxp, Sp
    return _cached(("gxp", o.key), go)


def def_dgrad(c: Case, mask_bits, accum_bits, old=None):
    """Definition of one dgrad call on gx's stored extent [n, cin, h+2*halo, w+2*halo]: returns (ref, S, parts) -- parts = the padded-domain
    values before the fold (None where nothing is folded), for the rounding bound of the dgrad + stand-alone-fold path.
    Folded call: interior = (fold(gxp) + old) * mask, ring = 0.  Padded call: (gxp + old) * reflect_pad(mask)."""
    o = operands(c)
    old = o.old if old is None else old
    gxp, Sp = def_dgrad_padded(c)
    am = block_mask(accum_bits, c.cin)[None, :, None, None]
    mm = block_mask(mask_bits, c.cin)[None, :, None, None]
    pos = (o.x > 0).astype(np.float64)
    p = c.k // 2
    hx = c.gx_halo
    if c.k == 1 or hx == 0:          # nothing outside the interior is computed; a halo ring (1x1 with halo 1) keeps its contents
        core = gxp if p == 0 else O.reflect_pad_adjoint(gxp, p)
        Score = Sp if p == 0 else O.reflect_pad_adjoint(Sp, p)
        keep = 1 - mm + mm * pos
        ref = old.copy()
        S = np.abs(old).copy()
        inner = (slice(None), slice(None), slice(hx, hx + c.h), slice(hx, hx + c.w))
        ref[inner] = (core + am * old[inner]) * keep
        S[inner] = Score + am * np.abs(old[inner])
        return ref, S, None
    keep_p = 1 - mm + mm * O.reflect_pad(pos, 1)
    if not c.fold:
        return (gxp + am * old) * keep_p, Sp + am * np.abs(old), None
    oldz = ring_zero(old)            # the folded call's contract: gx's ring is zero on entry
    parts = (gxp + am * oldz) * keep_p
    ref = np.zeros_like(gxp)
    ref[:, :, 1:-1, 1:-1] = O.reflect_pad_adjoint(parts, 1)
    S = np.zeros_like(gxp)
    S[:, :, 1:-1, 1:-1] = O.reflect_pad_adjoint(Sp + am * np.abs(oldz), 1)
    A_fold = np.zeros_like(gxp)
    A_fold[:, :, 1:-1, 1:-1] = O.reflect_pad_adjoint(np.abs(parts), 1)
    return ref, S, A_fold


def def_wgrad(c: Case, accumulate):
    o = operands(c)

    def go():
        _, gw, gb = O.conv2d_reflect_bwd(o.x, o.w, None, o.g, relu=False, need_gx=False)
        return gw, gb
    gw, gb = _cached(("wgrad", o.key), go)
    return (gw + o.dw_old, gb + o.db_old) if accumulate else (gw, gb)


def K_terms(c: Case):
    """number of products accumulated into one output"""
    return c.k * c.k * (c.cin if c.op == "fwd" else c.cout)


def bf16_bound(c: Case, A, S, extra_terms=2):
    """|got - ref| <= 2^-8 A + (K + 2) 2^-24 S: A = the sum of the magnitudes of the values the path stores in bf16 on the way to this element
    (one round-to-nearest each: half an ulp of an 8-bit significand is 2^-8 of the value just above a power of two, 2^-9 just below the next --
    2^-8 is attained, the bound has no slack there), S = the same sum on |operands| (+ |b| / |old|), K = the number of fp32-accumulated terms
    (bf16 x bf16 products are exact in fp32; each addition rounds to 2^-24 of a partial sum that S bounds)."""
    return 2.0 ** -8 * A + (K_terms(c) + extra_terms) * 2.0 ** -24 * S
