"""Golden F23: the BITS of every weight gradient whose per-block partial sums go through the fixed-order reduce of csrc/wgrad_reduce.hpp.

The suite holds dW / db to fp64 definitions within tolerances; that catches a wrong map, not a changed summation order.  This table of direct
calls through mmif.tensor is run once on a reference build (tests/golden/make_golden_wgrad_bits.py -> tests/golden/f23_wgrad_bits.json: a
SHA-256 per output) and again by tests/test_gpu_wgrad_bits.py on the tree's library.  Operands come from conv_cases.operands() or the same
kind of seeded numpy generator; nothing is drawn on the device.

Every reduce flavour (map type / slice count SL) is reached with accumulate 0 and 1, with db wanted and -- where the wrapper takes None --
not wanted, and in both regimes of the sum of G partials in SL slices (partial_sum(): four chains over g, g + SL, g + 2 SL, g + 3 SL, then a
tail):
    tail        G <= 3 SL                       the main loop never runs
    main+tail   G > 4 SL and G mod 4 SL != 0    main loop, then a tail of another length in some slices
The flavours whose SL follows G (wgrad_dma, wgrad_x3: SL = 16 if G > 64 else 4) cannot reach `tail` at SL 16 (G > 64 > 48).

The ConvLayer calls' G, bf16 and fp32 (x3), comes from the library (mmif_conv2d_route at 256 compute units: the route the launch itself
takes); the image, encoder and dense x3 kernels' G is not exported and is derived below from their launchers' formulas (for 256 compute
units where the formula has them; the shapes here keep G = the tile count, below every such cap).  tests/test_wgrad_bits_cpu.py checks both.
Shapes are the smallest that reach the regime: 16 x 16-tile producers run 2 x 33 x 40 (18 tiles), 1 x 33 x 40 (9) and 3 x 80 x 96 (90).
"""
from __future__ import annotations

import hashlib
import zlib
from dataclasses import dataclass

import numpy as np

import conv_cases as CC
from conv_cases import cdiv

NUM_CUS = 256           # the G column holds for this compute-unit count (the golden file records the device's)


def regime(G, sl):
    return "tail" if G <= 3 * sl else ("main+tail" if G > 4 * sl and G % (4 * sl) else "other")


def tiles(n, h, w, th, tw):
    return n * cdiv(h, th) * cdiv(w, tw)


# ------------------------------------------------------------------------------------------------------------------------------
# G of every launcher (csrc/conv_mfma.hip, conv_x3.hip, conv_image.hip, image_bwd.hip, enc_wgrad.hip, enc_bwd.hip)
# ------------------------------------------------------------------------------------------------------------------------------
def sl_by_G(G):
    return 16 if G > 64 else 4


def _G(op, kernel, cin, cout, k, n, h, w, dtype="bf16"):
    """G of the library's route for the call, which must be the kernel the caller means"""
    r = CC.route(op, dtype, cin, cout, n, h, w, k=k, impl="mfma" if dtype == "bf16" else "x3", num_cus=NUM_CUS)
    assert r is not None and r.name.startswith(kernel), (op, kernel, cin, cout, k, n, h, w, r)
    return r.G


def G_dma(cin, cout, n, h, w):
    return _G("wgrad", "wgrad_dma", cin, cout, 3, n, h, w)


def G_mfma(cin, cout, k, n, h, w):
    return _G("wgrad", "wgrad_mfma", cin, cout, k, n, h, w)


def G_taprow(cin, cout, n, h, w):
    return _G("wgrad", "wgrad_taprow", cin, cout, 3, n, h, w)


def G_pair(cin, n, h, w):
    return _G("bwd_pair", "bwd_pair", cin, cin // 2, 3, n, h, w)


def G_x3(cin, cout, k, n, h, w):
    """the reduce's G: the 1x1 kernel leaves three k-split partials per block"""
    return _G("wgrad", f"x3_wgrad<{k}>", cin, cout, k, n, h, w, "f32")


def G_x3_thin(cin, n, h, w, cout=16):
    return _G("wgrad", "x3_wgrad_thin<", cin, cout, 3, n, h, w, "f32")


def G_x3_dense(n, h, w):
    """mmif_dense_encoder_wgrad on fp32 tensors is no ConvLayer call: mmif_conv2d_route has no op for it (x3_dense_G, csrc/conv_route.hpp:
    two blocks per compute unit, at most 512, at most one per 8 x 16 tile)"""
    return min(min(2 * NUM_CUS, 512), tiles(n, h, w, 8, 16))


def G_image(n, h, w):
    return min(cdiv(n * h * w, 256), 512)


def G_image_bwd(n, h, w):
    G = min(tiles(n, h, w, 8, 32), 512)
    return G // 8 * 8 if G >= 8 else G


def G_enc_bwd(n, h, w, nb):
    """fb_geometry() of csrc/enc_bwd.hip: blocks per branch"""
    FB_W, FB_PAIRS = 32, 4
    keep = FB_W - 6
    nstrips = 1 if w <= FB_W - 2 else (w - (FB_W - 2) + keep - 1) // keep + 1
    cols = n * nstrips
    line_rows = cols * h
    gmax = max(1, min(NUM_CUS // nb, 256))

    def pos_of(v, cost):
        hv = h + cost
        c, y = divmod(v, hv)
        return min(c * h + min(y, h), line_rows)

    def steps(y_lo, y_hi):
        a_lo = max(y_lo - 3, 0)
        return 3 * ((y_hi + 2 - (a_lo - 3) + 2) // 3)

    best = None
    for cost in range(0, 13, 2):
        weighted = cols * (h + cost)
        rps = max(8 + cost, cdiv(weighted, gmax * FB_PAIRS))
        nblocks = cdiv(weighted, rps * FB_PAIRS)
        worst = 0
        for slot in range(nblocks * FB_PAIRS):
            pos, end, bars = pos_of(slot * rps, cost), pos_of((slot + 1) * rps, cost), 0
            while pos < end:
                y_lo = pos % h
                y_hi = min(h, y_lo + (end - pos))
                bars += 1 + steps(y_lo, y_hi)
                pos += y_hi - y_lo
            worst = max(worst, bars)
        if best is None or worst < best[0]:
            best = (worst, nblocks)
    return best[1]


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BitsCase:
    op: str                 # the mmif.tensor entry point (see run())
    reduces: tuple          # ((flavour, G, SL), ...) of the reduce launches the call makes
    n: int
    h: int
    w: int
    cin: int = 0
    cout: int = 0
    k: int = 3
    dtype: str = "bf16"
    accumulate: int = 0
    db: bool = True
    note: str = ""

    @property
    def id(self):
        ch = f"-{self.cin}to{self.cout}k{self.k}" if self.cin else (f"-k{self.k}" if self.op.startswith("image") else "")
        return (f"{self.op}-{self.dtype}{ch}-{self.n}x{self.h}x{self.w}-acc{self.accumulate}" + ("" if self.db else "-nodb")
                + (("-" + self.note) if self.note else ""))


S9, S18, S90 = (1, 33, 40), (2, 33, 40), (3, 80, 96)       # 9 / 18 / 90 tiles of 16 x 16


def _variants(cs, op, reduces_of, shapes, nodb=True, **kw):
    """accumulate 0 and 1 at every shape, and db = None once (at the last shape, accumulate 0)"""
    for i, s in enumerate(shapes):
        for acc in (0, 1):
            cs.append(BitsCase(op, reduces_of(*s), *s, accumulate=acc, **kw))
        if nodb and i == len(shapes) - 1:
            cs.append(BitsCase(op, reduces_of(*s), *s, accumulate=0, db=False, **kw))


def _cases():
    cs = []

    def dma(cin, cout):
        def f(n, h, w):
            G = G_dma(cin, cout, n, h, w)
            return ((f"wgrad_dma_reduce/{sl_by_G(G)}", G, sl_by_G(G)),)
        return f

    def mfma(cin, cout, k):
        name = f"wgrad_mfma_reduce<{k},{CC.pick_mfw(cout)},{CC.pick_icf(k, cin, cout)}>/4"
        return lambda n, h, w: ((name, G_mfma(cin, cout, k, n, h, w), 4),)

    def x3(cin, cout, k):
        def f(n, h, w):
            G = G_x3(cin, cout, k, n, h, w)
            return ((f"wgrad_x3_reduce<taps {k * k}>/{sl_by_G(G)}", G, sl_by_G(G)),)
        return f

    taprow = lambda n, h, w: (("taprow_wgrad_reduce/16", G_taprow(48, 16, n, h, w), 16),)
    # ---- conv_wgrad, bf16
    _variants(cs, "wgrad", dma(64, 64), [S9, S18, S90], cin=64, cout=64)                     # SL 4 tail, SL 4 main+tail, SL 16
    _variants(cs, "wgrad", dma(64, 136), [S90], cin=64, cout=136, note="ragged")             # 3 output groups: G = 80, SL 16
    _variants(cs, "wgrad", taprow, [S18, S90], cin=48, cout=16)
    _variants(cs, "wgrad", mfma(20, 12, 3), [S9, S18], cin=20, cout=12)
    _variants(cs, "wgrad", mfma(40, 40, 3), [S9, S18], cin=40, cout=40, nodb=False)
    _variants(cs, "wgrad", mfma(88, 64, 1), [S9, S18], cin=88, cout=64, k=1)
    _variants(cs, "wgrad", mfma(24, 40, 1), [S9, S18], cin=24, cout=40, k=1, nodb=False)
    # ---- conv_wgrad, fp32 (split-operand kernels; 8 x 16 tiles)
    _variants(cs, "wgrad", x3(64, 64, 3), [(1, 16, 40), (2, 40, 96), (3, 40, 96)], cin=64, cout=64, dtype="f32")      # G = 6, 60 (SL 4), 90 (SL 16)
    _variants(cs, "wgrad", x3(72, 40, 1), [(1, 16, 32), (1, 16, 40), (1, 80, 48)], cin=72, cout=40, k=1, dtype="f32")   # 3 G = 12, 18 (SL 4), 90 (SL 16)
    _variants(cs, "wgrad", lambda n, h, w: (("wgrad_x3_thin_reduce/16", G_x3_thin(48, n, h, w), 16),), [S18, (3, 40, 96)], cin=48, cout=16, dtype="f32")
    # ---- the one-call backwards
    _variants(cs, "bwd_pair", lambda n, h, w: (("taprow_wgrad_reduce/16", G_pair(64, n, h, w), 16),), [S18, S90], cin=64, cout=32)
    _variants(cs, "bwd_wide", dma(64, 64), [S18, S90], cin=64, cout=64)
    # ---- image layers
    img_in = lambda k: (lambda n, h, w: ((f"image_in_wgrad_reduce<{k}>/16", G_image(n, h, w), 16),))
    img_out = lambda k: (lambda n, h, w: ((f"image_out_wgrad_reduce<{k}>/16", G_image(n, h, w), 16),))
    for k in (3, 1):
        _variants(cs, "image_in_wgrad", img_in(k), [S18, S90], k=k)
        _variants(cs, "image_out_wgrad", img_out(k), [S18, S90], k=k)
    _variants(cs, "image_out_bwd", lambda n, h, w: (("image_out_wgrad_reduce<3>/16", G_image_bwd(n, h, w), 16),), [S18, S90], k=3)
    # ---- the DenseBlock encoder
    _variants(cs, "dense_encoder_wgrad", lambda n, h, w: (("enc_wgrad_reduce/16", min(tiles(n, h, w, 16, 16), 512), 16),), [S18, S90])
    _variants(cs, "dense_encoder_wgrad", lambda n, h, w: (("image_in_wgrad_reduce<3>/16", G_image(n, h, w), 16),
                                                           ("wgrad_x3_dense_reduce/16", G_x3_dense(n, h, w), 16)), [S18, (3, 40, 96)], dtype="f32")
    enc1 = lambda n, h, w: (("enc_wgrad_reduce/16", G_enc_bwd(n, h, w, 1), 16),)
    enc2 = lambda kind: (lambda n, h, w: ((f"enc_wgrad_reduce pair {kind}/16", G_enc_bwd(n, h, w, 2), 16),))
    ENC = [(3, 80, 96), (8, 144, 40)]       # one block per CU walks slices of the (image, strip) columns: G = 30 and 72, for one branch and for two
    _variants(cs, "dense_encoder_bwd", enc1, ENC, note="one")
    _variants(cs, "dense_encoder_bwd", enc2("distinct"), ENC, note="two-distinct")
    _variants(cs, "dense_encoder_bwd", enc2("shared"), ENC, note="two-shared")
    # ---- a deferred sequence: wide (SL 4 job) + wide (SL 16 job) + pair + image-out backward queued, then one launch
    for acc in (0, 1):
        cs.append(BitsCase("deferred", (("reduce_multi_kernel wgrad_dma_reduce/4", G_dma(64, 64, *S18), 4), ("reduce_multi_kernel wgrad_dma_reduce/16", G_dma(64, 64, *S90), 16),
                                        ("reduce_multi_kernel taprow_wgrad_reduce/16", G_pair(64, *S90), 16),
                                        ("reduce_multi_kernel image_out_wgrad_reduce<3>/16", G_image_bwd(*S90), 16)), *S90, accumulate=acc))
    return cs


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"
# flavours whose slice count follows G cannot sum G <= 48 partials in 16 slices
UNREACHABLE = {("wgrad_dma_reduce/16", "tail"), ("wgrad_x3_reduce<taps 9>/16", "tail"), ("wgrad_x3_reduce<taps 1>/16", "tail"),
               ("reduce_multi_kernel wgrad_dma_reduce/16", "tail")}


# ------------------------------------------------------------------------------------------------------------------------------
# running a case (GPU)
# ------------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def _rng(c, salt=0):
    return np.random.default_rng(zlib.crc32(repr((c.op, c.dtype, c.cin, c.cout, c.k, c.n, c.h, c.w, c.note, salt)).encode()))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def sha(arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(_f32(a).tobytes())
    return m.hexdigest()


class _Inputs:
    """every operand of a case as float32 numpy arrays, in a fixed order (their SHA-256 is recorded next to the outputs')"""

    def __init__(self):
        self.arrays = []

    def add(self, a):
        a = _f32(a)
        self.arrays.append(a)
        return a


def _conv_operands(c, inp, cin=None, cout=None, shape=None):
    n, h, w = shape or (c.n, c.h, c.w)
    cc = CC.Case("bits", "wgrad", cin or c.cin, cout or c.cout, n, h, w, k=c.k, dtype=c.dtype, impl="x3" if c.dtype == "f32" else "mfma")
    o = CC.operands(cc)
    return cc, (inp.add(o.x), inp.add(o.g), inp.add(o.w32), inp.add(o.dw_old), inp.add(o.db_old))


def _dev(a):
    import torch
    return torch.from_numpy(_f32(a)).to(DEV)


def _conv_call(c, op, cc, arrs, acc, want_db=True):
    """one conv_wgrad / conv_bwd_pair / conv_bwd_wide call on fresh destinations; returns {name: tensor}"""
    import torch
    from mmif import _lib as L
    from mmif import tensor as T
    x, g, w32, dw_old, db_old = arrs
    td = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    bx = T.BT.from_nchw(_dev(x), td)
    bg = T.BT.from_nchw(_dev(g), td, halo=1).as_folded()
    dw, db = _dev(dw_old), (_dev(db_old) if want_db else None)
    ws = torch.empty(T.wgrad_workspace_bytes(cc.cin, cc.cout, cc.k) // 4 + 1, dtype=torch.float32, device=DEV)
    if op == "wgrad":
        T.conv_wgrad(bx, bg, dw, db, cc.cin, cc.cout, cc.k, ws, bool(acc), L.IMPL_X3 if c.dtype == "f32" else L.IMPL_MFMA)
    else:
        pk = T.PackedWeights(cc.cout, cc.cin, cc.k, DEV, L.BF16)
        pk.pack(_dev(w32))
        gx = T.BT.alloc(cc.n, cc.cin, cc.h, cc.w, td, DEV, halo=1, zero=True)
        if op == "bwd_pair":
            T.conv_bwd_pair(bg, bx, gx, dw, db, cc.cin, cc.cout, cc.k, pk, ws, bool(acc))
        else:
            signs = torch.zeros(T.bwd_wide_signs_bytes(cc.n, cc.cin, cc.h, cc.w) + 64, dtype=torch.uint8, device=DEV)
            T.conv_bwd_wide(bg, bx, gx, dw, db, cc.cin, cc.cout, cc.k, pk, (1 << cdiv(cc.cin, 8)) - 1, ws, signs, int(acc))
    return {"dw": dw, **({"db": db} if want_db else {})}


def _image_out_operands(c, inp, shape=None):
    n, h, w = shape or (c.n, c.h, c.w)
    r = _rng(c, ("image_out", n, h, w))
    x = inp.add(CC.rnd(np.maximum(r.standard_normal((n, 16, h, w)), 0.0), "bf16"))
    wt = inp.add(r.standard_normal((1, 16, c.k, c.k)) * 0.2)
    gimg = inp.add(r.standard_normal((n, 1, h, w)))
    yimg = inp.add(np.maximum(r.standard_normal((n, 1, h, w)), 0.0))          # the layer's (ReLU) output: masks gimg where it is 0
    dw_old, db_old = inp.add(r.standard_normal((1, 16, c.k, c.k)) * 30), inp.add(r.standard_normal(1) * 30)
    return x, wt, gimg, yimg, dw_old, db_old


def _image_out_call(c, op, arrs, acc, want_db=True):
    import torch
    from mmif import tensor as T
    x, wt, gimg, yimg, dw_old, db_old = arrs
    n, _, h, w = x.shape
    bx = T.BT.from_nchw(_dev(x), torch.bfloat16)
    dw, db = _dev(dw_old), (_dev(db_old) if want_db else None)
    ws = torch.empty(T.image_wgrad_workspace_bytes(16, c.k) // 4 + 1, dtype=torch.float32, device=DEV)
    if op == "image_out_wgrad":
        T.image_out_wgrad(bx, _dev(gimg), _dev(yimg), dw, db, 16, c.k, ws, bool(acc))
    else:
        gx = T.BT.alloc(n, 16, h, w, torch.bfloat16, DEV, halo=1, zero=True)
        assert T.image_out_bwd_supported(bx, 16, c.k)
        T.image_out_bwd(bx, _dev(gimg), _dev(yimg), _dev(wt), gx, dw, db, 16, c.k, ws, bool(acc))
    return {"dw": dw, **({"db": db} if want_db else {})}


ENC_SHAPES = [((16, 1, 3, 3), (16,)), ((16, 16, 3, 3), (16,)), ((16, 32, 3, 3), (16,)), ((16, 48, 3, 3), (16,))]


def _enc_operands(c, inp, branch):
    r = _rng(c, ("enc", branch))
    shape = (c.n, 64, c.h, c.w)
    x = r.standard_normal(shape)
    x[np.abs(x) < 0.5] = 0.0                                    # ReLU-style activations: zeros mask the gradient chain
    x = inp.add(CC.rnd(np.abs(x) * (r.random(shape) > 0.3), c.dtype))
    g = inp.add(CC.rnd(r.standard_normal(shape), c.dtype))
    ws = [inp.add(r.standard_normal((16, 16 * (i + 1), 3, 3)) * (0.25 / (i + 1))) for i in range(3)]
    img = inp.add(r.random((c.n, 1, c.h, c.w)))
    old = [(inp.add(r.standard_normal(a) * 30), inp.add(r.standard_normal(b) * 30)) for a, b in ENC_SHAPES]
    return x, g, ws, img, old


def _enc_grads(old, want_db):
    return [(_dev(a), _dev(b) if want_db else None) for a, b in old]


def _named(grads, suffix=""):
    out = {}
    for L, (dw, db) in enumerate(grads):
        out[f"dw{L}{suffix}"] = dw
        if db is not None:
            out[f"db{L}{suffix}"] = db
    return out


def run(c: BitsCase):
    """run the case on the current device; returns (outputs {name: float32 tensor}, SHA-256 of the input operands)"""
    import torch
    from mmif import tensor as T
    from mmif._lib import lib
    inp = _Inputs()
    acc = c.accumulate
    if c.op in ("wgrad", "bwd_pair", "bwd_wide"):
        cc, arrs = _conv_operands(c, inp)
        out = _conv_call(c, c.op, cc, arrs, acc, c.db)
    elif c.op == "image_in_wgrad":
        r = _rng(c)
        td = torch.bfloat16
        img = inp.add(r.random((c.n, 1, c.h, c.w)))
        g = inp.add(CC.rnd(r.standard_normal((c.n, 16, c.h, c.w)), "bf16"))
        dw_old, db_old = inp.add(r.standard_normal((16, 1, c.k, c.k)) * 30), inp.add(r.standard_normal(16) * 30)
        dw, db = _dev(dw_old), (_dev(db_old) if c.db else None)
        ws = torch.empty(T.image_wgrad_workspace_bytes(16, c.k) // 4 + 1, dtype=torch.float32, device=DEV)
        T.image_in_wgrad(_dev(img), T.BT.from_nchw(_dev(g), td), dw, db, 16, c.k, ws, bool(acc))
        out = {"dw": dw, **({"db": db} if c.db else {})}
    elif c.op in ("image_out_wgrad", "image_out_bwd"):
        out = _image_out_call(c, c.op, _image_out_operands(c, inp), acc, c.db)
    elif c.op == "dense_encoder_wgrad":
        td = torch.bfloat16 if c.dtype == "bf16" else torch.float32
        x, g, _ws, img, old = _enc_operands(c, inp, 0)
        grads = _enc_grads(old, c.db)
        ws = torch.empty(T.dense_encoder_wgrad_workspace_bytes() // 4 + 1, dtype=torch.float32, device=DEV)
        F, GF = T.BT.from_nchw(_dev(x), td), T.BT.from_nchw(_dev(g), td, halo=1).as_folded()
        T.dense_encoder_wgrad(_dev(img), F.view(0, 6), GF.view(0, 8), grads, ws, bool(acc))
        out = _named(grads)
    elif c.op == "dense_encoder_bwd":
        ws = torch.empty(T.dense_encoder_bwd_workspace_bytes() // 4 + 1, dtype=torch.float32, device=DEV)
        branches, out = [], {}
        nb = 1 if c.note == "one" else 2
        for b in range(nb):
            x, g, wts, img, old = _enc_operands(c, inp, b)
            F, GF = T.BT.from_nchw(_dev(x), torch.bfloat16), T.BT.from_nchw(_dev(g), torch.bfloat16, halo=1).as_folded()
            pk = T.pack_dense_chain(*[_dev(t) for t in wts], DEV)
            shared = c.note == "two-shared" and b == 1
            grads = branches[0][5] if shared else _enc_grads(old, c.db)
            branches.append((GF.view(6, 2), GF.view(0, 6), F.view(0, 6), pk, _dev(img), grads, True if shared else bool(acc)))
            if not shared:
                out.update(_named(grads, "ab"[b] if nb == 2 else ""))
        T.dense_encoder_bwd(branches, ws)
    elif c.op == "deferred":
        calls = []                                             # (name, fn(acc) -> outputs, workspace bytes)
        for name, shape in (("wide4", S18), ("wide16", S90)):
            cc, arrs = _conv_operands(c, inp, 64, 64, shape)
            calls.append((name, (lambda cc=cc, arrs=arrs: _conv_call(c, "bwd_wide", cc, arrs, acc)), T.wgrad_workspace_bytes(64, 64, 3)))
        cc, arrs = _conv_operands(c, inp, 64, 32, S90)
        calls.append(("pair", (lambda cc=cc, arrs=arrs: _conv_call(c, "bwd_pair", cc, arrs, acc)), T.wgrad_workspace_bytes(64, 32, 3)))
        io = _image_out_operands(c, inp, S90)
        calls.append(("image", (lambda: _image_out_call(c, "image_out_bwd", io, acc)), T.image_wgrad_workspace_bytes(16, 3)))
        plain = {f"{name}.{k}": v for name, fn, _ in calls for k, v in fn().items()}
        torch.cuda.synchronize()
        arena = torch.empty(sum(b for _, _, b in calls) // 4 + 256 * len(calls), dtype=torch.float32, device=DEV)
        T.check(lib.mmif_reduce_defer_begin(arena.data_ptr(), arena.numel() * 4), "reduce_defer_begin")
        try:
            out = {f"{name}.{k}": v for name, fn, _ in calls for k, v in fn().items()}
            queued = lib.mmif_reduce_defer_pending()
        finally:
            T.check(lib.mmif_reduce_defer_flush(0, T.stream_ptr()), "reduce_defer_flush")
        torch.cuda.synchronize()
        assert queued == len(calls), f"{c.id}: {queued} of {len(calls)} reduces were queued"
        for k in out:
            assert torch.equal(out[k], plain[k]), f"{c.id}: {k} differs between the deferred launch and a reduce behind every producer"
    else:
        raise ValueError(c.op)
    torch.cuda.synchronize()
    return out, sha(inp.arrays)


def digest(t):
    """(SHA-256 of the float32 bytes of t + 0.0 -- the sign of an exact zero is not part of the contract --, fp64 sum)"""
    a = (t.detach().float() + 0.0).cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), float(a.astype(np.float64).sum())
