"""Every entry point of csrc/conv_general.hip and csrc/resample.hip against its fp64 definition (tests/general_cases.py), element-wise, with
derived bounds.

Device buffers are built in torch straight from the stored arrays and the C ABI is called through mmif._lib.lib (mmif/tensor.py's wrappers
allocate exact-size outputs, which could not carry guards).  Every output sits inside a larger allocation pre-filled with a sentinel, 64 guard
elements on either side, at an odd element offset in the cases marked so; a workspace is exactly the queried number of bytes of 1e30 garbage
with a guard behind it.  After the call: every output element within its bound (selections bit-exact), no sentinel left, nothing non-finite
that the definition does not have, guards and the workspace's guard untouched, inputs bit-identical; a second call on fresh buffers is
bit-identical (the "no atomics" claim of conv_general.hip's header).  An output passed as NULL (bias, db) cannot be watched: that the call
returns and every other buffer's guards are intact is all the evidence there is.  Chained: gconv_fwd -> relu_bwd on the kernel's own y ->
dgrad / wgrad; the max-pool's own indices fed to its backward; gconvt_fwd against gconv_dgrad of the mirrored conv, bit for bit.  Each wrapper of
mmif/tensor.py for this family must return the bits of the direct call.
"""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import general_cases as GC
from general_cases import CASES, SENT, SENT_U8, Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
RATIOS = {}           # entry point, output -> [max err / bound, max err, checks]
TDT = {"f32": torch.float32, "u8": torch.uint8}


class Buf:
    """a device array of `size` elements inside a sentinel-filled allocation: GUARD (+ 1 when odd) elements in front, at least GUARD behind"""

    def __init__(self, values=None, size=None, dtype="f32", odd=False):
        if values is not None:
            values = np.asarray(values).reshape(-1)
            size = values.size
        self.size, self.off, self.sent = size, GUARD + (1 if odd else 0), SENT if dtype == "f32" else SENT_U8
        self.full = torch.full((size + 2 * GUARD + 2,), self.sent, dtype=TDT[dtype], device=DEV)
        if values is not None and size:
            self.full[self.off:self.off + size] = torch.from_numpy(values.astype(np.float32 if dtype == "f32" else np.uint8)).to(DEV)
        self.before = self.full.clone()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.full.data_ptr() + self.off * self.full.element_size())

    @property
    def view(self):
        return self.full[self.off:self.off + self.size]

    def got(self):
        return self.view.cpu().numpy().astype(np.float64)

    def bits(self):
        return self.full.view(torch.int32) if self.full.dtype == torch.float32 else self.full

    def guards_untouched(self):
        g = torch.cat([self.full[:self.off], self.full[self.off + self.size:]])
        return bool((g == self.sent).all())

    def unchanged(self):
        return torch.equal(self.bits(), self.before.view(self.bits().dtype))


def _ptr(b):
    return None if b is None else b.ptr


class Workspace:
    """exactly `nbytes` (a multiple of 4, possibly 0) of 1e30 garbage, GUARD floats of it behind"""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.full = torch.full((self.n + GUARD,), 1e30, dtype=torch.float32, device=DEV)
        self.ptr, self.nbytes = ctypes.c_void_p(self.full.data_ptr()), nbytes

    def guard_untouched(self):
        return bool((self.full[self.n:] == 1e30).all())


class Run:
    """the case's call on fresh buffers: outs[name] = Buf per output of GC.define, ins = every operand, each of which must come back bit-identical"""

    def __init__(self, c, o=None):
        from mmif._lib import check, lib
        from mmif.tensor import stream_ptr
        o = GC.operands(c) if o is None else o
        st = stream_ptr()
        self.outs, self.ins, self.ws = {}, {}, []

        def inp(name, dtype="f32"):
            if o.get(name) is None:
                return None
            self.ins[name] = Buf(o[name], dtype=dtype, odd=c.offset)
            return self.ins[name]

        def out(name, size, present=True, dtype="f32"):
            if not present:
                return None
            self.outs[name] = Buf(size=int(size), dtype=dtype, odd=c.offset)
            return self.outs[name]

        def ws(nbytes):
            self.ws.append(Workspace(nbytes))
            return self.ws[-1]

        ep, n, ci, co, h, w, k = c.ep, c.n, c.cin, c.cout, c.h, c.w, c.k
        if ep == "gconv_fwd":
            x, wt, b, y = inp("x"), inp("w"), inp("bias"), out("y", n * co * c.ho * c.wo)
            rc = lib.mmif_gconv_fwd(x.ptr, wt.ptr, _ptr(b), y.ptr, n, ci, co, h, w, k, c.s, c.p, int(c.reflect), int(c.relu), st)
        elif ep == "gconv_dgrad":
            gy, wt, dx = inp("gy"), inp("w"), out("dx", n * ci * h * w)
            s = ws(lib.mmif_gconv_dgrad_workspace(n, ci, h, w, c.p, int(c.reflect)))
            rc = lib.mmif_gconv_dgrad(gy.ptr, wt.ptr, dx.ptr, n, ci, co, h, w, k, c.s, c.p, int(c.reflect), s.ptr, s.nbytes, st)
        elif ep == "gconv_wgrad":
            x, gy, dw, db = inp("x"), inp("gy"), out("dw", co * ci * k * k), out("db", co, c.db)
            s = ws(lib.mmif_gconv_wgrad_workspace(ci, co, k))
            rc = lib.mmif_gconv_wgrad(x.ptr, gy.ptr, dw.ptr, _ptr(db), n, ci, co, h, w, k, c.s, c.p, int(c.reflect), s.ptr, s.nbytes, st)
        elif ep == "gconvt_fwd":
            x, wt, b, y = inp("x"), inp("w"), inp("bias"), out("y", n * co * c.Ho * c.Wo)
            rc = lib.mmif_gconvt_fwd(x.ptr, wt.ptr, _ptr(b), y.ptr, n, ci, co, h, w, k, c.s, c.p, c.op, int(c.relu), st)
        elif ep == "gconvt_dgrad":
            gy, wt, dx = inp("gy"), inp("w"), out("dx", n * ci * h * w)
            rc = lib.mmif_gconvt_dgrad(gy.ptr, wt.ptr, dx.ptr, n, ci, co, h, w, k, c.s, c.p, c.op, st)
        elif ep == "gconvt_wgrad":
            x, gy, dw, db = inp("x"), inp("gy"), out("dw", co * ci * k * k), out("db", ci, c.db)
            s = ws(lib.mmif_gconv_wgrad_workspace(co, ci, k))
            rc = lib.mmif_gconvt_wgrad(x.ptr, gy.ptr, dw.ptr, _ptr(db), n, ci, co, h, w, k, c.s, c.p, c.op, s.ptr, s.nbytes, st)
        elif ep == "relu_bwd":
            g, y, r = inp("g"), inp("y"), out("out", h)
            rc = lib.mmif_relu_bwd(g.ptr, y.ptr, r.ptr, h, st)
        elif ep == "channel_sum":
            x, r = inp("x"), out("out", ci)
            rc = lib.mmif_channel_sum(x.ptr, r.ptr, n, ci, h, st)
        elif ep == "dwconv_fwd":
            x, wt, b, y = inp("x"), inp("w"), inp("bias"), out("y", n * ci * h * w)
            rc = lib.mmif_dwconv_fwd(x.ptr, wt.ptr, _ptr(b), y.ptr, n, ci, h, w, k, int(c.reflect), st)
        elif ep == "dwconv_dgrad":
            gy, wt, dx = inp("gy"), inp("w"), out("dx", n * ci * h * w)
            rc = lib.mmif_dwconv_dgrad(gy.ptr, wt.ptr, dx.ptr, n, ci, h, w, k, int(c.reflect), st)
        elif ep == "dwconv_wgrad":
            x, gy, dw, db = inp("x"), inp("gy"), out("dw", ci * k * k), out("db", ci, c.db)
            rc = lib.mmif_dwconv_wgrad(x.ptr, gy.ptr, dw.ptr, _ptr(db), n, ci, h, w, k, int(c.reflect), st)
        elif ep == "patchconv_fwd":
            x, wt, b, y = inp("x"), inp("w"), inp("bias"), out("y", n * ci * (h // k) * (w // k))
            rc = lib.mmif_patchconv_fwd(x.ptr, wt.ptr, _ptr(b), y.ptr, n, ci, h, w, k, st)
        elif ep == "patchconv_dgrad":
            gy, wt, dx = inp("gy"), inp("w"), out("dx", n * ci * h * w)
            rc = lib.mmif_patchconv_dgrad(gy.ptr, wt.ptr, dx.ptr, n, ci, h, w, k, st)
        elif ep == "patchconv_wgrad":
            x, gy, dw, db = inp("x"), inp("gy"), out("dw", ci * k * k), out("db", ci, c.db)
            s = ws(lib.mmif_patchconv_wgrad_workspace(ci, k))
            rc = lib.mmif_patchconv_wgrad(x.ptr, gy.ptr, dw.ptr, _ptr(db), n, ci, h, w, k, s.ptr, s.nbytes, st)
        elif ep == "bilinear_up_fwd":
            x, r = inp("x"), out("out", n * c.H * c.W)
            rc = lib.mmif_bilinear_up_fwd(x.ptr, r.ptr, n, h, w, c.H, c.W, st)
        elif ep == "bilinear_up_bwd":
            g, dx = inp("g"), out("dx", n * h * w)
            rc = lib.mmif_bilinear_up_bwd(g.ptr, dx.ptr, n, h, w, c.H, c.W, st)
        elif ep == "maxpool_nchw_fwd":
            x, y, idx = inp("x"), out("y", n * (h // k) * (w // k)), out("idx", n * (h // k) * (w // k), dtype="u8")
            rc = lib.mmif_maxpool_nchw_fwd(x.ptr, y.ptr, idx.ptr, n, h, w, k, st)
        elif ep == "maxpool_nchw_bwd":
            g, idx, dx = inp("g"), inp("idx", "u8"), out("dx", n * h * w)
            rc = lib.mmif_maxpool_nchw_bwd(g.ptr, idx.ptr, dx.ptr, n, h, w, k, st)
        elif ep == "nearest_up_fwd":
            x, y = inp("x"), out("y", n * h * k * w * k)
            rc = lib.mmif_nearest_up_fwd(x.ptr, y.ptr, n, h, w, k, st)
        elif ep == "nearest_up_bwd":
            g, dx = inp("g"), out("dx", n * h * w)
            rc = lib.mmif_nearest_up_bwd(g.ptr, dx.ptr, n, h, w, k, st)
        elif ep == "reflect_pad_fwd":
            l, r, t, b = c.pads
            x, y = inp("x"), out("y", n * (h + t + b) * (w + l + r))
            rc = lib.mmif_reflect_pad_fwd(x.ptr, y.ptr, n, h, w, l, r, t, b, st)
        elif ep == "reflect_pad_bwd":
            l, r, t, b = c.pads
            g, dx = inp("g"), out("dx", n * h * w)
            rc = lib.mmif_reflect_pad_bwd(g.ptr, dx.ptr, n, h, w, l, r, t, b, st)
        else:
            raise KeyError(ep)
        check(rc, c.id)
        torch.cuda.synchronize()

    def same_bits(self, other):
        return all(torch.equal(b.bits(), other.outs[k].bits()) for k, b in self.outs.items())


def _check(c, o, buf):
    got = buf.got()
    assert got.size == o.want.size, (c.id, o.name, got.size, o.want.shape)
    if not got.size:
        return
    if o.dtype == "f32":          # (a uint8 index is compared as a number: 255 is no index of a window of at most 15 x 15)
        left = got == SENT
        assert not left.any(), f"{c.id} {o.name}: {int(left.sum())} elements still hold the sentinel, first at {int(np.argmax(left))}"
    bad, err, ratio = GC.compare(o, got)
    r = float(ratio.max())
    e = RATIOS.setdefault(f"{c.ep} {o.name}", [0.0, 0.0, 0])
    e[0], e[1], e[2] = max(e[0], min(r, 1e30)), max(e[1], float(np.where(np.isfinite(err), err, 0.0).max())), e[2] + 1
    print(f"{c.id} {o.name}: max err {err.max():.3e}, max err / bound {r:.3f}")
    if bad.any():
        i = int(np.argmax(np.where(bad, np.maximum(ratio, 1e-300), 0.0)))
        idx = tuple(int(k) for k in np.unravel_index(i, o.want.shape))
        raise AssertionError(f"{c.id} {o.name}: {int(bad.sum())} of {bad.size} elements beyond the bound; worst at {idx}: got {got[i]!r}, want "
                             f"{o.want.reshape(-1)[i]!r}, err {err[i]:.3e}, bound {np.broadcast_to(o.bound, o.want.shape).reshape(-1)[i]:.3e} (err / bound {r:.3g})")


def _sweep(c, o=None):
    run = Run(c, o)
    outs = GC.define(c, o=o)
    assert {d.name for d in outs} == set(run.outs), (sorted(d.name for d in outs), sorted(run.outs))
    for name, b in run.outs.items():
        assert b.guards_untouched(), f"{c.id}: the guards around {name} were written"
    assert all(w.guard_untouched() for w in run.ws), f"{c.id}: the workspace was overrun"
    for name, b in run.ins.items():
        assert b.unchanged(), f"{c.id}: the input {name} was written"
    for d in outs:
        _check(c, d, run.outs[d.name])
    return run


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_kernel_equals_definition(c):
    run = _sweep(c)
    assert run.same_bits(Run(c)), f"{c.id}: a second call on fresh buffers differs"
    if c.plant == "ones":          # the transpose of an interpolation keeps the mass: sum dx = H W per plane
        d = GC.define(c)[0]
        dx = run.outs["dx"].got().reshape(c.n, -1)
        assert np.all(np.abs(dx.sum(1) - c.H * c.W) <= np.broadcast_to(d.bound, d.want.shape).reshape(c.n, -1).sum(1)), (c.id, dx.sum(1), c.H * c.W)


# ------------------------------------------------------------------------------------------------------------------------------ chained
CHAIN_FWD = [c for c in CASES if c.ep == "gconv_fwd" and c.relu][:12:2]


@pytest.mark.parametrize("c", CHAIN_FWD, ids=lambda c: c.id)
def test_conv_backward_on_the_forward_kernels_own_output(c):
    """gconv_fwd (ReLU) -> relu_bwd on the kernel's own y -> dgrad and wgrad, against the backward definitions evaluated at that stored y"""
    o = GC.operands(c)
    y = Run(c).outs["y"].got()
    gy = GC.f32(np.random.default_rng(c.h * 31 + c.w).standard_normal(y.size))
    rb = Case("relu_bwd", h=y.size, offset=c.offset)
    ob = dict(g=gy, y=y)
    masked = _sweep(rb, ob).outs["out"].got().reshape(c.n, c.cout, c.ho, c.wo)
    assert np.array_equal(masked, np.where(y > 0, gy, 0.0).reshape(masked.shape))
    _sweep(dataclasses.replace(c, ep="gconv_dgrad"), dict(gy=masked, w=o["w"]))
    _sweep(dataclasses.replace(c, ep="gconv_wgrad"), dict(gy=masked, x=o["x"]))


@pytest.mark.parametrize("c", [c for c in CASES if c.ep == "maxpool_nchw_fwd"][::2], ids=lambda c: c.id)
def test_maxpool_backward_on_the_forward_kernels_own_indices(c):
    f = Run(c)
    idx = f.outs["idx"].got().astype(np.uint8).reshape(c.n, c.h // c.k, c.w // c.k)
    g = GC.f32(np.random.default_rng(c.h).standard_normal(idx.shape))
    _sweep(dataclasses.replace(c, ep="maxpool_nchw_bwd"), dict(g=g, idx=idx))


@pytest.mark.parametrize("c", [c for c in CASES if c.ep == "gconvt_fwd"][::2], ids=lambda c: c.id)
def test_transposed_forward_is_the_input_gradient_of_the_mirrored_conv(c):
    """ConvTranspose2d(x; W[ci][co]) = gconv_dgrad(gy := x, W as [o = ci][c = co]) of the conv Ho x Wo -> h x w with zero padding (the identity
    conv_general.hip's header states), bit for bit where there is neither bias nor ReLU"""
    c = dataclasses.replace(c, bias=False, relu=False)
    o = {k: v for k, v in GC.operands(c).items() if k != "bias"}
    t = Run(c, o)
    m = Case("gconv_dgrad", n=c.n, cin=c.cout, cout=c.cin, h=c.Ho, w=c.Wo, k=c.k, s=c.s, p=c.p, reflect=False, offset=c.offset)
    assert (m.ho, m.wo) == (c.h, c.w)
    d = Run(m, dict(gy=o["x"], w=o["w"]))
    assert t.outs["y"].guards_untouched() and d.outs["dx"].guards_untouched()
    assert torch.equal(t.outs["y"].bits(), d.outs["dx"].bits())


# ------------------------------------------------------------------------------------------------------------------------------ wrappers
def _first(ep, pred=lambda c: True):
    return next(c for c in CASES if c.ep == ep and pred(c))


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _wrapper_calls():
    """entry point -> (case, what the wrapper of mmif/tensor.py is called with, the outputs in the wrapper's order)"""
    import mmif.tensor as T
    W = {}
    W["gconv_fwd"] = (T.gconv_fwd, lambda c, t: (t["x"], t["w"], t.get("bias"), c.s, c.p, c.reflect, c.relu), ("y",))
    W["gconv_dgrad"] = (T.gconv_dgrad, lambda c, t: (t["gy"], t["w"], (c.n, c.cin, c.h, c.w), c.s, c.p, c.reflect), ("dx",))
    W["gconv_wgrad"] = (T.gconv_wgrad, lambda c, t: (t["x"], t["gy"], c.k, c.s, c.p, c.reflect, c.db), ("dw", "db"))
    W["gconvt_fwd"] = (T.gconvt_fwd, lambda c, t: (t["x"], t["w"], t.get("bias"), c.s, c.p, c.op, c.relu), ("y",))
    W["gconvt_dgrad"] = (T.gconvt_dgrad, lambda c, t: (t["gy"], t["w"], (c.n, c.cin, c.h, c.w), c.s, c.p, c.op), ("dx",))
    W["gconvt_wgrad"] = (T.gconvt_wgrad, lambda c, t: (t["x"], t["gy"], c.k, c.s, c.p, c.op), ("dw",))
    W["relu_bwd"] = (T.relu_bwd, lambda c, t: (t["g"], t["y"]), ("out",))
    W["channel_sum"] = (T.channel_sum, lambda c, t: (t["x"],), ("out",))
    W["dwconv_fwd"] = (T.dwconv_fwd, lambda c, t: (t["x"], t["w"], t.get("bias"), c.reflect), ("y",))
    W["dwconv_dgrad"] = (T.dwconv_dgrad, lambda c, t: (t["gy"], t["w"], c.reflect), ("dx",))
    W["dwconv_wgrad"] = (T.dwconv_wgrad, lambda c, t: (t["x"], t["gy"], c.k, c.reflect, c.db), ("dw", "db"))
    W["patchconv_fwd"] = (T.patchconv_fwd, lambda c, t: (t["x"], t["w"], t.get("bias")), ("y",))
    W["patchconv_dgrad"] = (T.patchconv_dgrad, lambda c, t: (t["gy"], t["w"], (c.h, c.w)), ("dx",))
    W["patchconv_wgrad"] = (T.patchconv_wgrad, lambda c, t: (t["x"], t["gy"], c.k, c.db), ("dw", "db"))
    W["bilinear_up_fwd"] = (T.bilinear_up_fwd, lambda c, t: (t["x"][None], c.H // c.h), ("out",))
    W["bilinear_up_bwd"] = (T.bilinear_up_bwd, lambda c, t: (t["g"][None], (c.h, c.w)), ("dx",))
    W["maxpool_nchw_fwd"] = (T.maxpool_nchw_fwd, lambda c, t: (t["x"][None], c.k), ("y", "idx"))
    W["maxpool_nchw_bwd"] = (T.maxpool_nchw_bwd, lambda c, t: (t["g"][None], t["idx"][None], (c.h, c.w), c.k), ("dx",))
    W["nearest_up_fwd"] = (T.nearest_up_fwd, lambda c, t: (t["x"][None], c.k), ("y",))
    W["nearest_up_bwd"] = (T.nearest_up_bwd, lambda c, t: (t["g"][None], c.k), ("dx",))
    W["reflect_pad_fwd"] = (T.reflect_pad_fwd, lambda c, t: (t["x"][None], c.pads), ("y",))
    W["reflect_pad_bwd"] = (T.reflect_pad_bwd, lambda c, t: (t["g"][None], (c.h, c.w), c.pads), ("dx",))
    return W


WRAPPER_CASE = {   # a case whose operands the wrapper can express
    "gconvt_wgrad": lambda c: not c.db,          # (the wrapper passes no scratch for the alias's "db")
    "gconv_dgrad": lambda c: c.reflect and c.p > 0, "maxpool_nchw_fwd": lambda c: c.k == 3 and c.h % 3, "patchconv_wgrad": lambda c: c.db and c.h % c.k,
}
WRAPPED = ("gconv_fwd", "gconv_dgrad", "gconv_wgrad", "gconvt_fwd", "gconvt_dgrad", "gconvt_wgrad", "relu_bwd", "channel_sum", "dwconv_fwd", "dwconv_dgrad",
           "dwconv_wgrad", "patchconv_fwd", "patchconv_dgrad", "patchconv_wgrad", "bilinear_up_fwd", "bilinear_up_bwd", "maxpool_nchw_fwd", "maxpool_nchw_bwd",
           "nearest_up_fwd", "nearest_up_bwd", "reflect_pad_fwd", "reflect_pad_bwd")


def test_the_wrapper_list_is_the_family():
    assert set(WRAPPED) == set(GC.EPS)


@pytest.mark.parametrize("ep", WRAPPED)
def test_wrapper_returns_the_bits_of_the_direct_call(ep):
    """the only place the wrappers' own workspace sizing and shape arithmetic are checked"""
    fn, args, names = _wrapper_calls()[ep]
    if ep in ("bilinear_up_fwd", "bilinear_up_bwd"):          # no case of the table has one scale on both axes: one is made here
        c = Case(ep, n=6, h=5, w=3, H=15, W=9)
    else:
        c = _first(ep, WRAPPER_CASE.get(ep, lambda c: c.h * c.w > 1))
    o = GC.operands(c)
    if ep == "channel_sum":
        o = dict(x=o["x"].reshape(c.n, c.cin, c.h, 1))
    t = {k: _dev(v, torch.uint8 if k == "idx" else torch.float32) for k, v in o.items()}
    res = fn(*args(c, t))
    res = res if isinstance(res, tuple) else (res,)
    torch.cuda.synchronize()
    direct = Run(c)
    for name, r in zip(names, res):
        if name not in direct.outs:
            assert r is None, (ep, name)
            continue
        d = direct.outs[name].view
        assert r.numel() == d.numel(), (ep, name, tuple(r.shape), d.numel())
        same = torch.equal(r.reshape(-1).view(torch.int32), d.view(torch.int32)) if r.dtype == torch.float32 else torch.equal(r.reshape(-1), d)
        assert same, f"{c.id} {name}: the wrapper's result differs from the direct call"
        want = GC.define(c)[[x.name for x in GC.define(c)].index(name)].want
        assert tuple(r.shape)[-want.ndim:] == want.shape, (ep, name, tuple(r.shape), want.shape)


def test_zz_report_error_over_bound_per_entry_point():
    """prints the measured maximum of every entry point and output as a fraction of its bound ($MMIF_GENERAL_SWEEP_REPORT: also as JSON)"""
    for k in sorted(RATIOS):
        r, e, n = RATIOS[k]
        print(f"{k:28s} max err/bound {r:8.4f}   max err {e:.3e}   checks {n}")
    path = os.environ.get("MMIF_GENERAL_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)
