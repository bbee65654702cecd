"""Every entry point of the blocked-layout glue family (csrc/nest.hip: mmif_maxpool2x2_fwd / _bwd / _bwd_relu, mmif_upsample2x_fwd / _bwd /
_bwd_relu, mmif_relu_mask, mmif_fuse_attn_fwd / _bwd / _bwd_cached; csrc/misc.hip: mmif_fuse_elem_fwd / _bwd, mmif_nchw_to_blocked,
mmif_blocked_to_nchw, mmif_zero), both storage types, against its fp64 definition (tests/nest_cases.py), element-wise, with derived bounds.

Device buffers are built in torch straight from the stored arrays and read back whole: the two conversion kernels are under test like the
others, not the measuring instrument.  Operands are views at cb_off 1 (inputs) or 2 (outputs) of wider tensors between sentinel guard blocks
(both attention inputs as halves of one tensor, ga / gb as halves of one tensor: the engines' layout), or tensors of their own at cb_off 0.
Outputs are pre-filled with the sentinel: after the call the guards are untouched, every element the definition leaves alone (the halo of an
outgoing gradient that is written interior-only) still holds it, and no defined element does.  Inputs are bit-identical afterwards.

Bounds (nest_cases.py; u = 2^-24, ULP = 2^-8): selection and copy kernels bit-exact; everything else |got - want| <= K u A (+ ULP |want|, bf16
store), accumulate + u (|old| + A).  Also: a second call on the same operands is bit-identical; mmif_fuse_attn_bwd_cached after the forward is
bit-identical to mmif_fuse_attn_bwd on a garbage workspace; _bwd_relu is the plain call followed by the definition's mask, bit for bit.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import nest_cases as NC
from nest_cases import CASES, SENT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}           # kernel, storage type, output -> [max err / bound, max err, checks]
GUARD_FLOATS = 64     # sentinel floats on either side of a plain fp32 NCHW destination


def _td(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Buf:
    """blocked device buffer [n][cbt][hs][ws][8]: guards[0] sentinel blocks, the arrays (each [n, 8k, hs, ws], stored domain) in turn,
    guards[1] sentinel blocks; views[i] is the BT of arrs[i] with logical extent h x w"""

    def __init__(self, c, arrs, h, w, halo, guards, flags=0):
        from mmif import tensor as T
        n = arrs[0].shape[0]
        hs, ws = h + 2 * halo, w + 2 * halo
        assert all(a.shape == (n, a.shape[1], hs, ws) and a.shape[1] % 8 == 0 for a in arrs), [a.shape for a in arrs]
        self.cbs = [a.shape[1] // 8 for a in arrs]
        self.offs = [guards[0] + sum(self.cbs[:i]) for i in range(len(arrs))]
        self.cbt = guards[0] + sum(self.cbs) + guards[1]
        full = np.full((n, self.cbt * 8, hs, ws), SENT, np.float32)
        for a, off, cb in zip(arrs, self.offs, self.cbs):
            full[:, off * 8:(off + cb) * 8] = a
        self.buf = torch.from_numpy(np.ascontiguousarray(full.reshape(n, self.cbt, 8, hs, ws).transpose(0, 1, 3, 4, 2))).to(_td(c)).to(DEV)
        self.before = self.buf.clone()
        self.views = [T.BT(self.buf, n, h, w, halo, self.cbt, off, cb, T._CODE[_td(c)], flags) for off, cb in zip(self.offs, self.cbs)]

    def split(self):
        """([the views' contents], everything outside them), float64, [n, channels, hs, ws]"""
        b = self.buf.float().cpu().numpy()
        n, cbt, hs, ws, _ = b.shape
        a = b.transpose(0, 1, 4, 2, 3).reshape(n, cbt * 8, hs, ws)
        inside = np.zeros(a.shape[1], bool)
        out = []
        for off, cb in zip(self.offs, self.cbs):
            out.append(a[:, off * 8:(off + cb) * 8])
            inside[off * 8:(off + cb) * 8] = True
        return out, a[:, ~inside]

    def unchanged(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


def _group(c, arrs, h, w, halo, off, flags=0):
    """the case's layout for a group of same-shaped operands: views of one tensor behind `off` guard blocks (one more guard behind), or one
    tensor each at cb_off 0.  -> (views, buffers)"""
    if c.view:
        b = Buf(c, arrs, h, w, halo, (off, 1), flags)
        return b.views, [b]
    bs = [Buf(c, [a], h, w, halo, (0, 0), flags) for a in arrs]
    return [b.views[0] for b in bs], bs


def _ins(c, arrs, h, w, halo=0, flags=0):
    return _group(c, [np.asarray(a, np.float32) for a in arrs], h, w, halo, 1, flags)


def _grad_in(c, stored):
    from mmif import _lib as L
    gh, gw = c.ghw
    (g,), bufs = _ins(c, [stored], gh, gw, c.halo, L.T_FOLDED if c.g == "folded" else 0)
    return g, bufs


def _outs(c, init, h, w, halo, flags=0):
    return _group(c, [np.asarray(a, np.float32) for a in init], h, w, halo, 2, flags)


def _grad_out_init(c, old):
    """an outgoing halo-1 gradient before the call: the old value inside when the call accumulates, the sentinel everywhere else"""
    shape = (c.n, c.C, c.h, c.w)
    inner = old if c.acc else np.full(shape, SENT)
    return NC.embed(np.asarray(inner, np.float64))


class Run:
    """one launch of the case's entry point on fresh buffers"""

    def __init__(self, c, cached=None, mask=None):
        from mmif import tensor as T
        from mmif._lib import lib
        o = NC.operands(c)
        mask = c.mask if mask is None else mask
        self.ins, self.outs, self.flat = [], [], None
        k = c.k
        if k in ("pool_fwd", "up_fwd"):
            (x,), self.ins = _ins(c, [o["x"]], c.h, c.w)
            oh, ow = (c.h // 2, c.w // 2) if k == "pool_fwd" else c.target
            (y,), self.outs = _outs(c, [np.full((c.n, c.C, oh, ow), SENT)], oh, ow, 0)
            (T.maxpool_fwd if k == "pool_fwd" else T.upsample_fwd)(x, y)
        elif k == "pool_bwd":
            (x,), self.ins = _ins(c, [o["x"]], c.h, c.w)
            g, gb = _grad_in(c, o["g"])
            self.ins += gb
            (gx,), self.outs = _outs(c, [_grad_out_init(c, o["old"])], c.h, c.w, 1)
            T.maxpool_bwd(x, g, gx, c.acc, relu=bool(mask))
        elif k == "up_bwd":
            g, self.ins = _grad_in(c, o["g"])
            xm = None
            if mask:
                (xm,), xb = _ins(c, [o["xm"]], c.h, c.w)
                self.ins += xb
            (gx,), self.outs = _outs(c, [_grad_out_init(c, o["old"])], c.h, c.w, 1)
            T.upsample_bwd(g, gx, c.acc, relu_of=xm)
        elif k == "relu_mask":
            from mmif import _lib as L
            (x,), self.ins = _ins(c, [o["x"]], c.h, c.w)
            (g,), self.outs = _outs(c, [o["g"]], c.h, c.w, c.halo, L.T_FOLDED if c.g == "folded" else 0)
            T.relu_mask_(x, g)
        elif k in ("attn_fwd", "attn_bwd"):
            (a, b), self.ins = _ins(c, [o["a"], o["b"]], c.h, c.w)
            mode = T.ATTN_MODES[c.mode]
            ws = torch.full_like(T.attn_workspace(c.n, c.C, DEV), 1e30)          # garbage: nothing may be taken from it uncomputed
            if k == "attn_fwd":
                (out,), self.outs = _outs(c, [np.full(o["a"].shape, SENT)], c.h, c.w, 0)
                T.attn_fwd(a, b, out, mode, ws)
            else:
                g, gb_ = _grad_in(c, o["g"])
                self.ins += gb_
                (ga, gb), self.outs = _outs(c, [_grad_out_init(c, o["old_a"]), _grad_out_init(c, o["old_b"])], c.h, c.w, 1)
                cached = c.cached if cached is None else cached
                if cached:
                    (tmp,), _ = _outs(c, [np.full(o["a"].shape, SENT)], c.h, c.w, 0)
                    T.attn_fwd(a, b, tmp, mode, ws)
                T.attn_bwd(a, b, g, ga, gb, mode, c.acc, ws, cached=cached)
        elif k in ("elem_fwd", "elem_bwd"):
            mode = NC.ELEM_MODES.index(c.mode)
            if c.same:
                (a,), self.ins = _ins(c, [o["a"]], c.h, c.w)
                b = a
            else:
                (a, b), self.ins = _ins(c, [o["a"], o["b"]], c.h, c.w)
            if k == "elem_fwd":
                (out,), self.outs = _outs(c, [np.full(o["a"].shape, SENT)], c.h, c.w, 0)
                T.fuse_elem_fwd(a, b, out, mode)
            else:
                g, gb_ = _grad_in(c, o["g"])
                self.ins += gb_
                (ga, gb), self.outs = _outs(c, [np.full(o["g"].shape, SENT)] * 2, c.h, c.w, c.halo, g.flags)
                need = mask or c.mode == "max"
                T.fuse_elem_bwd(a if need else None, b if need else None, g, ga, gb, mode, mask)
        elif k == "to_blocked":
            src = torch.from_numpy(o["src"].astype(np.float32)).to(DEV)
            (dst,), self.outs = _outs(c, [np.full((c.n, c.C, c.h + 2 * c.halo, c.w + 2 * c.halo), SENT)], c.h, c.w, c.halo)
            T.check(lib.mmif_nchw_to_blocked(ctypes.c_void_p(src.data_ptr()), c.c, dst.d, T.stream_ptr()), "nchw_to_blocked")
            self.src = src
        elif k == "to_nchw":
            g, self.ins = _grad_in(c, o["g"])
            count = c.n * c.c * c.h * c.w
            self.flat = torch.full((count + 2 * GUARD_FLOATS,), SENT, dtype=torch.float32, device=DEV)
            T.check(lib.mmif_blocked_to_nchw(g.d, ctypes.c_void_p(self.flat.data_ptr() + 4 * GUARD_FLOATS), c.c, T.stream_ptr()), "blocked_to_nchw")
        elif k == "zero":
            (t,), self.outs = _outs(c, [np.full((c.n, c.C, c.h + 2 * c.halo, c.w + 2 * c.halo), 3.0)], c.h, c.w, c.halo)
            t.zero_()
        else:
            raise AssertionError(k)
        torch.cuda.synchronize()

    def results(self, c):
        """[got] per output of NC.define(c), and everything outside the outputs"""
        if self.flat is not None:
            f = self.flat.cpu().numpy().astype(np.float64)
            return [f[GUARD_FLOATS:-GUARD_FLOATS].reshape(c.n, c.c, c.h, c.w)], np.concatenate([f[:GUARD_FLOATS], f[-GUARD_FLOATS:]])
        got, outside = [], []
        for b in self.outs:
            g_, o_ = b.split()
            got += g_
            outside.append(o_.ravel())
        return got, np.concatenate(outside)

    def same_bits(self, other):
        if self.flat is not None:
            return torch.equal(self.flat.view(torch.int32), other.flat.view(torch.int32))
        return all(torch.equal(_bits(a.buf), _bits(b.buf)) for a, b in zip(self.outs, other.outs))


def _check(c, name, got, want, bound):
    assert got.shape == want.shape, (got.shape, want.shape)
    defined = want != SENT
    if c.k != "zero":
        assert float(np.abs(want[defined]).max()) > 0, f"{c.id} {name}: all-zero reference"
    left = (got == SENT) & defined
    assert not left.any(), f"{c.id} {name}: {int(left.sum())} defined elements still hold the sentinel, first at {tuple(np.argwhere(left)[0])}"
    spoilt = (got != SENT) & ~defined
    assert not spoilt.any(), f"{c.id} {name}: {int(spoilt.sum())} elements the call must leave alone were written, first at {tuple(np.argwhere(spoilt)[0])}"
    err, bound = np.abs(got - want), np.asarray(bound, np.float64)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    r = float(ratio.max())
    e = RATIOS.setdefault(f"{c.k} {c.dtype} {name}", [0.0, 0.0, 0])
    e[0], e[1], e[2] = max(e[0], min(r, 1e30)), max(e[1], float(err.max())), e[2] + 1
    print(f"{c.id} {name}: max err {err.max():.3e}, max err / bound {r:.3f}")
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"{c.id} {name}: {int(bad.sum())} of {bad.size} elements beyond the bound; worst at [n, ch, ys, xs] = "
                             f"{tuple(int(k) for k in i)}: got {got[i]!r}, want {want[i]!r}, err {err[i]:.3e}, "
                             f"bound {np.broadcast_to(bound, err.shape)[i]:.3e} (err / bound {r:.3g})")


def _sweep(c):
    run = Run(c)
    got, outside = run.results(c)
    assert bool((outside == SENT).all()), f"{c.id}: guard blocks next to the output were written"
    if c.view and run.flat is None:
        assert outside.size > 0
    assert all(b.unchanged() for b in run.ins), f"{c.id}: an input was written"
    outs = NC.define(c)
    assert len(outs) == len(got)
    for o, g_ in zip(outs, got):
        _check(c, o.name, g_, o.want, o.bound)
    return run, got


@pytest.mark.parametrize("c", [c for c in CASES if not c.stride], ids=lambda c: c.id)
def test_kernel_equals_definition(c):
    run, got = _sweep(c)
    # ---- determinism: the same call on fresh buffers; for the attention backward the other of cached / uncached
    again = Run(c, cached=(not c.cached) if c.k == "attn_bwd" else None)
    assert run.same_bits(again), f"{c.id}: a second call differs" + (" (cached against uncached)" if c.k == "attn_bwd" else "")
    # ---- the mask riding in the backward = the plain call, then the definition's mask
    if c.k in ("pool_bwd", "up_bwd") and c.mask:
        plain, _ = Run(c, mask=0).results(c)
        o = NC.operands(c)
        keep = NC.embed(NC.relu_keep(o["x"] if c.k == "pool_bwd" else o["xm"]).astype(np.float64))
        want = np.where(keep == SENT, plain[0], np.where(keep == 1, plain[0], 0.0))
        assert np.array_equal(got[0], want), f"{c.id}: _bwd_relu is not _bwd followed by the mask"


@pytest.mark.parametrize("c", [c for c in CASES if c.stride], ids=lambda c: c.id)
def test_second_trip_of_the_grid_stride_loop(c):
    """more items than grid_for()'s 8192 blocks x 256 threads (misc.hip: 4096): the whole result, once"""
    assert c.items > NC.GRID_CAP_ITEMS
    _sweep(c)


def test_zz_report_error_over_bound_per_family():
    """prints the measured maximum of every kernel, storage type and output as a fraction of its bound ($MMIF_NEST_SWEEP_REPORT: also as JSON)"""
    for k in sorted(RATIOS):
        r, e, n = RATIOS[k]
        print(f"{k:28s} max err/bound {r:8.4f}   max err {e:.3e}   checks {n}")
    path = os.environ.get("MMIF_NEST_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)
