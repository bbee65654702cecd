"""Every entry point of the pair-conv family (csrc/pair.hip: mmif_pairconv_fwd / _dgrad / _wgrad / _bwd, both storage types, the bf16 forward
under $MMIF_PAIR_STRIP 1 and 0) against its fp64 definition (tests/pair_cases.py), element-wise, with derived bounds.

Outputs are views of buffers pre-filled with a sentinel, with one guard channel block on either side: the guards must stay untouched, and no
sentinel may survive inside the views (gx: the whole stored domain [h+2][w+2] is written).  Operands are views at a non-zero cb_off of one
tensor (the engine's layout) or tensors of their own.  An all-zero reference fails the case.

Bounds (pair_cases.py; u = 2^-24, ULP = 2^-8):
  forward, gx   |got - want| <= T u S (+ ULP |want|, bf16 store): S = the definition on absolute values, T = its number of terms; an element the
                ReLU mask zeroes has bound 0
  dw, db        |got - want| <= D u sum|g x|, D = Case.wgrad_depth (the longest chain of dependent fp32 additions, read from the kernels);
                accumulate: + u (|old| + sum|g x|) for the final addition
Also: dw / db bit-identical on two consecutive calls; accumulate = 1 gives old + fresh within one fp32 rounding; mmif_pairconv_bwd refuses an
unfolded `add`.  The kernel-against-kernel tests (tests/test_gpu_pairconv_bwd.py) keep asserting bit identity between the kernels.
"""
import json
import os

import numpy as np
import pytest
import torch

import pair_cases as PC
from pair_cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -1024.0        # bf16-exact, far from every reference value
RATIOS = {}           # entry point, storage type, output -> [max err / bound, max err, checks]


def _td(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


class Buf:
    """blocked device buffer [n][cbt][hs][ws][8]: guards[0] sentinel blocks, the arrays (each [n, 8k, hs, ws]) in turn, guards[1] sentinel blocks"""

    def __init__(self, c, arrs, halo, guards, flags=0):
        from mmif import tensor as T
        self.c, self.halo, self.flags = c, halo, flags
        n = arrs[0].shape[0]
        hs, ws = c.h + 2 * halo, c.w + 2 * halo
        assert all(a.shape == (n, a.shape[1], hs, ws) and a.shape[1] % 8 == 0 for a in arrs)
        self.cbs = [a.shape[1] // 8 for a in arrs]
        self.offs = [guards[0] + sum(self.cbs[:i]) for i in range(len(arrs))]
        self.cbt = guards[0] + sum(self.cbs) + guards[1]
        full = np.full((n, self.cbt * 8, hs, ws), SENT, np.float32)
        for a, off, cb in zip(arrs, self.offs, self.cbs):
            full[:, off * 8:(off + cb) * 8] = a
        self.buf = torch.from_numpy(np.ascontiguousarray(full.reshape(n, self.cbt, 8, hs, ws).transpose(0, 1, 3, 4, 2))).to(_td(c)).to(DEV)
        self.before = self.buf.clone()
        self.views = [T.BT(self.buf, n, c.h, c.w, halo, self.cbt, off, cb, T._CODE[_td(c)], flags) for off, cb in zip(self.offs, self.cbs)]

    def numpy(self):
        b = self.buf.float().cpu().numpy()
        n, cbt, hs, ws, _ = b.shape
        return b.transpose(0, 1, 4, 2, 3).reshape(n, cbt * 8, hs, ws).astype(np.float64)

    def split(self):
        """([the views' contents], everything outside them)"""
        a = self.numpy()
        inside = np.zeros(a.shape[1], bool)
        out = []
        for off, cb in zip(self.offs, self.cbs):
            out.append(a[:, off * 8:(off + cb) * 8])
            inside[off * 8:(off + cb) * 8] = True
        return out, a[:, ~inside]

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32),
                           self.before.view(torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32))


def _inputs(c, arrs, halo=0, flags=0):
    """the case's layout for a group of same-shaped inputs: views of one tensor behind a guard block, or one tensor each at cb_off 0"""
    if c.pair:
        b = Buf(c, arrs, halo, (1, 1), flags)
        return b.views, [b]
    bs = [Buf(c, [a], halo, (0, 0), flags) for a in arrs]
    return [b.views[0] for b in bs], bs


def _grad_inputs(c, stored, kind):
    from mmif import _lib as L
    return _inputs(c, stored, 0 if kind == "h0" else 1, L.T_FOLDED if kind == "folded" else 0)


def _outputs(c, count, halo):
    shape = (c.n, c.C, c.h + 2 * halo, c.w + 2 * halo)
    return Buf(c, [np.full(shape, SENT)] * count, halo, (1, 1))


def _family(c, what):
    s = f"{c.op} {c.dtype}"
    if c.op == "fwd" and c.dtype == "bf16":
        s += f" strip={c.strip}"
    return f"{s} {what}"


def _check(c, what, got, want, bound, blocked=True):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float(np.abs(want).max()) > 0, f"{c.id} {what}: all-zero reference"
    if blocked:
        left = (got == SENT) & (want != SENT)
        assert not left.any(), f"{c.id} {what}: {int(left.sum())} elements never written, first at {tuple(np.argwhere(left)[0])}"
    err = np.abs(got - want)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    r = float(ratio.max())
    e = RATIOS.setdefault(_family(c, what.split()[0]), [0.0, 0.0, 0])
    e[0], e[1], e[2] = max(e[0], r), max(e[1], float(err.max())), e[2] + 1
    print(f"{c.id} {what}: max err {err.max():.3e}, max err / bound {r:.3f}")
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        where = f"[n, ch, y, x] = {tuple(int(k) for k in i)}, channel block {int(i[1]) // 8}" if blocked else f"index {tuple(int(k) for k in i)}"
        raise AssertionError(f"{c.id} {what}: {int(bad.sum())} of {bad.size} elements beyond the bound; worst at {where}: got {got[i]!r}, "
                             f"want {want[i]!r}, err {err[i]:.3e}, bound {np.broadcast_to(bound, err.shape)[i]:.3e} (err / bound {r:.2f})")


def _guards(c, out, what):
    _, outside = out.split()
    assert outside.size and bool((outside == SENT).all()), f"{c.id}: guard channel blocks next to {what} were written"


def _w(o):
    return torch.from_numpy(o.w.astype(np.float32)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", [c for c in CASES if c.op == "fwd"], ids=lambda c: c.id)
def test_forward_equals_definition(c):
    from mmif import tensor as T
    o = PC.operands(c)
    (a, b), ins = _inputs(c, [o.a, o.b])
    r1 = r2 = None
    if c.res == "ops":
        r1, r2 = a, b
    elif c.res == "other":
        (r1, r2), rin = _inputs(c, [o.r1, o.r2])
        ins += rin
    out = _outputs(c, c.nout, 0)
    bias = torch.from_numpy(o.bias.astype(np.float32)).to(DEV) if c.bias else None
    prev = os.environ.get("MMIF_PAIR_STRIP")
    os.environ["MMIF_PAIR_STRIP"] = str(c.strip)          # read by the library at every call
    try:
        T.pairconv_fwd(a, b, _w(o), bias, c.nout, out.views[0], out.views[1] if c.nout == 2 else None, c.relu, r1, r2)
        torch.cuda.synchronize()
    finally:
        if prev is None:
            os.environ.pop("MMIF_PAIR_STRIP", None)
        else:
            os.environ["MMIF_PAIR_STRIP"] = prev
    _guards(c, out, "oa / ob")
    assert all(i.unchanged() for i in ins), f"{c.id}: an input was written"
    want, bounds = PC.def_fwd(c)
    got, _ = out.split()
    for name, g_, w_, b_ in zip(("oa", "ob"), got, want, bounds):
        _check(c, name, g_, w_, b_)


# ------------------------------------------------------------------------------------------------------------------------------ backward
def _backward_operands(c):
    o = PC.operands(c)
    (xa, xb), ins = _inputs(c, [o.a, o.b])
    gv, gin = _grad_inputs(c, o.g, c.g)
    ins += gin
    add = None
    if o.add is not None:
        (add,), ain = _grad_inputs(c, [o.add], c.add)
        ins += ain
    return o, xa, xb, gv[0], (gv[1] if c.nout == 2 else None), add, ins


def _check_gx(c, gx):
    _guards(c, gx, "gxa / gxb")
    want, bounds = PC.def_gx(c)
    got, _ = gx.split()
    for name, g_, w_, b_ in zip(("gxa", "gxb"), got, want, bounds):
        _check(c, name, g_, w_, b_)


def _check_dw(c, o, call):
    """call(dw, db, accumulate) runs the entry point.  accumulate = 0 onto garbage, twice: the definition, bit-identical; accumulate = 1 onto
    known values: the definition, and old + fresh within one fp32 rounding"""
    def run(acc, dw0, db0):
        dw, db = torch.from_numpy(dw0.astype(np.float32)).to(DEV), torch.from_numpy(db0.astype(np.float32)).to(DEV)
        call(dw, db, acc)
        torch.cuda.synchronize()
        return dw.cpu().numpy(), db.cpu().numpy()
    assert set(c.accumulate) == {0, 1}
    dw, db = run(0, np.full(o.dw_old.shape, 1e30), np.full(o.db_old.shape, -1e30))
    dw2, db2 = run(0, np.full(o.dw_old.shape, -7.0), np.full(o.db_old.shape, np.nan))
    assert np.array_equal(dw.view(np.int32), dw2.view(np.int32)) and np.array_equal(db.view(np.int32), db2.view(np.int32)), \
        f"{c.id}: dw / db differ between two consecutive calls"
    wdw, wdb, bdw, bdb = PC.def_wgrad(c, 0)
    _check(c, "dw acc=0", dw.astype(np.float64), wdw, bdw, blocked=False)
    _check(c, "db acc=0", db.astype(np.float64), wdb, bdb, blocked=False)
    dwa, dba = run(1, o.dw_old, o.db_old)
    wdw, wdb, bdw, bdb = PC.def_wgrad(c, 1)
    _check(c, "dw acc=1", dwa.astype(np.float64), wdw, bdw, blocked=False)
    _check(c, "db acc=1", dba.astype(np.float64), wdb, bdb, blocked=False)
    for name, new, old, fresh in (("dw", dwa, o.dw_old, dw), ("db", dba, o.db_old, db)):
        s = old + fresh.astype(np.float64)
        assert np.all(np.abs(new.astype(np.float64) - s) <= PC.U * np.abs(s)), f"{c.id}: accumulated {name} is not old + fresh within one fp32 rounding"


@pytest.mark.parametrize("c", [c for c in CASES if c.op == "dgrad"], ids=lambda c: c.id)
def test_input_gradient_equals_definition(c):
    from mmif import tensor as T
    o, xa, xb, ga, gb, add, ins = _backward_operands(c)
    gx = _outputs(c, 2, 1)
    m = c.mask_bits
    T.pairconv_dgrad(ga, gb, _w(o), c.nout, xa if m else None, xb if m else None, gx.views[0], gx.views[1], m, add=add)
    torch.cuda.synchronize()
    assert all(i.unchanged() for i in ins), f"{c.id}: an input was written"
    _check_gx(c, gx)


@pytest.mark.parametrize("c", [c for c in CASES if c.op == "wgrad"], ids=lambda c: c.id)
def test_weight_gradient_equals_definition(c):
    from mmif import tensor as T
    o, xa, xb, ga, gb, _add, ins = _backward_operands(c)
    ws = torch.empty(T.pairconv_wgrad_workspace_bytes() // 4, dtype=torch.float32, device=DEV)
    _check_dw(c, o, lambda dw, db, acc: T.pairconv_wgrad(xa, xb, ga, gb, c.nout, dw, db, ws, accumulate=bool(acc)))
    assert all(i.unchanged() for i in ins), f"{c.id}: an input was written"


@pytest.mark.parametrize("c", [c for c in CASES if c.op == "bwd"], ids=lambda c: c.id)
def test_fused_backward_equals_definition(c):
    """gx straight against the definition (not only against mmif_pairconv_dgrad), dw / db as for mmif_pairconv_wgrad"""
    from mmif import tensor as T
    from mmif._lib import MmifError
    o, xa, xb, ga, gb, add, ins = _backward_operands(c)
    ws = torch.empty(T.pairconv_wgrad_workspace_bytes() // 4, dtype=torch.float32, device=DEV)
    gx = _outputs(c, 2, 1)
    w = _w(o)

    def call(dw, db, acc):
        T.pairconv_bwd(ga, gb, w, c.nout, xa, xb, gx.views[0], gx.views[1], dw, db, ws, c.mask_bits, add=add, accumulate=bool(acc))
    _check_dw(c, o, call)
    assert all(i.unchanged() for i in ins), f"{c.id}: an input was written"
    _check_gx(c, gx)
    if add is not None and add.halo == 1:          # the same tensor, not flagged folded: refused before anything is launched
        raw = T.BT(add.buf, add.n, add.h, add.w, 1, add.cb_total, add.cb_off, add.cb, add.code, 0)
        d = torch.zeros(c.nout * 18, device=DEV)
        with pytest.raises(MmifError, match="folded first"):
            T.pairconv_bwd(ga, gb, w, c.nout, xa, xb, gx.views[0], gx.views[1], d, d[:c.nout], ws, c.mask_bits, add=raw)


def test_zz_report_error_over_bound():
    """prints the measured maximum of every entry point, storage type and output as a fraction of its bound ($MMIF_PAIR_SWEEP_REPORT: also as JSON)"""
    for k in sorted(RATIOS):
        r, e, n = RATIOS[k]
        print(f"{k:32s} max err/bound {r:8.4f}   max err {e:.3e}   checks {n}")
    path = os.environ.get("MMIF_PAIR_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)
