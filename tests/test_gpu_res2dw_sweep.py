"""Every entry point of csrc/res2dw.hip against its fp64 definition (tests/res2dw_cases.py), element-wise, with derived bounds.

The C ABI is called through mmif._lib.lib on device buffers that sit between non-zero sentinel guards (a case's `guard` floats on either side:
3 puts the outputs off a 16-byte boundary, i.e. on the kernels' scalar load / store path); the workspace is exactly the queried number of bytes
with a guard behind it.  After the calls: y and dx within the STAGE-WISE bound of the fp64 stage applied to the device's own previous segment
(what catches a wrong halo or reflect index) and within the END-TO-END bound of the full fp64 chain; dw and db, computed from the device's own
y and dx, within the bound of their accumulation chain; no sentinel left inside, guards and inputs untouched; a second run of all four outputs
on fresh buffers is bit-identical; every illegal argument class returns MMIF_EINVAL and a short workspace MMIF_EWORKSPACE."""
import ctypes

import numpy as np
import pytest
import torch

import res2dw_cases as RC
from res2dw_cases import CASES, SENT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_GUARD = 64
worst = {}      # output -> (max err / bound, max err) over the cases run so far; printed by every case and by the last test


class Buf:
    def __init__(self, guard, values=None, size=None):
        if values is not None:
            values = np.asarray(values, np.float32).reshape(-1)
            size = values.size
        self.size, self.off = size, guard
        self.full = torch.full((size + 2 * guard,), SENT, dtype=torch.float32, device=DEV)
        if values is not None:
            self.full[guard:guard + size] = torch.from_numpy(values).to(DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.full.data_ptr() + 4 * self.off)

    @property
    def view(self):
        return self.full[self.off:self.off + self.size]

    def guards_untouched(self):
        return bool((self.full[:self.off] == SENT).all()) and bool((self.full[self.off + self.size:] == SENT).all())


def run_case(c, o):
    """the four calls of a case on fresh buffers -> dict of output Bufs (db absent when NULL)"""
    from mmif._lib import lib
    from mmif.tensor import stream_ptr
    st = stream_ptr()
    g = c.guard
    x, gy, w = Buf(g, o["x"]), Buf(g, o["gy"]), Buf(g, o["w"])
    b = Buf(g, o["bias"]) if c.bias else None
    outs = dict(y=Buf(g, size=x.size), dx=Buf(g, size=x.size), dw=Buf(g, size=c.packed))
    if c.bias:
        outs["db"] = Buf(g, size=c.nseg * c.c)
    args = (c.n, c.c, c.nseg, c.h, c.w)
    nbytes = lib.mmif_res2dw_wgrad_workspace(*args)
    assert nbytes == c.workspace_bytes
    ws = torch.full((nbytes // 4 + WS_GUARD,), 1e30, dtype=torch.float32, device=DEV)
    err = lambda: lib.mmif_last_error().decode()
    assert lib.mmif_res2dw_fwd(x.ptr, w.ptr, b.ptr if b else None, outs["y"].ptr, *args, int(c.reflect), st) == 0, err()
    assert lib.mmif_res2dw_dgrad(gy.ptr, w.ptr, outs["dx"].ptr, *args, int(c.reflect), st) == 0, err()
    # a workspace one float short is refused before any launch; the queried size is enough
    assert lib.mmif_res2dw_wgrad(x.ptr, outs["y"].ptr, gy.ptr, outs["dx"].ptr, outs["dw"].ptr, outs["db"].ptr if c.bias else None, *args,
                                 int(c.reflect), ctypes.c_void_p(ws.data_ptr()), nbytes - 4, st) == RC.EWORKSPACE
    assert lib.mmif_res2dw_wgrad(x.ptr, outs["y"].ptr, gy.ptr, outs["dx"].ptr, outs["dw"].ptr, outs["db"].ptr if c.bias else None, *args,
                                 int(c.reflect), ctypes.c_void_p(ws.data_ptr()), nbytes, st) == 0, err()
    torch.cuda.synchronize()
    assert bool((ws[nbytes // 4:] == 1e30).all()), "the workspace's guard was written"
    for name, buf in (("x", x), ("gy", gy), ("w", w)):
        assert buf.guards_untouched() and np.array_equal(buf.view.cpu().numpy(), np.asarray(o[name], np.float32).reshape(-1)), f"input {name} changed"
    return outs


def _hold(c, kind, name, got, want, bound):
    got, w, b = got.reshape(-1), np.asarray(want).reshape(-1), np.asarray(bound).reshape(-1)
    err = np.abs(got - w)
    ratio = float(np.max(err / np.maximum(b, 1e-300)))
    key = f"{name} {kind}"
    worst[key] = (max(worst.get(key, (0, 0))[0], ratio), max(worst.get(key, (0, 0))[1], float(err.max())))
    print(f"{c.id} {key}: max err {err.max():.3e}, max err / bound {ratio:.3f}")
    i = int(np.argmax(err - b))
    assert (err <= b).all(), f"{key}[{i}]: got {got[i]!r}, want {w[i]!r}, bound {b[i]:.3e}"


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_case_within_its_bounds(c):
    o = RC.operands(c)
    outs = run_case(c, o)
    shape = (c.n, c.nseg * c.c, c.h, c.w)
    got = {}
    for name, buf in outs.items():
        assert buf.guards_untouched(), f"{name}: a guard was written"
        got[name] = buf.view.cpu().numpy()
        assert np.isfinite(got[name]).all() and not (got[name] == SENT).any(), f"{name}: an element was not written"
    y32, dx32 = got["y"].reshape(shape), got["dx"].reshape(shape)
    g64 = {k: v.astype(np.float64) for k, v in got.items()}
    # stage-wise: each segment against the fp64 stage on the device's own previous segment
    sw, sb = RC.stage_define(c, o, y32, dx32), RC.stage_bounds(c, o, y32, dx32)
    for name in ("y", "dx"):
        _hold(c, "stage", name, g64[name], sw[name], sb[name])
    # end to end: the full fp64 chain
    ew, eb = RC.define(c, o), RC.bounds(c, o)
    for name in ("y", "dx"):
        _hold(c, "chain", name, g64[name], ew[name], eb[name])
    # the weight gradient of the operands it was given: the device's own y and dx
    dw, db = RC.wgrad(c, o, y32, dx32)
    wb = RC.wgrad_bounds(c, o, y32, dx32)
    _hold(c, "sum", "dw", g64["dw"], dw, wb["dw"])
    if c.bias:
        _hold(c, "sum", "db", g64["db"], db, wb["db"])
    # a second run on fresh buffers: the same bits, all four outputs
    again = run_case(c, o)
    for name in outs:
        assert torch.equal(outs[name].view.view(torch.int32), again[name].view.view(torch.int32)), f"{name} differs between two runs"


def test_illegal_arguments_are_refused_before_any_launch():
    from mmif._lib import lib
    from mmif.tensor import stream_ptr
    st = stream_ptr()
    t = torch.full((4096,), SENT, dtype=torch.float32, device=DEV)
    p = ctypes.c_void_p(t.data_ptr())
    for (n, c, nseg, h, wd, reflect), msg in RC.ILLEGAL:
        a = (n, c, nseg, h, wd)
        assert lib.mmif_res2dw_fwd(p, p, None, p, *a, reflect, st) == RC.EINVAL and msg in lib.mmif_last_error(), a
        assert lib.mmif_res2dw_dgrad(p, p, p, *a, reflect, st) == RC.EINVAL and msg in lib.mmif_last_error(), a
        assert lib.mmif_res2dw_wgrad(p, p, p, p, p, None, *a, reflect, p, 4096 * 4, st) == RC.EINVAL and msg in lib.mmif_last_error(), a
        assert reflect or lib.mmif_res2dw_wgrad_workspace(*a) == 0
    torch.cuda.synchronize()
    assert bool((t == SENT).all())


@pytest.mark.parametrize("c", [c for c in CASES if c.numel < 100000][::4], ids=lambda c: c.id)
def test_wrappers_and_autograd_function_return_the_same_bits(c):
    import core.block as B
    from mmif import tensor as T
    o = RC.operands(c)
    outs = run_case(c, o)
    x, gy, w = (torch.from_numpy(o[k]).to(DEV) for k in ("x", "gy", "w"))
    b = torch.from_numpy(o["bias"]).to(DEV) if c.bias else None
    same = lambda a, buf: torch.equal(a.reshape(-1).view(torch.int32), buf.view.view(torch.int32))
    y = T.res2dw_fwd(x, w, b, c.nseg, c.reflect)
    dx = T.res2dw_dgrad(gy, w, c.nseg, c.reflect)
    assert same(y, outs["y"]) and same(dx, outs["dx"])
    dw, db = T.res2dw_wgrad(x, y, gy, dx, c.nseg, c.reflect, c.bias)
    assert same(dw, outs["dw"]) and (db is None) == (not c.bias) and (db is None or same(db, outs["db"]))
    ws = [torch.from_numpy(np.ascontiguousarray(t, np.float32)).reshape(c.c, 1, k, k).to(DEV).requires_grad_()
          for t, k in zip(RC.unpack(c, o["w"]), [1] + [3] * (c.nseg - 1))]
    bs = [t.clone().requires_grad_() for t in b.chunk(c.nseg)] if c.bias else []
    xr = x.clone().requires_grad_()
    yf = B._Res2DwFn.apply(xr, c.reflect, c.nseg, *ws, *bs)
    assert yf.shape == x.shape and same(yf, outs["y"])
    yf.backward(gy)
    assert same(xr.grad, outs["dx"]) and same(torch.cat([t.grad.reshape(-1) for t in ws]), outs["dw"])
    if c.bias:
        assert same(torch.cat([t.grad for t in bs]), outs["db"])


def test_report_the_worst_figures():
    """(the figures quoted in the docstring of tests/res2dw_cases.py and in DESIGN.md 4.8; holds nothing itself)"""
    for key in sorted(worst):
        print(f"worst over the cases run: {key}: max err / bound {worst[key][0]:.3f}, max err {worst[key][1]:.3e}")
