"""Every entry point of csrc/mixdw.hip against its fp64 definition (tests/mixdw_cases.py), element-wise, with derived bounds.

The C ABI is called through mmif._lib.lib on device buffers that sit between non-zero sentinel guards (a case's `guard` floats on either side:
3 puts the outputs off a 16-byte boundary, i.e. on the kernels' scalar-store path); the workspace is exactly the queried number of bytes with a
guard behind it.  After the calls: every output element within its bound, no sentinel left inside, guards untouched; the weight gradient run
twice is bit-identical; the wrappers of mmif/tensor.py and the autograd Function return the bits of the direct calls; MixConvBlock's one-launch
depth-wise stage agrees with its own per-layer path within the summed bounds."""
import ctypes

import numpy as np
import pytest
import torch

import mixdw_cases as MC
from mixdw_cases import CASES, SENT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_GUARD = 64


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
    """the three calls of a case on fresh buffers -> dict of output Bufs (db absent when NULL) and the workspace tensor"""
    from mmif._lib import lib
    from mmif.tensor import stream_ptr
    st = stream_ptr()
    g = c.guard
    x, gy, w = Buf(g, o["x"]), Buf(g, o["gy"]), Buf(g, o["w"])
    b = Buf(g, o["bias"]) if c.bias else None
    numel = x.size
    outs = dict(y=Buf(g, size=numel), dx=Buf(g, size=numel), dw=Buf(g, size=c.packed))
    if c.bias:
        outs["db"] = Buf(g, size=c.nseg * c.c)
    args = (c.n, c.c, c.nseg, c.k0, c.h, c.w)
    nbytes = lib.mmif_mixdw_wgrad_workspace(*args)
    assert nbytes == c.workspace_bytes
    ws = torch.full((nbytes // 4 + WS_GUARD,), 1e30, dtype=torch.float32, device=DEV)
    err = lambda: lib.mmif_last_error().decode()
    assert lib.mmif_mixdw_fwd(x.ptr, w.ptr, b.ptr if b else None, outs["y"].ptr, *args, int(c.reflect), st) == 0, err()
    assert lib.mmif_mixdw_dgrad(gy.ptr, w.ptr, outs["dx"].ptr, *args, int(c.reflect), st) == 0, err()
    assert lib.mmif_mixdw_wgrad(x.ptr, gy.ptr, outs["dw"].ptr, outs["db"].ptr if c.bias else None, *args, int(c.reflect),
                                ctypes.c_void_p(ws.data_ptr()), nbytes, st) == 0, err()
    torch.cuda.synchronize()
    assert bool((ws[nbytes // 4:] == 1e30).all()), "the workspace's guard was written"
    for name, buf in (("x", x), ("gy", gy), ("w", w)):
        assert buf.guards_untouched() and np.array_equal(buf.view.cpu().numpy(), np.asarray(o[name], np.float32).reshape(-1)), f"input {name} changed"
    return outs


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_case_within_its_bound(c):
    o = MC.operands(c)
    want, bound = MC.define(c, o), MC.bounds(c, o)
    outs = run_case(c, o)
    for name, buf in outs.items():
        got = buf.view.cpu().numpy().astype(np.float64)
        w, b = np.asarray(want[name]).reshape(-1), np.asarray(bound[name]).reshape(-1)
        assert buf.guards_untouched(), f"{name}: a guard was written"
        assert np.isfinite(got).all()
        err = np.abs(got - w)
        worst = int(np.argmax(err - b))
        print(f"{c.id} {name}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(b, 1e-300)):.3f}")
        assert (err <= b).all(), f"{name}[{worst}]: got {got[worst]!r}, want {w[worst]!r}, bound {b[worst]:.3e}"
    # a second weight gradient on fresh buffers: the same bits
    again = run_case(c, o)
    for name in ("dw", "db"):
        if name in outs:
            assert torch.equal(outs[name].view.view(torch.int32), again[name].view.view(torch.int32)), f"{name} differs between two runs"


def _seg_params(c, o):
    ws = [torch.from_numpy(np.ascontiguousarray(w, np.float32)).reshape(c.c, 1, k, k).to(DEV).requires_grad_() for w, k in zip(MC.unpack(c, o["w"]), c.ks)]
    bs = [t.clone().requires_grad_() for t in torch.from_numpy(o["bias"]).to(DEV).chunk(c.nseg)] if c.bias else []
    return ws, bs


@pytest.mark.parametrize("c", [c for c in CASES if c.n * c.c * c.nseg * c.h * c.w < 200000][::3], ids=lambda c: c.id)
def test_wrappers_and_autograd_function_return_the_same_bits(c):
    import core.block as B
    from mmif import tensor as T
    o = MC.operands(c)
    outs = run_case(c, o)
    x, gy, w = (torch.from_numpy(o[k]).to(DEV) for k in ("x", "gy", "w"))
    b = torch.from_numpy(o["bias"]).to(DEV) if c.bias else None
    shape = x.shape
    same = lambda a, buf: torch.equal(a.reshape(-1).view(torch.int32), buf.view.view(torch.int32))
    assert same(T.mixdw_fwd(x, w, b, c.nseg, c.k0, c.reflect), outs["y"])
    assert same(T.mixdw_dgrad(gy, w, c.nseg, c.k0, c.reflect), outs["dx"])
    dw, db = T.mixdw_wgrad(x, gy, c.nseg, c.k0, c.reflect, c.bias)
    assert same(dw, outs["dw"]) and (db is None) == (not c.bias) and (db is None or same(db, outs["db"]))
    ws, bs = _seg_params(c, o)
    xr = x.clone().requires_grad_()
    y = B._MixDwFn.apply(xr, c.k0, c.reflect, c.nseg, *ws, *bs)
    assert y.shape == shape and same(y, outs["y"])
    y.backward(gy)
    assert same(xr.grad, outs["dx"])
    assert same(torch.cat([t.grad.reshape(-1) for t in ws]), outs["dw"])
    if c.bias:
        assert same(torch.cat([t.grad for t in bs]), outs["db"])


@pytest.mark.parametrize("scale,hw,bias", [(4, (17, 65), False), (4, (4, 4), True), (2, (16, 63), True), (1, (5, 7), False)])
def test_mixconvblock_one_launch_against_its_own_per_layer_path(scale, hw, bias):
    """MixConvBlock._mix (one csrc/mixdw.hip launch per direction on the un-chunked tensor) against _mix_layers (chunk, one ConvLayer per group,
    concatenation) on the same weights: each side is within its bound of the same fp64 definition -- the fused side by the bounds of
    tests/mixdw_cases.py, the per-layer side by (k k + 1) u A forward, (9 k k + 1) u A dgrad (dwconv_dgrad_kernel's single chain over up to 9
    images) and, for the weight gradient, its one-block chain n ceil(hw / 256) + 11 (k <= 3; k = 5, 7 run the mixdw kernels there too)."""
    import core.block as B
    import torch.nn as nn
    torch.manual_seed(scale * 100 + hw[0])
    cin = 6
    blk = B.MixConvBlock(cin, cin, scale=scale, bias=bias).to(DEV)
    assert blk._fused
    if bias:
        for d in blk.dwconvs:
            nn.init.normal_(d.layers[0].bias)
    x = torch.randn(2, cin, *hw, device=DEV)
    c = MC.Case(n=2, c=cin, nseg=scale, k0=1, h=hw[0], w=hw[1], reflect=True, bias=bias)
    res = []
    for fused in (True, False):
        blk.zero_grad()
        z = blk.pwconv1(x).detach().requires_grad_()
        if fused:
            convs = [d.layers[0] for d in blk.dwconvs]
            y = B._MixDwFn.apply(z, 1, True, scale, *[m.weight for m in convs], *[m.bias for m in convs if m.bias is not None])
        else:
            y = blk._mix_layers(z)
        if fused:
            gy = torch.randn_like(y)
            zz = z.detach()
        y.backward(gy)
        res.append(dict(y=y.detach().cpu().numpy().astype(np.float64), dx=z.grad.cpu().numpy().astype(np.float64),
                        dw=torch.cat([d.layers[0].weight.grad.reshape(-1) for d in blk.dwconvs]).cpu().numpy().astype(np.float64),
                        db=torch.cat([d.layers[0].bias.grad for d in blk.dwconvs]).cpu().numpy().astype(np.float64) if bias else None))
    o = dict(x=zz.cpu().numpy(), gy=gy.cpu().numpy(), w=torch.cat([d.layers[0].weight.detach().reshape(-1) for d in blk.dwconvs]).cpu().numpy(),
             bias=torch.cat([d.layers[0].bias.detach() for d in blk.dwconvs]).cpu().numpy() if bias else None)
    bound = MC.bounds(c, o)
    kc = np.repeat(np.asarray(c.ks, np.float64), cin)[None, :, None, None]
    layer = dict(y=bound["y"], dx=(9 * kc * kc + 1) * MC.U * MC.dgrad(c, o, mag=True))
    adw, adb = MC.wgrad(c, o, mag=True)
    t_layer = max(2 * MC.cdiv(hw[0] * hw[1], 256) + 11, 16 + MC.cdiv(2 * c.tiles, 4))
    layer["dw"], layer["db"] = (t_layer + 1) * MC.U * adw, (t_layer + 1) * MC.U * adb
    # the block's own forward takes the one-launch path
    y_block = blk._mix(x)
    assert np.array_equal(y_block.detach().cpu().numpy().astype(np.float64), res[0]["y"])
    for name in ("y", "dx", "dw", "db"):
        if res[0][name] is None:
            continue
        tol = np.asarray(bound[name]).reshape(-1) + np.asarray(layer[name]).reshape(-1)
        err = np.abs(res[0][name].reshape(-1) - res[1][name].reshape(-1))
        print(f"scale {scale} {hw} {name}: max err {err.max():.3e}, max err / summed bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert (err <= tol).all(), name
