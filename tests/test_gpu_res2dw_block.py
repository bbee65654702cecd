"""Res2ConvBlock on the one-launch chain kernels of csrc/res2dw.hip against the same module forced through its per-layer path (_mix_layers:
chunk, layout-converting adds, one depth-wise ConvLayer per group, concatenation).  Tolerances: the project's own for this block
(test_res2_conv_block_vs_golden): y 2e-5, dx 5e-5, parameters 1e-4, relative to the largest element."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(y=2e-5, dx=5e-5, param=1e-4)

BLOCKS = {
    "16-32-s4": (dict(in_ch=16, out_ch=32, scale=4), (2, 16, 20, 36)),
    "6-8-s8-bias": (dict(in_ch=6, out_ch=8, scale=8, bias=True), (2, 6, 20, 36)),
    "6-8-s8-bias-3x5": (dict(in_ch=6, out_ch=8, scale=8, bias=True), (2, 6, 3, 5)),
    "16-32-s4-3x5": (dict(in_ch=16, out_ch=32, scale=4), (1, 16, 3, 5)),
}


def _block(kw, seed):
    import core.block as B
    torch.manual_seed(seed)
    blk = B.Res2ConvBlock(**kw).to(DEV)
    for p in blk.parameters():
        if p.dim() == 1:
            nn.init.normal_(p, std=0.5)     # (biases start at zero: give them something to carry)
    return blk


def _run(blk, x, gy, layers):
    """(y, dx, {name: grad}) of the module, routed as it routes itself or with its depth-wise stage forced through _mix_layers"""
    blk.zero_grad()
    xr = x.clone().requires_grad_()
    if layers:
        routed = blk._mix
        blk._mix = lambda t: blk._mix_layers(blk.pwconv1(t))
    try:
        y = blk(xr)
        y.backward(gy)
    finally:
        if layers:
            blk._mix = routed
    torch.cuda.synchronize()
    return y.detach(), xr.grad.detach(), {k: p.grad.detach().clone() for k, p in blk.named_parameters() if p.grad is not None}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_as_routed_agrees_with_its_per_layer_path(name):
    kw, shape = BLOCKS[name]
    blk = _block(kw, 7)
    assert blk._fused
    torch.manual_seed(11)
    x = torch.randn(*shape, device=DEV)
    gy = torch.randn(shape[0], kw["out_ch"], *shape[2:], device=DEV)
    y1, dx1, g1 = _run(blk, x, gy, layers=False)
    y0, dx0, g0 = _run(blk, x, gy, layers=True)
    print(f"{name}: y {_rel(y1, y0):.2e}, dx {_rel(dx1, dx0):.2e}, params {max(_rel(g1[k], g0[k]) for k in g0):.2e}")
    assert _rel(y1, y0) <= TOL["y"] and _rel(dx1, dx0) <= TOL["dx"]
    assert set(g1) == set(g0) == {k for k, _ in blk.named_parameters() if not k.startswith("dwconv.")}
    for k in g0:
        assert _rel(g1[k], g0[k]) <= TOL["param"], k


@pytest.mark.parametrize("name", ["16-32-s4", "6-8-s8-bias"])
def test_mix_on_a_device_tensor_is_the_one_launch_kernel(name):
    from mmif import tensor as T
    kw, shape = BLOCKS[name]
    blk = _block(kw, 3)
    torch.manual_seed(5)
    x = torch.randn(*shape, device=DEV)
    with torch.no_grad():
        z = blk.pwconv1(x)
        convs = [d.layers[0] for d in blk.dwconvs]
        wp = torch.cat([m.weight.reshape(-1) for m in convs])
        bp = torch.cat([m.bias for m in convs]) if convs[0].bias is not None else None
        assert wp.numel() == T.res2dw_packed_numel(kw["in_ch"], kw["scale"])
        want = T.res2dw_fwd(z, wp, bp, kw["scale"], True)
        got = blk._mix(x)
        layers = blk._mix_layers(z)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert _rel(layers, want) <= TOL["y"]


def test_a_block_with_a_norm_keeps_the_per_layer_path():
    import core.block as B
    torch.manual_seed(2)
    blk = B.Res2ConvBlock(6, 8, 4, norm=nn.BatchNorm2d).to(DEV).eval()
    assert not blk._fused
    x = torch.randn(2, 6, 20, 36, device=DEV)
    with torch.no_grad():
        got, want = blk._mix(x), blk._mix_layers(blk.pwconv1(x))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not B.Res2ConvBlock(2, 2, scale=9)._fused
