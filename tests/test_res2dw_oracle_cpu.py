"""No GPU: the fp64 definitions of tests/res2dw_cases.py equal torch's float64 autograd of the composition the kernels replace (chunk -> add ->
F.pad -> F.conv2d(groups) -> cat), the weight gradient's G_i / in_i identities included; the case table covers what it claims; every planted
wrong definition exceeds the bound on some case; include/mmif.h declares the entry points, mmif/_lib.py carries their prototypes, and the
library refuses every illegal argument combination before any launch; Res2ConvBlock decides its route as documented and keeps its layout."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import res2dw_cases as RC
from res2dw_cases import CASES, TH, TW, WTH, WTW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmif_res2dw_fwd", "mmif_res2dw_dgrad", "mmif_res2dw_wgrad_workspace", "mmif_res2dw_wgrad")
_memo = {}


def truth(c):
    """(operands, the four fp64 outputs, the end-to-end bounds + the weight gradient's): computed once per case and shared"""
    if c.id not in _memo:
        o = RC.operands(c)
        d = RC.define(c, o)
        b = RC.bounds(c, o)
        b.update(RC.wgrad_bounds(c, o, d["y"], d["dx"]))
        _memo[c.id] = (o, d, b)
    return _memo[c.id]


def _torch_composition(c, o):
    x = torch.from_numpy(o["x"]).double().requires_grad_()
    ws = [torch.from_numpy(np.ascontiguousarray(w)).double().reshape(c.c, 1, k, k).requires_grad_()
          for w, k in zip(RC.unpack(c, o["w"]), [1] + [3] * (c.nseg - 1))]
    b = torch.from_numpy(o["bias"]).double().requires_grad_() if c.bias else None
    xs = torch.chunk(x, c.nseg, dim=1)
    outs, y = [], None
    for i in range(c.nseg):
        y = y + xs[i] if i > 1 else xs[i]
        if i > 0:
            y = F.pad(y, (1, 1, 1, 1), mode="reflect" if c.reflect else "constant")
        y = F.conv2d(y, ws[i], b[i * c.c:(i + 1) * c.c] if c.bias else None, groups=c.c)
        outs.append(y)
    out = torch.cat(outs, dim=1)
    out.backward(torch.from_numpy(o["gy"]).double())
    return dict(y=out.detach().numpy(), dx=x.grad.numpy(), dw=torch.cat([w.grad.reshape(-1) for w in ws]).numpy(), db=b.grad.numpy() if c.bias else None)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_definitions_equal_torch_float64_autograd(c):
    o, got, _ = truth(c)
    want = _torch_composition(c, o)
    for name in ("y", "dx", "dw", "db"):
        if want[name] is None:
            continue
        g, w = np.asarray(got[name]).reshape(-1), want[name].reshape(-1)
        scale = max(np.abs(w).max(), 1e-30)
        assert np.abs(g - w).max() <= 1e-12 * scale * max(1, c.n * c.h * c.w) ** 0.5, name


def test_stage_wise_definitions_reproduce_the_chain_from_its_own_outputs():
    """fed the chain's own y / dx as `the device's`, the stage-wise definitions return the chain"""
    for c in CASES:
        o, d, _ = truth(c)
        s = RC.stage_define(c, o, d["y"].astype(np.float32), d["dx"].astype(np.float32))
        for name in ("y", "dx"):
            assert np.abs(s[name] - d[name]).max() <= 1e-5 * max(np.abs(d[name]).max(), 1e-30), (c.id, name)   # (the fp32 rounding of what is fed)
        sb = RC.stage_bounds(c, o, d["y"].astype(np.float32), d["dx"].astype(np.float32))
        assert all(sb[k].shape == d[k].shape and (sb[k][d[k] != 0] > 0).all() for k in ("y", "dx"))


def test_bounds_are_small_against_the_outputs():
    """no bound of y or dx exceeds 1e-3 of its output's scale (a weight gradient is a sum of random sign that may cancel: its bound is held
    to 1e-4 of the sum of its terms' magnitudes), none is zero where the output is not, and the end-to-end bound is no smaller than the stage's"""
    for c in CASES:
        o, want, bound = truth(c)
        sb = RC.stage_bounds(c, o, want["y"].astype(np.float32), want["dx"].astype(np.float32))
        for name in ("y", "dx", "dw", "db"):
            w, b = np.asarray(want[name]), np.asarray(bound[name])
            assert b.shape == w.shape
            if name in ("y", "dx"):
                assert b.max() <= 1e-3 * np.abs(w).max(), (c.id, name, b.max(), np.abs(w).max())
            else:
                mags = dict(zip(("dw", "db"), RC.wgrad(c, o, want["y"], want["dx"], mag=True)))[name]
                assert (b <= 1e-4 * mags).all(), (c.id, name)
            assert (b[w != 0] > 0).all(), (c.id, name)
        for name in ("y", "dx"):
            assert (bound[name] >= sb[name] * (1 - 1e-6)).all(), (c.id, name)


def test_the_table_covers_what_it_claims():
    assert {c.nseg for c in CASES} == set(RC.NSEGS) == {1, 2, 3, 4, 8}
    assert {c.c for c in CASES} >= {1, 3, 16, 48} and {c.n for c in CASES} >= {1, 2, 3}
    for nseg in RC.NSEGS:
        mine = [c for c in CASES if c.nseg == nseg]
        assert {c.reflect for c in mine} == {True, False} and {c.bias for c in mine} == {True, False}, nseg
        assert {c.guard for c in mine} == {3, 4}
        # every tile-edge class of the chain kernels: one below, at, one above the tile and two tiles plus one, in both axes
        assert {c.h for c in mine} >= {TH - 1, TH, TH + 1, 2 * TH + 1} and {c.w for c in mine} >= {TW - 1, TW, TW + 1, 2 * TW + 1}, nseg
    assert {c.h for c in CASES} >= {WTH - 1, WTH, WTH + 1, 2 * WTH + 1} and WTW == TW      # the weight gradient's tile
    assert any(c.h % TH not in (0, TH - 1) and c.w % TW not in (0, TW - 1) and c.h > TH and c.w > TW for c in CASES)    # ragged last tile, both axes
    # a chain of 8 crossing tile borders in both axes, under both paddings
    assert {c.reflect for c in CASES if c.nseg == 8 and (c.h > TH or c.w > TW)} == {True, False}
    assert any(c.nseg == 8 and c.h > TH and c.w > TW for c in CASES)
    for hw in RC.SMALL_REFLECT:
        assert hw in ((2, 2), (2, 5), (3, 3), (7, 4)) and any(c.reflect and c.nseg == 8 and (c.h, c.w) == hw for c in CASES)
    assert any(not c.reflect and (c.h, c.w) == (1, 1) for c in CASES) and any(not c.reflect and (c.h, c.w) == (1, 9) and c.nseg > 1 for c in CASES)
    assert any(c.n * c.c * c.tiles > RC.MAX_BLOCKS and c.n * c.c * c.nseg * c.wtiles > RC.MAX_BLOCKS for c in CASES)
    assert all(c.guard > 0 and RC.SENT != 0.0 for c in CASES)
    for c in CASES:
        assert c.workspace_bytes == c.n * c.c * c.nseg * c.wtiles * RC.SLOTS * 4
        assert not c.reflect or c.nseg < 2 or min(c.h, c.w) >= 2
        assert c.numel < 700000                                     # (every case well under a second)
    classes = {msg for _, msg in RC.ILLEGAL}
    assert classes == {b"nseg must be 1..8", b"bad arguments", b"reflect padding needs h,w >= 2", b"too many elements"}


def test_the_kernel_constants_are_the_tables():
    src = open(os.path.join(ROOT, "multi-modal-image-fusion_amd", "csrc", "res2dw.hip")).read()
    assert f"R2_TH = {TH}, R2_TW = {TW}" in src and f"R2_WTH = {WTH}, R2_WTW = {WTW};" in src and f"R2_MAX_BLOCKS = {RC.MAX_BLOCKS};" in src
    assert f"R2_SLOTS = {RC.SLOTS};" in src and f"R2_SUBS = {RC.SUBS};" in src and f"R2_SMAX = {RC.SMAX};" in src
    body = src.split("#include")[1]
    assert "atomic" not in body and "getenv" not in body and "hipMalloc" not in body and "Synchronize" not in body
    assert "res2dw.hip" in open(os.path.join(ROOT, "multi-modal-image-fusion_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("mut", sorted(RC.MUTATIONS))
def test_every_planted_wrong_definition_exceeds_the_bound_somewhere(mut):
    hit = []
    for c in CASES:
        o, true, bound = truth(c)
        wrong = RC.define(c, o, mut)
        for name in RC.MUTATIONS[mut]:
            t, w = np.asarray(true[name]), np.asarray(wrong[name])
            if t.shape == w.shape and (np.abs(t - w) > np.asarray(bound[name])).any():
                hit.append((c.id, name))
    assert hit, mut
    assert {n for _, n in hit} == set(RC.MUTATIONS[mut]), (mut, hit[:4])


def test_header_and_prototypes_declare_the_entry_points():
    from mmif._lib import SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mmif.h")).read()
    assert all(f"{n}(" in hdr for n in NAMES)
    assert all(n in SIGNATURES for n in NAMES)
    assert len(SIGNATURES["mmif_res2dw_fwd"][1]) == 11 and len(SIGNATURES["mmif_res2dw_dgrad"][1]) == 10
    assert len(SIGNATURES["mmif_res2dw_wgrad_workspace"][1]) == 5 and len(SIGNATURES["mmif_res2dw_wgrad"][1]) == 15


def test_library_exports_the_entry_points_and_validates_without_gpu():
    from mmif._lib import lib
    from mmif import tensor as T
    assert all(hasattr(lib, n) for n in NAMES)
    f = (ctypes.c_float * 64)()
    big = (ctypes.c_char * (1 << 16))()
    ws, nws = ctypes.addressof(big), 1 << 16
    for (n, c, nseg, h, wd, reflect), msg in RC.ILLEGAL:
        a = (n, c, nseg, h, wd)
        for call, who in ((lambda: lib.mmif_res2dw_fwd(f, f, None, f, *a, reflect, None), b"res2dw_fwd"),
                          (lambda: lib.mmif_res2dw_dgrad(f, f, f, *a, reflect, None), b"res2dw_dgrad"),
                          (lambda: lib.mmif_res2dw_wgrad(f, f, f, f, f, None, *a, reflect, ws, nws, None), b"res2dw_wgrad")):
            assert call() == RC.EINVAL, (a, who)
            err = lib.mmif_last_error()
            assert who + b":" in err and msg in err, (a, err)
        assert reflect or lib.mmif_res2dw_wgrad_workspace(*a) == 0        # (the query has no padding mode)
    # reflect padding of a lone 1 x 1 segment pads nothing: legal whatever the plane
    assert lib.mmif_res2dw_wgrad_workspace(1, 1, 1, 1, 1) == RC.SLOTS * 4
    # null pointers and a short workspace (legal geometry)
    a = (1, 1, 2, 4, 4)
    assert lib.mmif_res2dw_fwd(None, f, None, f, *a, 1, None) == -1 and b"res2dw_fwd: null pointer" in lib.mmif_last_error()
    assert lib.mmif_res2dw_dgrad(f, None, f, *a, 1, None) == -1 and b"res2dw_dgrad: null pointer" in lib.mmif_last_error()
    assert lib.mmif_res2dw_wgrad(f, f, f, None, f, None, *a, 1, ws, nws, None) == -1 and b"res2dw_wgrad: null pointer" in lib.mmif_last_error()
    need = lib.mmif_res2dw_wgrad_workspace(*a)
    assert need == 1 * 2 * 1 * RC.SLOTS * 4
    assert lib.mmif_res2dw_wgrad(f, f, f, f, f, None, *a, 1, ws, need - 4, None) == RC.EWORKSPACE and b"res2dw_wgrad: workspace" in lib.mmif_last_error()
    for c in CASES:
        assert lib.mmif_res2dw_wgrad_workspace(c.n, c.c, c.nseg, c.h, c.w) == c.workspace_bytes
        assert T.res2dw_packed_numel(c.c, c.nseg) == c.packed == truth(c)[0]["w"].size


def test_res2convblock_decides_its_route_and_keeps_its_layout():
    import core.block as B
    blk = B.Res2ConvBlock(16, 32, 4)
    assert blk._fused and [d.layers[0].kernel_size for d in blk.dwconvs] == [(1, 1), (3, 3), (3, 3), (3, 3)]
    assert B.Res2ConvBlock(48, 64, 8)._fused and B.Res2ConvBlock(6, 8, 8, bias=True)._fused
    assert not B.Res2ConvBlock(4, 4, norm=nn.BatchNorm2d)._fused and not B.Res2ConvBlock(2, 2, scale=9)._fused
    sd = blk.state_dict()
    assert [k for k in sd if k.startswith("dwconvs.")] == [f"dwconvs.{i}.layers.0.weight" for i in range(4)] and "dwconv.layers.0.weight" in sd
    assert hasattr(blk, "_mix_layers") and hasattr(B, "_Res2DwFn")
    # a CPU tensor keeps the per-layer path, which has no CPU kernels: the same error as before
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        blk(torch.zeros(1, 16, 8, 8))
