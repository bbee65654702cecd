"""tests/general_cases.py without a GPU: its fp64 definitions of csrc/conv_general.hip's and csrc/resample.hip's entry points against torch's
float64 operators and their autograd (F.conv2d on F.pad, F.conv_transpose2d, groups = c, F.max_pool2d(return_indices=True), F.interpolate(
align_corners=True), nn.Upsample('nearest'), nn.ReflectionPad2d with negative amounts, aten.threshold_backward), against
oracle.fusion_oracle and the recorded reference arrays of tests/golden; the case table shown to hold every entry point declared in
include/mmif.h and every edge class it claims; the planted values counted in the stored operands; no bound beyond 1e-3 of its output's scale
unless the output says why; every listed wrong definition shown to leave the true one's bound.

Agreement with torch float64 is to TOL = 1e-12 of the largest value (both sides sum the same float64 terms in another order: 2^-53 times a few
hundred terms).  The bilinear definition takes its source coordinate in fp32, as the kernel, ATen's float32 path and the numpy oracle do, while
torch's float64 operator takes it in float64: the two differ by the rounding of r and of r Y, at most 3 u s per weight (BL_TOL)."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import general_cases as GC
from general_cases import CASES, Case
from oracle import fusion_oracle as O
from test_oracle_golden import F11_CASES, F15_LAYERS, f11_tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-12
BIG = 300_000          # elements: the cases above this are pinned through their small siblings of the same geometry class


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    return t.requires_grad_(True) if grad else t


def _nerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def _want(c, o, name="", mut=None):
    outs = GC.define(c, mut, o)
    return outs[0].want if not name else next(d.want for d in outs if d.name == name)


def _by(ep, small=True):
    return [c for c in CASES if c.ep == ep and (not small or c.n * max(c.cin, c.cout) * c.h * c.w <= BIG)]


# ------------------------------------------------------------------------------------------------------------------------------ torch
@pytest.mark.parametrize("c", _by("gconv_fwd") + _by("gconv_dgrad") + _by("gconv_wgrad"), ids=lambda c: c.id)
def test_conv_definitions_equal_torch_float64_autograd(c):
    """the case's geometry through all three definitions: forward (bias, ReLU), input gradient and weight / bias gradient on the masked gy"""
    r = np.random.default_rng(c.h * 1000 + c.w)
    x, w, b = r.standard_normal((c.n, c.cin, c.h, c.w)), r.standard_normal((c.cout, c.cin, c.k, c.k)), r.standard_normal(c.cout)
    tx, tw, tb = _t(x, True), _t(w, True), _t(b, True)
    xp = F.pad(tx, (c.p,) * 4, mode="reflect" if c.reflect else "constant") if c.p else tx
    z = F.conv2d(xp, tw, tb if c.bias else None, stride=c.s)
    y = torch.relu(z) if c.relu else z
    assert tuple(y.shape) == (c.n, c.cout, c.ho, c.wo)
    cf = Case("gconv_fwd", **{k: getattr(c, k) for k in ("n", "cin", "cout", "h", "w", "k", "s", "p", "reflect", "bias", "relu")})
    assert _nerr(_want(cf, dict(x=x, w=w, bias=b if c.bias else None)), y.detach().numpy()) <= TOL
    gy = r.standard_normal(tuple(y.shape))
    y.backward(_t(gy))
    masked = gy * (y.detach().numpy() > 0) if c.relu else gy
    assert _nerr(_want(dataclasses.replace(cf, ep="gconv_dgrad"), dict(gy=masked, w=w)), tx.grad.numpy()) <= TOL
    cw = dataclasses.replace(cf, ep="gconv_wgrad", db=True)
    assert _nerr(_want(cw, dict(x=x, gy=masked), "dw"), tw.grad.numpy()) <= TOL
    assert _nerr(_want(cw, dict(x=x, gy=masked), "db"), masked.sum((0, 2, 3))) <= TOL
    if c.bias:
        assert _nerr(_want(cw, dict(x=x, gy=masked), "db"), tb.grad.numpy()) <= TOL


@pytest.mark.parametrize("c", _by("gconvt_fwd") + _by("gconvt_dgrad") + _by("gconvt_wgrad"), ids=lambda c: c.id)
def test_transposed_conv_definitions_equal_torch_float64_autograd(c):
    r = np.random.default_rng(c.h * 1000 + c.w + 7)
    x, w, b = r.standard_normal((c.n, c.cin, c.h, c.w)), r.standard_normal((c.cin, c.cout, c.k, c.k)), r.standard_normal(c.cout)
    tx, tw = _t(x, True), _t(w, True)
    y = F.conv_transpose2d(tx, tw, _t(b), stride=c.s, padding=c.p, output_padding=c.op)
    assert tuple(y.shape) == (c.n, c.cout, c.Ho, c.Wo)
    cf = dataclasses.replace(c, ep="gconvt_fwd", bias=True, relu=False, db=True)
    assert _nerr(_want(cf, dict(x=x, w=w, bias=b)), y.detach().numpy()) <= TOL
    gy = r.standard_normal(tuple(y.shape))
    y.backward(_t(gy))
    assert _nerr(_want(dataclasses.replace(cf, ep="gconvt_dgrad"), dict(gy=gy, w=w)), tx.grad.numpy()) <= TOL
    assert _nerr(_want(dataclasses.replace(cf, ep="gconvt_wgrad"), dict(x=x, gy=gy), "dw"), tw.grad.numpy()) <= TOL
    assert _nerr(_want(dataclasses.replace(cf, ep="gconvt_wgrad"), dict(x=x, gy=gy), "db"), x.sum((0, 2, 3))) <= TOL


@pytest.mark.parametrize("c", _by("dwconv_fwd") + _by("patchconv_fwd") + _by("patchconv_wgrad"), ids=lambda c: c.id)
def test_depthwise_and_patch_definitions_equal_torch_float64_autograd(c):
    fam = "dwconv" if c.ep.startswith("dw") else "patchconv"
    r = np.random.default_rng(c.h * 1000 + c.w + 3)
    x, w, b = r.standard_normal((c.n, c.cin, c.h, c.w)), r.standard_normal((c.cin, 1, c.k, c.k)), r.standard_normal(c.cin)
    tx, tw, tb = _t(x, True), _t(w, True), _t(b, True)
    if fam == "dwconv":
        p = c.k // 2
        xp = F.pad(tx, (p,) * 4, mode="reflect" if c.reflect else "constant") if p else tx
        y = F.conv2d(xp, tw, tb, groups=c.cin)
    else:
        y = F.conv2d(tx, tw, tb, stride=c.k, groups=c.cin)
    cf = dataclasses.replace(c, ep=fam + "_fwd", bias=True, db=True)
    assert _nerr(_want(cf, dict(x=x, w=w, bias=b)), y.detach().numpy()) <= TOL
    gy = r.standard_normal(tuple(y.shape))
    y.backward(_t(gy))
    assert _nerr(_want(dataclasses.replace(cf, ep=fam + "_dgrad"), dict(gy=gy, w=w)), tx.grad.numpy()) <= TOL
    assert _nerr(_want(dataclasses.replace(cf, ep=fam + "_wgrad"), dict(x=x, gy=gy), "dw"), tw.grad.numpy()) <= TOL
    assert _nerr(_want(dataclasses.replace(cf, ep=fam + "_wgrad"), dict(x=x, gy=gy), "db"), tb.grad.numpy()) <= TOL
    if fam == "patchconv":          # what the kernel does not read gets exactly +0.0
        dx = _want(dataclasses.replace(cf, ep="patchconv_dgrad"), dict(gy=gy, w=w))
        rest = dx[:, :, (c.h // c.k) * c.k:], dx[:, :, :, (c.w // c.k) * c.k:]
        assert all(not a.any() and not np.signbit(a).any() for a in rest)


@pytest.mark.parametrize("c", _by("relu_bwd") + _by("channel_sum"), ids=lambda c: c.id)
def test_relu_backward_and_channel_sum_equal_torch(c):
    o = GC.operands(c)
    if c.ep == "relu_bwd":
        want = torch.ops.aten.threshold_backward(_t(o["g"]).float(), _t(o["y"]).float(), 0.0).numpy()
        got = _want(c, o).astype(np.float32)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))          # the bits: a -0.0 gradient passes as -0.0, a blocked one is +0.0
    else:
        assert _nerr(_want(c, o), _t(o["x"]).sum((0, 2)).numpy()) <= TOL


BL_TOL = 3 * GC.U          # times the source coordinate, per weight


@pytest.mark.parametrize("c", _by("bilinear_up_fwd") + _by("bilinear_up_bwd"), ids=lambda c: c.id)
def test_bilinear_definition_equals_torch_float64(c):
    r = np.random.default_rng(c.H * 100 + c.W)
    x = r.standard_normal((1, c.n, c.h, c.w))
    tx = _t(x, True)
    y = F.interpolate(tx, size=(c.H, c.W), mode="bilinear", align_corners=True)
    tol = BL_TOL * (c.h + c.w) * 4
    assert _nerr(_want(dataclasses.replace(c, ep="bilinear_up_fwd", plant=""), dict(x=x[0])), y.detach().numpy()[0]) <= tol
    g = r.standard_normal((c.n, c.H, c.W))
    y.backward(_t(g[None]))
    assert _nerr(_want(dataclasses.replace(c, ep="bilinear_up_bwd", plant=""), dict(g=g)), tx.grad.numpy()[0]) <= tol
    ones = _want(dataclasses.replace(c, ep="bilinear_up_bwd", plant="ones"), dict(g=np.ones((c.n, c.H, c.W))))
    assert np.allclose(ones.reshape(c.n, -1).sum(1), c.H * c.W, rtol=1e-12)          # the transpose keeps the mass


@pytest.mark.parametrize("c", _by("maxpool_nchw_fwd"), ids=lambda c: c.id)
def test_maxpool_definition_equals_torch(c):
    """values everywhere (NaN as NaN); indices wherever a window holds at most one NaN (ATen keeps the LAST NaN of a window, the kernel and the
    definition the first: the header promises 'the first maximum' and says nothing of NaN); the backward as autograd routes it"""
    o = GC.operands(c)
    k = c.k
    tx = _t(o["x"][None], True)
    y, ti = F.max_pool2d(tx, k, k, return_indices=True)
    outs = {d.name: d.want for d in GC.define(c)}
    assert np.array_equal(outs["y"], y.detach().numpy()[0], equal_nan=True)
    ti = ti.numpy()[0]
    oy, ox = np.meshgrid(np.arange(c.h // k), np.arange(c.w // k), indexing="ij")
    tidx = (ti // c.w - oy * k) * k + (ti % c.w - ox * k)
    many_nan = np.isnan(GC.pool_windows(o["x"], k)).sum(-1) > 1
    assert np.array_equal(outs["idx"][~many_nan], tidx[~many_nan]) and outs["idx"].dtype == np.uint8
    clean = np.nan_to_num(o["x"], nan=9.0, neginf=-9.0)
    cx = _t(clean[None], True)
    cy = F.max_pool2d(cx, k, k)
    g = np.random.default_rng(k).standard_normal(tuple(cy.shape[1:]))
    cy.backward(_t(g[None]))
    idx = GC.define(c, o=dict(x=clean))[1].want
    assert np.array_equal(_want(dataclasses.replace(c, ep="maxpool_nchw_bwd"), dict(g=g, idx=idx)), cx.grad.numpy()[0])


@pytest.mark.parametrize("c", _by("nearest_up_bwd") + _by("reflect_pad_bwd"), ids=lambda c: c.id)
def test_nearest_and_reflect_pad_definitions_equal_torch(c):
    r = np.random.default_rng(c.h * 10 + c.w)
    x = GC.f32(r.standard_normal((c.n, c.h, c.w)))
    tx = _t(x[None], True)
    if c.ep == "nearest_up_bwd":
        y, fwd = nn.Upsample(scale_factor=c.k, mode="nearest")(tx), "nearest_up_fwd"
    else:
        y, fwd = nn.ReflectionPad2d(c.pads)(tx), "reflect_pad_fwd"
    assert np.array_equal(_want(dataclasses.replace(c, ep=fwd), dict(x=x)), y.detach().numpy()[0])
    g = r.standard_normal(tuple(y.shape[1:]))
    y.backward(_t(g[None]))
    assert _nerr(_want(c, dict(g=g)), tx.grad.numpy()[0]) <= TOL


# ------------------------------------------------------------------------------------------------------------------------------ oracle, golden
@pytest.mark.parametrize("case", F11_CASES, ids=[c[0] for c in F11_CASES])
def test_definitions_reproduce_the_recorded_general_conv_arrays(case):
    """tests/golden/f11_general_conv.npz (the reference's ConvLayer in float32) and oracle.fusion_oracle.conv2d_general_* / conv_transpose2d_*"""
    name, cin, cout, k, stride, transposed, pmode, relu, N, H, W = case
    g = np.load(os.path.join(GOLD, "f11_general_conv.npz"))
    w, b, x = (a.astype(np.float64) for a in f11_tensors(case))
    fam = "gconvt" if transposed else "gconv"
    c = Case(fam + "_fwd", n=N, cin=cin, cout=cout, h=H, w=W, k=k, s=stride, p=k // 2, op=1 if transposed else 0, reflect=pmode == "reflect", relu=relu)
    y = _want(c, dict(x=x, w=w, bias=b))
    gy = O.closed_form_signed(y.shape, 1.5, 1.0).astype(np.float64)
    masked = gy * (y > 0) if relu else gy
    dx = _want(dataclasses.replace(c, ep=fam + "_dgrad"), dict(gy=masked, w=w))
    dw = _want(dataclasses.replace(c, ep=fam + "_wgrad"), dict(x=x, gy=masked), "dw")
    db = masked.sum((0, 2, 3)) if transposed else _want(dataclasses.replace(c, ep=fam + "_wgrad"), dict(x=x, gy=masked), "db")
    x32, w32, b32 = (a.astype(np.float32) for a in (x, w, b))
    if transposed:
        oy = O.conv_transpose2d_fwd(x32, w32, b32, stride, k // 2, 1, relu)
        ob = O.conv_transpose2d_bwd(x32, w32, oy, gy.astype(np.float32), stride, k // 2, 1, relu)
    else:
        oy = O.conv2d_general_fwd(x32, w32, b32, stride, k // 2, pmode == "reflect", relu)
        ob = O.conv2d_general_bwd(x32, w32, oy, gy.astype(np.float32), stride, k // 2, pmode == "reflect", relu)
    for got, key, orc in ((y, "_y", oy), (dx, "_dx", ob[0]), (dw, "_dw", ob[1]), (db, "_db", ob[2])):
        ref = g[name + key]
        # (a ReLU near-tie of the float32 reference may flip against float64: its gy, of order 1, then shows in dx / dw; none does at these inputs)
        assert np.abs(got - ref).max() <= 3e-6 * max(1.0, np.abs(ref).max()), (name, key, np.abs(got - ref).max())
        assert np.abs(got - orc).max() <= 3e-6 * max(1.0, np.abs(orc).max()), (name, key, "oracle")


@pytest.mark.parametrize("case", [c for c in F15_LAYERS if c[1].get("groups", 1) > 1], ids=lambda c: c[0])
def test_definitions_reproduce_the_recorded_depthwise_layer_arrays(case):
    name, kw, shape = case
    g = np.load(os.path.join(GOLD, "f15_n4_res2.npz"))
    k, has_bias = kw["ksize"], kw.get("bias", True)
    w = O.closed_form_param(0, "layers.0.weight", (shape[1], 1, k, k), 15).astype(np.float64)
    b = O.closed_form_param(1, "layers.0.bias", (shape[1],), 15).astype(np.float64) if has_bias else None
    x = O.closed_form_signed(shape, 0.5, 1.0).astype(np.float64)
    c = Case("dwconv_fwd", n=shape[0], cin=shape[1], h=shape[2], w=shape[3], k=k, reflect=True, bias=has_bias)
    y = _want(c, dict(x=x, w=w, bias=b))
    gy = O.closed_form_signed(y.shape, 1.5, 1.0).astype(np.float64)
    dx = _want(dataclasses.replace(c, ep="dwconv_dgrad"), dict(gy=gy, w=w))
    wg = {d.name: d.want for d in GC.define(dataclasses.replace(c, ep="dwconv_wgrad"), o=dict(x=x, gy=gy))}
    pairs = [(y, "_y"), (dx, "_dx"), (wg["dw"], "_dp_layers.0.weight")] + ([(wg["db"], "_dp_layers.0.bias")] if has_bias else [])
    oy = O.dwconv_fwd(x.astype(np.float32), w.astype(np.float32), None if b is None else b.astype(np.float32), True)
    ob = O.dwconv_bwd(x.astype(np.float32), w.astype(np.float32), gy.astype(np.float32), True)
    for (got, key), orc in zip(pairs, (oy,) + tuple(ob)):
        ref = g[name + key]
        assert np.abs(got - ref).max() <= 3e-6 * max(1.0, np.abs(ref).max()), (name, key)
        assert np.abs(got - orc).max() <= 3e-6 * max(1.0, np.abs(orc).max()), (name, key, "oracle")


@pytest.mark.parametrize("name,shape,scale", [("bl_x2", (2, 3, 5, 7), 2), ("bl_x8", (1, 4, 4, 3), 8), ("bl_x2_row", (1, 2, 1, 6), 2)])
def test_bilinear_definition_reproduces_the_recorded_arrays_and_the_oracle(name, shape, scale):
    """the bl_* arrays of tests/golden/f12_n4_models.npz (the reference's Upsample('bilinear') in float32 on x = closed_form_signed(shape, 0.4, 1.0),
    gy = closed_form_signed(target, 1.3, 1.0): tests/golden/make_golden.py make_f12) and oracle.fusion_oracle.bilinear_up_*, whose fp32 source
    coordinates the definition shares bit for bit.  Tolerances: the recorded forward is the same fp32 expression the kernel evaluates, so the
    definition's own forward bound holds for it; the recorded backward is ATen's scatter, which adds the up to Tx Ty contributions of an input
    pixel one by one where the kernel adds Tx, then Ty: (Tx Ty + 1) u A on top of the definition's bound (bl_x8, 256 contributions per pixel: 5.2e-6 shown against
    a worst-case 1.7e-3 at that element; bl_x2: 2.4e-7 against 6.0e-6).  The numpy oracle's backward forms 1 - l in float32 (u per weight, two axes and their product: 3 u A), sums in float64 and rounds once (u |dx|)."""
    g = np.load(os.path.join(GOLD, "f12_n4_models.npz"))
    N, C, h, w = shape
    H, W = h * scale, w * scale
    assert g[name + "_y"].shape == (N, C, H, W) and g[name + "_dx"].shape == shape
    for hh, HH in ((h, H), (w, W)):
        y0, y1, l = O._bilinear_weights(hh, HH)
        d0, d1, dl, _ = GC.bl_weights(hh, HH)
        assert np.array_equal(y0, d0) and np.array_equal(y1, d1) and np.array_equal(l.astype(np.float64), dl)
    x, gy = O.closed_form_signed(shape, 0.4, 1.0), O.closed_form_signed((N, C, H, W), 1.3, 1.0)
    c = Case("bilinear_up_fwd", n=N * C, h=h, w=w, H=H, W=W)
    fy = GC.define(c, o=dict(x=x.astype(np.float64).reshape(N * C, h, w)))[0]
    fdx = GC.define(dataclasses.replace(c, ep="bilinear_up_bwd"), o=dict(g=gy.astype(np.float64).reshape(N * C, H, W)))[0]
    y, dx = fy.want.reshape(N, C, H, W), fdx.want.reshape(shape)
    assert np.all(np.abs(y - g[name + "_y"]) <= fy.bound.reshape(y.shape))
    (My, _, _), (Mx, _, _) = GC.bl_mats(h, H), GC.bl_mats(w, W)
    A = np.einsum("Yy,pYX,Xx->pyx", My, np.abs(gy.astype(np.float64)).reshape(N * C, H, W), Mx)
    TxTy = int((Mx != 0).sum(0).max() * (My != 0).sum(0).max())
    tol = (fdx.bound + (TxTy + 1) * GC.U * A).reshape(shape)
    err = np.abs(dx - g[name + "_dx"])
    print(f"{name}: dx max err {err.max():.2e}, tolerance at that element {tol.reshape(-1)[err.argmax()]:.2e}")
    assert np.all(err <= tol)
    oy, odx = O.bilinear_up_fwd(x, scale), O.bilinear_up_bwd(gy, (h, w))
    assert np.all(np.abs(y - oy) <= fy.bound.reshape(y.shape)) and np.all(np.abs(dx - odx) <= (3 * GC.U * A + GC.U * np.abs(fdx.want)).reshape(shape))


# ------------------------------------------------------------------------------------------------------------------------------ the table
def _extern_c(path):
    return set(re.findall(r'extern\s+"C"\s+[\w\s\*]+?\b(mmif_[a-z0-9_]+)\s*\(', open(path).read()))


def test_every_declared_entry_point_of_the_two_files_has_a_case():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmif.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mmif_[a-z0-9_]+)\s*\(", hdr))
    csrc = os.path.join(ROOT, "multi-modal-image-fusion_amd", "csrc")
    family = (_extern_c(os.path.join(csrc, "conv_general.hip")) | _extern_c(os.path.join(csrc, "resample.hip"))) & declared
    assert len(family) >= 25, sorted(family)
    covered = {"mmif_" + c.ep for c in CASES} | {GC.WORKSPACE_OF[c.ep] for c in CASES if c.ep in GC.WORKSPACE_OF}
    assert family == covered, (sorted(family - covered), sorted(covered - family))
    assert set(GC.EPS) == {c.ep for c in CASES}


def test_the_table_covers_what_it_claims():
    for ep in ("gconv_fwd", "gconv_dgrad", "gconv_wgrad"):
        cs = [c for c in CASES if c.ep == ep]
        assert {1, 15, 16, 17, 33} <= {c.ho for c in cs} | {c.wo for c in cs}, ep
        assert any(c.ho != c.wo for c in cs)
        assert {c.cin for c in cs} >= ({7, 8, 9} if ep == "gconv_wgrad" else {1, 3, 4, 5, 9}), ep
        assert {c.cout for c in cs} >= {1, 7, 8, 9, 17}, ep
        geoms = {(c.k, c.s, c.p, c.reflect) for c in cs}
        want = {(k, s, p, r) for (k, s, p) in GC.GEOMS for r in (False, True) if not (r and p == 0)}
        assert want <= geoms and len(want) == 28, (ep, sorted(want - geoms))
        assert any(0 < c.p < c.k // 2 for c in cs) and any(c.p == 0 and c.k > 1 for c in cs) and any(c.k == 7 and c.s == 2 for c in cs)
        for s2 in (0, 1):
            assert any(c.s == 2 and (c.h + 2 * c.p - c.k) % 2 == s2 for c in cs), (ep, s2)
        assert any(c.reflect and c.h == c.p + 1 and c.w == c.p + 1 for c in cs) and any(c.reflect and c.h == 3 and c.p == 2 for c in cs)
        assert any(c.reflect and c.h == 4 and c.p == 3 for c in cs)
        assert {c.n for c in cs} >= {1, 3} and any(c.offset for c in cs) and any(not c.offset for c in cs)
    assert {(c.bias, c.relu) for c in CASES if c.ep == "gconv_fwd"} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c.db for c in CASES if c.ep == "gconv_wgrad"} == {False, True}
    wg = [c for c in CASES if c.ep == "gconv_wgrad"]
    assert any(c.wg()[2] > 1 and c.wg()[0] % c.wg()[1] for c in wg), "no ragged second trip of the tile loop"
    assert any(c.wg()[3] > 1024 for c in wg) and any(c.wg()[3] > 1024 and c.wg()[0] > 1 for c in wg)
    assert any(c.k == 7 and 256 < WG * 49 < 512 for c in wg for WG in (GC.WG_CC,))
    ct = [c for c in CASES if c.transposed]
    for ep in ("gconvt_fwd", "gconvt_dgrad", "gconvt_wgrad"):
        assert {(c.k, c.s, c.p, c.op) for c in ct if c.ep == ep} == set(GC.CONVT_GEOMS), ep
        assert any(max(c.Ho, c.Wo) > 16 for c in ct if c.ep == ep) and any(c.Ho in (15, 16, 17) or c.Wo in (15, 16, 17) for c in ct if c.ep == ep)
    assert {c.bias for c in ct if c.ep == "gconvt_fwd"} == {False, True} and {c.db for c in ct if c.ep == "gconvt_wgrad"} == {False, True}
    for ep in ("gconvt_fwd", "gconvt_dgrad", "gconvt_wgrad"):          # the same channel edges as the plain conv
        assert {c.cin for c in ct if c.ep == ep} >= ({7, 8, 9} if ep == "gconvt_wgrad" else {1, 3, 4, 5, 9}), ep
        assert {c.cout for c in ct if c.ep == ep} >= {1, 7, 8, 9, 17} and {c.n for c in ct if c.ep == ep} >= {1, 3}, ep
    assert {c.relu for c in ct if c.ep == "gconvt_fwd"} == {False, True}
    tw = [c for c in ct if c.ep == "gconvt_wgrad"]          # the alias's own tile loop and workspace branch
    assert any(c.wg()[2] > 1 and c.wg()[0] % c.wg()[1] for c in tw) and any(c.wg()[3] > 1024 and c.wg()[0] > 1 for c in tw)
    assert sum(c.wg()[2] > 1 and c.wg()[0] % c.wg()[1] > 0 and c.wg()[3] <= 1024 for c in wg) >= 2
    assert {c.h for c in CASES if c.ep == "relu_bwd"} == {0, 1, 255, 256, 257}
    assert {(c.h, c.cin) for c in CASES if c.ep == "channel_sum"} == {(hw, ch) for hw in (1, 255, 256, 257, 1000) for ch in (1, 5)}
    assert all(c.n == 3 for c in CASES if c.ep == "channel_sum")
    for ep in ("dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad"):
        cs = [c for c in CASES if c.ep == ep]
        flag = (lambda c: c.bias) if ep == "dwconv_fwd" else (lambda c: c.db)
        assert {(c.k, c.reflect, flag(c)) for c in cs} == {(k, r, f) for k in (1, 3) for r in (False, True) for f in (False, True)}, ep
        assert {(c.h, c.w) for c in cs} == set(GC.DW_HW) and {c.cin for c in cs} == {1, 3, 5} and all(c.n == 3 for c in cs)
        assert any(c.h * c.w > 256 and (c.h * c.w) % 256 for c in cs) and any(c.h == 2 and c.k == 3 and c.reflect for c in cs)
    for ep in ("patchconv_fwd", "patchconv_dgrad", "patchconv_wgrad"):
        cs = [c for c in CASES if c.ep == ep]
        assert {c.k for c in cs} == set(GC.PATCH_S) == {2, 3, 4, 7, 8, 11, 16}
        assert {c.patch_L() for c in cs} == {4, 8, 16, 32, 64} and any(c.k * c.k > c.patch_L() for c in cs) and any(256 % (c.k * c.k) for c in cs)
        assert any(c.h % c.k and c.w % c.k for c in cs) and any(c.h % c.k == 0 and c.w % c.k == 0 for c in cs), ep
    pw = [c for c in CASES if c.ep == "patchconv_wgrad"]
    assert {c.patch_rows() for c in pw} == {1, 63, 64, 65, 130} and {c.db for c in pw} == {False, True}
    assert {c.bias for c in CASES if c.ep == "patchconv_fwd"} == {False, True}
    for ep in ("bilinear_up_fwd", "bilinear_up_bwd"):
        cs = [c for c in CASES if c.ep == ep]
        assert {(c.h, c.H) for c in cs} == set(GC.BILINEAR), ep
        assert any((c.h, c.H) != (c.w, c.W) for c in cs) and {c.n for c in cs} == {1, 6}
    assert sum(c.plant == "ones" for c in CASES if c.ep == "bilinear_up_bwd") == 7
    for ep in ("maxpool_nchw_fwd", "maxpool_nchw_bwd"):
        cs = [c for c in CASES if c.ep == ep]
        assert {c.k for c in cs} == {1, 2, 3, 4, 15}
        for k in (2, 3, 4, 15):
            assert any(c.k == k and (c.h % k or c.w % k) for c in cs) and any(c.k == k and not (c.h % k or c.w % k) for c in cs), (ep, k)
    for ep in ("nearest_up_fwd", "nearest_up_bwd"):
        cs = [c for c in CASES if c.ep == ep]
        assert {(c.k, c.h, c.w) for c in cs} == {(s, h, w) for s in (1, 2, 3, 4) for (h, w) in GC.NEAREST_HW} and {c.n for c in cs} == {1, 6}
    for ep in ("reflect_pad_fwd", "reflect_pad_bwd"):
        cs = [c for c in CASES if c.ep == ep]
        assert {(c.h, c.w) for c in cs} == {(1, 1), (2, 2), (3, 5), (6, 7)}
        for side in range(4):
            ext = lambda c: (c.w, c.w, c.h, c.h)[side] - 1
            assert any(c.pads[side] == ext(c) > 0 and not any(c.pads[j] for j in range(4) if j != side) for c in cs), (ep, side)
            assert any(c.pads[side] < 0 and not any(c.pads[j] for j in range(4) if j != side) for c in cs), (ep, side)
        assert any(c.pads == (c.w - 1, c.w - 1, c.h - 1, c.h - 1) and c.h > 1 for c in cs) and any(min(c.pads) < 0 < max(c.pads) for c in cs)
        assert any(c.pads == (0, 0, 0, 0) and (c.h, c.w) == (1, 1) for c in cs)
    odd = sum(c.offset for c in CASES) / len(CASES)
    assert 0.15 <= odd <= 0.35, odd
    assert all(GC.elements(c) <= 1_100_000 for c in CASES)


def test_planted_selections_are_in_the_stored_operands():
    for c in CASES:
        if c.ep == "relu_bwd" and c.h >= 255:
            y, g = GC.operands(c)["y"], GC.operands(c)["g"]
            assert ((y == 0) & np.signbit(y)).sum() >= 2 and ((y == 0) & ~np.signbit(y)).sum() >= 2
            assert (y == 2.0 ** -149).sum() >= 2 and (y == 2.0 ** -126).sum() >= 2 and np.float32(2.0 ** -149) > 0
            assert (np.abs(g[(y == 0) | (y == 2.0 ** -149) | (y == 2.0 ** -126)]) >= 0.5).all()          # each with a gradient that shows
            assert ((g == 0) & np.signbit(g)).sum() >= 1
        if c.ep == "maxpool_nchw_fwd":
            x = GC.operands(c)["x"]
            win = GC.pool_windows(x, c.k)
            assert np.array_equal(x[np.isfinite(x)], np.round(x[np.isfinite(x)])) and np.abs(x[np.isfinite(x)]).max() <= 3
            if c.k > 1:
                ties = (win == win.max(-1, keepdims=True)).sum(-1)
                assert (ties[np.isfinite(win).all(-1)] > 1).mean() > 0.2, c.id          # many windows hold their maximum more than once
                assert c.plant == "windows" and set(GC.maxpool_plants(c).values()) == {"all_neg_inf", "signed_zeros", "one_nan_not_first", "all_nan"}
                outs = {d.name: d.want for d in GC.define(c)}
                assert np.isneginf(win[0, 0, 0]).all() and np.isneginf(outs["y"][0, 0, 0]) and outs["idx"][0, 0, 0] == 0
                z = win[0, 0, 1]
                assert z[1] == 0 and np.signbit(z[1]) and z[-1] == 0 and not np.signbit(z[-1]) and (np.delete(z, [1, c.k * c.k - 1]) < 0).all()
                assert outs["idx"][0, 0, 1] == 1 and np.signbit(outs["y"][0, 0, 1])          # the first of the two zeros, with its sign
                assert np.isnan(win[0, 1, 0]).sum() == 1 and np.isnan(win[0, 1, 0][1]) and np.isnan(outs["y"][0, 1, 0]) and outs["idx"][0, 1, 0] == 1
                assert np.isnan(win[0, 1, 1]).all() and np.isnan(outs["y"][0, 1, 1]) and outs["idx"][0, 1, 1] == 0


# ------------------------------------------------------------------------------------------------------------------------------ bounds, mutations
def test_no_bound_is_vacuous_and_every_case_is_alive():
    loose = []
    for c in CASES:
        for o in GC.define(c):
            assert o.want.shape == np.shape(o.bound) and (np.asarray(o.bound) >= 0).all() and np.isfinite(o.bound).all(), (c.id, o.name)
            if o.exact is True:
                assert not np.asarray(o.bound).any()
                continue
            if not o.want.size:
                continue
            assert np.isfinite(o.want).all() and o.want.any(), (c.id, o.name)
            r = float(np.max(o.bound)) / float(np.abs(o.want).max())
            # a bound past 1e-3 of the output's scale must say why, and the reason it gives, the conditioning of the sum, must account for
            # all of the excess: what is left, the chain's (T + 1) u, stays below 1e-3 like everyone else's
            assert bool(o.why_loose) == (r > 1e-3), (c.id, o.name, r, o.why_loose)
            if o.why_loose:
                loose.append((c.id, o.name, r))
                assert o.cond > 1 and r / o.cond <= 1e-3, (c.id, o.name, r, o.cond)
    print(loose)
    assert len(loose) <= 0.02 * len(CASES), loose


def _caught(c, mut):
    true, wrong = GC.define(c), GC.define(c, mut)
    for t, m in zip(true, wrong):
        if t.want.shape != m.want.shape:
            return True          # another extent: the sweep sizes the output from the definition
        if t.want.size and GC.compare(t, m.want)[0].any():
            return True
    return False


@pytest.mark.parametrize("mut", list(GC.MUTATIONS))
def test_every_wrong_definition_leaves_the_bound_of_the_true_one(mut):
    eps, pred = GC.MUTATIONS[mut]
    for ep in eps:
        cases = [c for c in CASES if c.ep == ep and pred(c) and GC.elements(c) <= BIG]
        assert cases, f"{mut}: no {ep} case can show it"
        caught = [c.id for c in cases if _caught(c, mut)]
        print(f"{mut} on {ep}: caught by {len(caught)} of {len(cases)} cases")
        assert len(caught) >= max(1, len(cases) // 2), (mut, ep, len(caught), len(cases))
