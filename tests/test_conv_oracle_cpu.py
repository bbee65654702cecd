"""tests/conv_cases.py without a GPU: its fp64 definitions against torch's float64 autograd and golden F3, its case list against the
library's dispatch (mmif_conv2d_route on descriptors without data: every kernel name reached, the thresholds between kernels), and the
non-vacuity of every case's reference."""
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC
from conv_cases import CASES
from gpu_util import G, close
from oracle import fusion_oracle as O
from test_oracle_golden import F3_CASES, f3_tensors


def _small(c):
    """N = 1 on the big maps: the definition's batch handling is covered by the small ones"""
    return dataclasses.replace(c, n=1) if c.h * c.w > 4096 else c


def _classes():
    seen, out = set(), []
    for c in CASES:
        key = (c.cin, c.cout, c.k, c.h, c.w)
        if key not in seen:
            seen.add(key)
            out.append(_small(dataclasses.replace(c, dtype="f32", op="dgrad", fold=True, gy_folded=True, gy_halo=1, gx_halo=1, switches=(), slot=(0, 0),
                                                  note="", label="")))
    return out


def _nerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("c", _classes(), ids=lambda c: f"{c.cin}to{c.cout}k{c.k}-{c.n}x{c.h}x{c.w}")
def test_definitions_equal_torch_float64_autograd(c):
    """forward, padded-domain and folded input gradient (with mask / accumulate as (gx_old + gx) * mask), dw and db against
    F.conv2d(F.pad(x, mode='reflect'), w, b) in float64: 1e-12, max-normalised"""
    o = CC.operands(c)
    p = c.k // 2
    x = torch.from_numpy(o.x).requires_grad_(True)
    w = torch.from_numpy(o.w).requires_grad_(True)
    b = torch.from_numpy(o.b).requires_grad_(True)
    xp = (F.pad(x, (p, p, p, p), mode="reflect") if p else x * 1.0)
    xp.retain_grad()
    z = F.conv2d(xp, w, b)
    z.backward(torch.from_numpy(o.g))
    for relu in (True, False):
        y = CC.def_fwd(dataclasses.replace(c, op="fwd", relu=relu))[0]
        assert _nerr(y, (z.clamp_min(0) if relu else z).detach().numpy()) <= 1e-12
    gxp = CC.def_dgrad_padded(c)[0]
    assert _nerr(gxp, xp.grad.numpy()) <= 1e-12
    dw, db = CC.def_wgrad(c, 0)
    assert _nerr(dw, w.grad.numpy()) <= 1e-12 and _nerr(db, b.grad.numpy()) <= 1e-12
    dw1, db1 = CC.def_wgrad(c, 1)
    assert _nerr(dw1, (w.grad + torch.from_numpy(o.dw_old)).numpy()) <= 1e-12 and _nerr(db1, (b.grad + torch.from_numpy(o.db_old)).numpy()) <= 1e-12
    pos = (x.detach() > 0).double()
    old = torch.from_numpy(o.old)
    for mb, ab in CC.FEW_BITS + ((0, CC.ALL),):
        mm = torch.from_numpy(CC.block_mask(mb, c.cin))[None, :, None, None]
        am = torch.from_numpy(CC.block_mask(ab, c.cin))[None, :, None, None]
        keep = 1 - mm + mm * pos
        if p:
            want = torch.zeros_like(old)
            want[:, :, 1:-1, 1:-1] = (x.grad + am * old[:, :, 1:-1, 1:-1]) * keep
            got = CC.def_dgrad(c, mb, ab)[0]
            assert _nerr(got, want.numpy()) <= 1e-12, "folded"
            keep_p = F.pad(keep.expand_as(pos), (1, 1, 1, 1), mode="reflect")
            want = (xp.grad + am * old) * keep_p
            got = CC.def_dgrad(dataclasses.replace(c, fold=False), mb, ab)[0]
            assert _nerr(got, want.numpy()) <= 1e-12, "padded"
        else:
            c0 = dataclasses.replace(c, fold=False, gy_halo=0, gx_halo=0)
            o0 = CC.operands(c0)
            x0 = torch.from_numpy(o0.x).requires_grad_(True)
            F.conv2d(x0, torch.from_numpy(o0.w)).backward(torch.from_numpy(o0.g))
            keep0 = 1 - mm + mm * (x0.detach() > 0).double()
            want = (x0.grad + am * torch.from_numpy(o0.old)) * keep0
            assert _nerr(CC.def_dgrad(c0, mb, ab)[0], want.numpy()) <= 1e-12, "1x1"


def test_padded_gradient_of_an_unfolded_gy_is_that_of_its_fold():
    """gy_folded=False cases hand the kernel a padded-domain gy; the definition's g is its fold (the kernel folds while loading)"""
    c = next(c for c in CASES if not c.gy_folded)
    o = CC.operands(c)
    assert float(np.abs(o.gp[:, :, 0]).max()) > 0
    assert _nerr(o.g, CC.rnd(O.reflect_pad_adjoint(o.gp, 1), c.dtype)) == 0     # (stored once in the tensor's format before it is multiplied)


@pytest.mark.parametrize("case", [c for c in F3_CASES if c[1] > 1 and c[2] > 1], ids=lambda c: c[0])
def test_definitions_equal_golden_f3(case):
    """the float64 definitions on golden F3's operands, at the bar test_f3_conv_layer holds (2e-5)"""
    ref = {**np.load(os.path.join(G, "f3_conv.npz")), **np.load(os.path.join(G, "f3_conv_2.npz"))}
    name, cin, cout, k, relu, N, H, W = case
    x, w, b, gy = (a.astype(np.float64) for a in f3_tensors(case))
    y = O.conv2d_reflect_fwd(x, w, b, relu)
    close(y, ref[name + "_y"], 2e-5, "y")
    g = gy * (y > 0) if relu else gy
    gx = O.reflect_pad_adjoint(O.conv2d_reflect_dgrad_padded(g, w), k // 2)
    close(gx, ref[name + "_dx"], 2e-5, "dx")
    gx2, gw, gb = O.conv2d_reflect_bwd(x, w, y, gy, relu)
    assert np.array_equal(gx, gx2), "the padded-domain scatter folded is conv2d_reflect_bwd's gx, bit for bit"
    close(gw, ref[name + "_dw"], 2e-5, "dw")
    close(gb, ref[name + "_db"], 2e-5, "db")


def test_every_case_reaches_its_kernel_and_every_kernel_is_reached():
    """at 256 compute units the library's dispatch gives each case's label for every bit pair it runs; every required name has a case"""
    wrong = [(c.id, m, a, c.expected(256, m, a)) for c in CASES for m, a in c.bits if c.expected(256, m, a) != c.label]
    assert not wrong, wrong[:10]
    reached = {c.label for c in CASES}
    missing = [l for l in CC.REQUIRED_LABELS if l not in reached]
    print("unreached kernels:", missing)
    assert not missing, missing


def test_tile_thresholds_of_the_asynchronous_kernel():
    """512 tiles of 16x16 take thin_conv_async_kernel on a 256-CU part, 511 do not; fewer compute units lower the threshold"""
    ek = CC.expected_kernel
    assert ek("fwd", "bf16", 40, 24, 8, 128, 128) == "thin_async<2>" and ek("fwd", "bf16", 40, 24, 73, 16, 112) == "mfma<3,2>"
    assert ek("dgrad", "bf16", 16, 16, 3, 180, 200, fold=True) == "mfma<3,1>" and ek("dgrad", "bf16", 16, 16, 3, 208, 224, fold=True) == "thin_async<1>"
    assert ek("dgrad", "bf16", 16, 16, 3, 180, 200, fold=True, num_cus=128) == "thin_async<1>"
    assert ek("fwd", "bf16", 16, 48, 3, 178, 190) == "mfma<3,3>" and ek("fwd", "bf16", 16, 48, 3, 208, 224) == "thin_async<3>"
    assert ek("fwd", "bf16", 16, 16, 3, 208, 224) == "mfma<3,1>", "16 outputs forward stays on the register-staged kernel"


@pytest.mark.parametrize("cin,cout,k,h,w,fast,slow", [
    (8, 64, 3, 4096, 8191, "conv_dma<L0,org0>", "mfma<3,4>"),            # plane * 16 * CHUNK_CB: 2^25 granules per plane is the first too many
    (40, 24, 3, 2, 11184810, "thin_async<2>", "mfma<3,2>"),              # plane * 16 * TN_MAXCB: 22 369 621 is the last plane that fits
    (64, 32, 3, 2048, 8191, "thin_wide", "mfma<3,2>"),                   # plane * 16 * TNW_MAXCB: 2^24
    (8, 64, 1, 8192, 16383, "conv1x1_stream", "mfma<1,4>"),              # the 1x1 kernel's plane * 16: 2^27
], ids=["conv_dma", "thin_async", "thin_wide", "conv1x1_stream"])
def test_32_bit_plane_limits_of_the_fast_kernels(cin, cout, k, h, w, fast, slow):
    """a forward whose input plane is the last that keeps the kernel's 32-bit byte offsets takes the fast kernel; one more column of
    pixels (the first plane at or past the limit) falls back to the register-staged kernel.  Geometry only: no memory behind it."""
    per_plane = {"conv_dma<L0,org0>": 16 * 4, "thin_async<2>": 16 * 6, "thin_wide": 16 * 8, "conv1x1_stream": 16}[fast]
    assert h * w * per_plane < (1 << 31) <= h * (w + 1) * per_plane
    assert CC.expected_kernel("fwd", "bf16", cin, cout, 1, h, w, k=k) == fast
    assert CC.expected_kernel("fwd", "bf16", cin, cout, 1, h, w + 1, k=k) == slow


@pytest.mark.parametrize("num_cus", [8, 256])
def test_two_tiles_per_persistent_block_is_the_threshold(num_cus):
    """the asynchronous kernels (both geometries) want 2 G tiles, G = the compute units rounded down to a multiple of 8: 2 G - 1 tiles stay
    on the register-staged kernel, 2 G and 2 G + 1 leave it"""
    G = num_cus // 8 * 8
    for cin, cout, fast in ((40, 24, "thin_async<2>"), (64, 32, "thin_wide")):
        got = [CC.route("fwd", "bf16", cin, cout, n, 16, 16, num_cus=num_cus) for n in (2 * G - 1, 2 * G, 2 * G + 1)]
        assert [r.name for r in got] == ["mfma<3,2>", fast, fast], (num_cus, cin, cout, got)
        assert [r.tiles for r in got] == [2 * G - 1, 2 * G, 2 * G + 1] and [r.G for r in got] == [2 * G - 1, G, G]


@pytest.mark.parametrize("c", [_small(c) for c in CASES], ids=lambda c: c.id)
def test_case_is_not_vacuous(c):
    """non-zero reference; 20-80 % of a masked block's pixels pass; old values of the order of the new ones"""
    o = CC.operands(c)
    if c.op == "fwd":
        y = CC.def_fwd(c)[0]
        O.assert_alive(y, c.id, 0.2, 0.8) if c.relu else O.assert_alive(y, c.id)
        return
    if c.op in ("wgrad", "bwd_pair", "bwd_wide"):
        dw, db = CC.def_wgrad(c, 0)
        O.assert_alive(dw, c.id), O.assert_alive(db, c.id)
        r = np.abs(o.dw_old).mean() / np.abs(dw).mean()
        assert 0.1 <= r <= 10, f"{c.id}: |dw_old| / |dw| = {r}"
        if c.op == "wgrad":
            return
    new = CC.def_dgrad(c, 0, 0)[0]
    O.assert_alive(new, c.id)
    inner = (slice(None), slice(None), slice(c.gx_halo, c.gx_halo + c.h), slice(c.gx_halo, c.gx_halo + c.w))
    for m, a in c.bits:
        for blk in range(CC.cdiv(c.cin, 8)):
            ch = slice(8 * blk, min(8 * blk + 8, c.cin))
            if (m >> blk) & 1:
                frac = float((o.x[:, ch] > 0).mean())
                assert 0.2 <= frac <= 0.8, f"{c.id}: block {blk}: {frac:.2f} of the mask passes"
            if (a >> blk) & 1:
                r = np.abs(o.old[inner][:, ch]).mean() / np.abs(new[inner][:, ch]).mean()
                assert 0.1 <= r <= 10, f"{c.id}: block {blk}: |old| / |new| = {r}"
