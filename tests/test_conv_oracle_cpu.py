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
    """at 256 compute units the library's dispatch gives each case's label for every bit pair it runs; every required name has a case.  An x3
    forward case runs in the three operand formats (tests/test_gpu_conv_sweep.py): it reaches the kernel of each"""
    wrong = [(c.id, m, a, c.expected(256, m, a)) for c in CASES for m, a in c.bits if c.expected(256, m, a) != c.label]
    assert not wrong, wrong[:10]
    reached = {c.label for c in CASES}
    for c in CASES:
        if c.impl == "x3" and c.op == "fwd":
            by_format = c.x3_forward_labels()
            assert by_format[16] == c.label and len(set(by_format.values())) == 3, (c.id, by_format)
            reached |= set(by_format.values())
    missing = [l for l in CC.REQUIRED_LABELS if l not in reached]
    print("unreached kernels:", missing)
    assert not missing, missing
    assert len(set(CC.REQUIRED_LABELS)) == len(CC.REQUIRED_LABELS) and not reached & CC.UNREACHABLE
    assert all(len(l) < 32 for l in CC.REQUIRED_LABELS + sorted(CC.UNREACHABLE)), "mmif_route.name is char[32]"


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


# ------------------------------------------------------------------------------------------------------------------------------
# the fp32 split-operand (x3) routes on a grid of geometries: what the launches take from csrc/conv_route.hpp, asked through
# mmif_conv2d_route and mmif_conv2d_wgrad_workspace
# ------------------------------------------------------------------------------------------------------------------------------
X3_CH = (1, 8, 13, 16, 17, 32, 33, 48, 49, 64, 65, 72, 128, 136)
X3_MAPS = [(2, 33, 40), (1, 16, 16), (2, 17, 17), (2, 2, 9), (1, 3, 3), (2, 5, 7), (1, 512, 512)]
X3_CUS = (8, 64, 256, 304)
XT_PER = 9 * 768 + 64                  # floats of one wgrad_x3_thin_kernel partial (csrc/wgrad_reduce.hpp)


def _xw_per(cin, cout, k):
    """floats of one wgrad_x3_kernel tile group: a [64 x 64 x taps | 64] partial per 64 x 64 channel pair (wgrad_x3_reduce::per)"""
    return CC.cdiv(cin, 64) * CC.cdiv(cout, 64) * (64 * 64 * k * k + 64)


def _x3_formats(fn):
    from mmif._lib import lib
    prev = lib.mmif_get_x3_forward_pieces()
    try:
        for pieces in CC.X3_FORMATS:
            lib.mmif_set_x3_forward_pieces(pieces)
            fn(pieces)
    finally:
        lib.mmif_set_x3_forward_pieces(prev)


def test_x3_forward_and_dgrad_routes_on_a_grid():
    """every legal call is taken; the name says the operation, the kernel size, the operand format and the M-block width asked for, and the
    tile geometry it names (32 columns x 16 rows; nw4: 8 rows, three blocks per compute unit; rj4: 32 rows) is the one the grid is sized by:
    1 <= G = min(tiles, blocks per CU x compute units); org = 1 exactly for the folded 3x3 call at h, w >= 4 off the m16 kernel"""
    seen = {}

    def check(pieces):
        fmt = {16: "h16", 3: "b3", 2: "b2"}[pieces]
        for k in (1, 3):
            for (n, h, w) in X3_MAPS:
                for cin in X3_CH:
                    for cout in X3_CH:
                        for ncu in X3_CUS:
                            calls = [("fwd", False, cout)] + ([("dgrad", f, cin) for f in (False, True)] if pieces == 16 else [])
                            for op, fold, n_out in calls:
                                r = CC.route(op, "f32", cin, cout, n, h, w, fold=fold, k=k, impl="x3", num_cus=ncu)
                                what = (op, fold, k, cin, cout, n, h, w, ncu, r)
                                assert r is not None and r.name in CC.X3_LABELS, what
                                head, _, args = r.name[:-1].partition("<")
                                args = args.split(",")
                                assert head == ("x3" if op == "fwd" else "x3_dgrad") and args[0] == str(k) and args[1] == f"mb{2 if n_out > 32 else 1}", what
                                assert (args[2] == fmt) if op == "fwd" else not {"h16", "b3", "b2"} & set(args), what
                                rows, per_cu = (8, 3) if "nw4" in args else ((32, 1) if "rj4" in args else (16, 1))
                                halo = 1 if op == "dgrad" else 0          # (the tiles cover gx's stored extent; these gx have a halo of 1)
                                assert r.org == (1 if (fold and k == 3 and h >= 4 and w >= 4 and "m16" not in args) else 0), what
                                ext = 2 * (halo - r.org)
                                assert r.tiles == n * CC.cdiv(h + ext, rows) * CC.cdiv(w + ext, 32), what
                                assert 1 <= r.G == min(r.tiles, per_cu * ncu) and r.slices == 0, what
                                seen.setdefault(r.name, set()).add((op, k, n_out > 32, pieces if op == "fwd" else 0))
    _x3_formats(check)
    assert all(len(v) == 1 for v in seen.values()), "one name, one (operation, kernel size, M-block width, format)"
    assert set(seen) == {l for l in CC.X3_LABELS if "wgrad" not in l}, "the grid reaches every forward / input-gradient kernel and no other name"


def test_x3_weight_gradient_routes_fit_the_workspace_on_a_grid():
    """1 <= G <= tiles per launched tile group (the 1x1 kernel leaves three k-split partials per block: the reduce's G is three times that), and the
    partials the reduce sums fit the workspace mmif_conv2d_wgrad_workspace answers for the layer, whatever the compute units -- the
    property the thin launcher used to guard at run time.  The <16,6,2,3> fallback is taken by no call up to 256 compute units; it is
    what keeps the property at 304, where five thin blocks per CU would outgrow the workspace."""
    from mmif import tensor as T
    seen = {}
    for k in (1, 3):
        for cin in X3_CH:
            for cout in X3_CH:
                ws = T.wgrad_workspace_bytes(cin, cout, k)
                for (n, h, w) in X3_MAPS:
                    for ncu in X3_CUS:
                        r = CC.route("wgrad", "f32", cin, cout, n, h, w, k=k, impl="x3", num_cus=ncu)
                        what = (k, cin, cout, n, h, w, ncu, r)
                        assert r is not None and r.name in set(CC.X3_LABELS) | CC.UNREACHABLE, what
                        thin = r.name.startswith("x3_wgrad_thin<")
                        assert thin == (k == 3 and cin <= 48 and cout <= 16 and r.name != "x3_wgrad_thin16"), what
                        th = 16 if r.name == "x3_wgrad_thin16" else 8
                        assert r.tiles == n * CC.cdiv(h, th) * CC.cdiv(w, 16), what
                        split = 3 if k == 1 else 1
                        assert r.G % split == 0 and 1 <= r.G // split <= r.tiles, what
                        assert r.slices == (16 if (thin or r.G > 64) else 4), what
                        assert r.G * (XT_PER if thin else _xw_per(cin, cout, k)) * 4 <= ws, what
                        assert r.name != "x3_wgrad_thin16" or ncu > 256, what
                        seen.setdefault(r.name, set()).add((k, 2 if cin <= 16 else (4 if cin <= 32 else 6)) if thin else (k,))
    assert all(len(v) == 1 for v in seen.values()), "one name, one kernel"
    assert set(seen) == {l for l in CC.X3_LABELS if "wgrad" in l} | CC.UNREACHABLE
    assert CC.expected_kernel("wgrad", "f32", 16, 16, 1, 512, 512, impl="x3", num_cus=304) == "x3_wgrad_thin16"      # 1520 blocks x 6976 floats
    for ncu in range(1, 257):           # ... and nowhere on a real part: every thin layer class, more tiles than any grid
        for cin in (16, 32, 48):
            assert CC.expected_kernel("wgrad", "f32", cin, 16, 4, 512, 512, impl="x3", num_cus=ncu) == f"x3_wgrad_thin<{cin // 8}>"


def test_x3_bwd_wide_reports_both_halves():
    """name, tiles and org of the input-gradient half, G and slices of the weight-gradient half"""
    for cin, cout, k in [(72, 64, 3), (13, 21, 3), (16, 16, 3), (88, 64, 1)]:
        for (n, h, w) in X3_MAPS:
            r = CC.route("bwd_wide", "f32", cin, cout, n, h, w, k=k, impl="x3")
            d = CC.route("dgrad", "f32", cin, cout, n, h, w, k=k, fold=True, impl="x3")
            g = CC.route("wgrad", "f32", cin, cout, n, h, w, k=k, impl="x3")
            assert (r.name, r.tiles, r.org, r.G, r.slices) == (d.name, d.tiles, d.org, g.G, g.slices), (cin, cout, k, n, h, w, r, d, g)


def test_a_refused_x3_call_has_an_empty_route():
    from mmif import _lib as L

    def ask(op, cin, cout, n, h, w, k=3, dtype=L.F32, gy_halo=1, gy_flags=L.T_FOLDED, impl=L.IMPL_X3):
        def t(c, halo, flags=0):
            return L.MmifTensor(None, dtype, n, h, w, halo, CC.cdiv(c, 8), 0, CC.cdiv(c, 8), flags)
        a, b = {"fwd": (t(cin, 0), t(cout, 0)), "dgrad": (t(cout, gy_halo, gy_flags), t(cin, 1))}.get(op, (t(cin, 0), t(cout, gy_halo, gy_flags)))
        r = L.MmifRoute()
        r.name, r.G, r.slices, r.tiles, r.org = b"stale", 7, 7, 7, 7
        taken = L.lib.mmif_conv2d_route(L.ROUTE_OPS[op], a, b, cin, cout, k, 0, 0, 0, impl, 256, r)
        return taken, (r.name, r.G, r.slices, r.tiles, r.org)

    assert ask("fwd", 16, 16, 1, 16, 16)[0] == 1 and ask("dgrad", 16, 16, 1, 16, 16)[0] == 1 and ask("wgrad", 16, 16, 1, 16, 16)[0] == 1
    assert ask("fwd", 16, 16, 1, 4096, 4095)[0] == 1, "the last plane eight of which 32-bit byte offsets address"
    refused = [ask("fwd", 16, 16, 1, 16, 16, dtype=L.BF16),                     # the x3 kernels take fp32 tensors
               ask("fwd", 16, 16, 1, 1, 16), ask("wgrad", 16, 16, 1, 16, 1),    # reflect padding needs h, w >= 2
               ask("fwd", 16, 520, 1, 16, 16), ask("dgrad", 520, 16, 1, 16, 16),        # mask / accumulate bits address 64 channel blocks
               ask("bwd_wide", 520, 16, 1, 16, 16),
               ask("dgrad", 16, 16, 1, 16, 16, gy_flags=0), ask("wgrad", 16, 16, 1, 16, 16, gy_flags=0),   # a padded-domain gradient
               ask("bwd_wide", 16, 16, 1, 16, 16, gy_flags=0),
               ask("fwd", 16, 16, 1, 4096, 4096), ask("wgrad", 16, 16, 1, 4096, 4096)]
    assert all(r == (0, (b"", 0, 0, 0, 0)) for r in refused), refused
