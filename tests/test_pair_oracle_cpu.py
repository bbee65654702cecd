"""tests/pair_cases.py without a GPU: its fp64 definitions of the pair-conv kernels against torch's float64 autograd, the fold identities the
engine relies on, every case shown to tell the true definition from each plausible wrong one by more than ten times its own tolerance, and the
case table shown to hold every edge it claims."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pair_cases as PC
from pair_cases import CASES, Case


def _nerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _stack(a, b):
    return torch.stack([a, b], dim=2).reshape(-1, 2, a.shape[2], a.shape[3])


AUTOGRAD = [Case("bwd", "f32", 2, 1, 2, 2, 2, mask="all", add="h0", g="h0", relu=True, res="other"),
            Case("bwd", "f32", 2, 3, 3, 5, 1, mask="alt", add="folded", g="folded", relu=False, res="ops"),
            Case("bwd", "bf16", 1, 3, 17, 18, 2, mask="all", add="raw", g="raw", relu=True, res="ops", bias=False),
            Case("bwd", "f32", 1, 8, 6, 7, 2, mask="b67", add="raw", g="h0", relu=True, res="none")]


@pytest.mark.parametrize("c", AUTOGRAD, ids=lambda c: c.id)
def test_definitions_equal_torch_float64_autograd(c):
    """pairs stacked as [N*C, 2, H, W], F.pad(mode='reflect') + F.conv2d in float64: forward with ReLU / residual; the padded-domain gradient =
    the autograd gradient w.r.t. the explicitly padded (pre-activation) tensor, the folded one = w.r.t. the unpadded tensor; dw, db: 1e-12"""
    o = PC.operands(c)
    n, C = c.n, c.C
    w, bias = _t(o.w).requires_grad_(True), _t(o.bias).requires_grad_(True)
    gs = [PC.logical(g, c.g) for g in o.g]
    G = _stack(*[_t(g) for g in gs]) if c.nout == 2 else _t(gs[0]).reshape(-1, 1, c.h, c.w)
    add = PC.logical(o.add, c.add)
    mm = _t(PC.block_mask(c.mask_bits, C))

    # ---- forward, dw, db
    z = F.conv2d(F.pad(_stack(_t(o.a), _t(o.b)), (1, 1, 1, 1), mode="reflect"), w, bias)
    y = (z.clamp_min(0) if c.relu else z).reshape(n, C, c.nout, c.h, c.w)
    want = [y[:, :, i] for i in range(c.nout)]
    if c.res != "none":
        want[0] = want[0] + _t(o.r1) + _t(o.r2)
    outs, _ = PC.def_fwd(c)
    for got, ref in zip(outs, want):
        assert _nerr(got, ref.detach().numpy()) <= 1e-12
    (z * G).sum().backward()
    dw, db, _, _ = PC.def_wgrad(c, 0)
    assert _nerr(dw, w.grad.numpy()) <= 1e-12 and _nerr(db, bias.grad.numpy()) <= 1e-12
    dw1, db1, _, _ = PC.def_wgrad(c, 1)
    assert _nerr(dw1, w.grad.numpy() + o.dw_old) <= 1e-12 and _nerr(db1, bias.grad.numpy() + o.db_old) <= 1e-12

    # ---- gx: the operands are ReLU outputs of a pre-activation with the operands' signs; a masked block's gradient goes through that ReLU.
    # (the convolution's own gradient does not depend on the operand values, only the mask does)
    def through(pre):          # relu on the masked blocks, identity on the others
        return mm * pre.clamp_min(0) + (1 - mm) * pre
    # padded domain: leaves are the explicitly padded pre-activations
    pa = F.pad(_t(o.a), (1, 1, 1, 1), mode="reflect").requires_grad_(True)
    pb = F.pad(_t(o.b), (1, 1, 1, 1), mode="reflect").requires_grad_(True)
    xa, xb = through(pa), through(pb)
    loss = (F.conv2d(_stack(xa, xb), w.detach()) * G).sum() + (_t(PC.pad0(add)) * (xa + xb)).sum()
    loss.backward()
    (gxa, gxb), _ = PC.def_gx(c)
    assert _nerr(gxa, pa.grad.numpy()) <= 1e-12 and _nerr(gxb, pb.grad.numpy()) <= 1e-12
    # folded: leaves are the unpadded pre-activations
    ua, ub = _t(o.a).requires_grad_(True), _t(o.b).requires_grad_(True)
    xa, xb = through(ua), through(ub)
    loss = (F.conv2d(F.pad(_stack(xa, xb), (1, 1, 1, 1), mode="reflect"), w.detach()) * G).sum() + (_t(add) * (xa + xb)).sum()
    loss.backward()
    assert _nerr(PC.fold(gxa), ua.grad.numpy()) <= 1e-12 and _nerr(PC.fold(gxb), ub.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("c", AUTOGRAD, ids=lambda c: c.id)
def test_fold_identities(c):
    """fold(masked gxp) == mask * fold(gxp);  fold(gxp + pad0(add)) == fold(gxp) + add;  an unfolded g / add means its fold"""
    o = PC.operands(c)
    gs = [PC.logical(g, c.g) for g in o.g]
    add = PC.logical(o.add, c.add)
    plain = PC.gx_on(gs, o.w, o.a, o.b, 0, None)
    masked = PC.gx_on(gs, o.w, o.a, o.b, c.mask_bits, None)
    added = PC.gx_on(gs, o.w, o.a, o.b, 0, add)
    mm = PC.block_mask(c.mask_bits, c.C)
    for x, p, m, ad in zip((o.a, o.b), plain, masked, added):
        keep = 1 - mm + mm * (x > 0)
        assert float(np.abs(p[:, :, 0]).max()) > 0, "the ring of the padded-domain gradient is alive"
        assert _nerr(PC.fold(m), keep * PC.fold(p)) <= 1e-12
        assert _nerr(PC.fold(ad), PC.fold(p) + add) <= 1e-12
    # unfolded tensors: the definition on the stored halo-1 tensor equals the definition on a folded tensor holding its fold
    for kind, stored in (("g", o.g[0]), ("add", o.add)):
        if getattr(c, kind) != "raw":
            continue
        assert float(np.abs(stored[:, :, 0]).max()) > 0 and float(np.abs(stored[:, :, :, -1]).max()) > 0, "an unfolded tensor's ring is alive"
        refolded = PC.pad0(PC.fold(stored))
        assert np.array_equal(PC.logical(stored, "raw"), PC.logical(refolded, "folded"))
    if c.g == "raw":
        dw, db, _, _ = PC.def_wgrad(c)
        dw2, db2 = PC.wgrad_on(o.a, o.b, [PC.logical(PC.pad0(PC.fold(g)), "folded") for g in o.g])
        assert np.array_equal(dw, dw2) and np.array_equal(db, db2)
    if c.add == "raw":
        got, _ = PC.def_gx(c)
        want = PC.gx_on(gs, o.w, o.a, o.b, c.mask_bits, PC.logical(PC.pad0(PC.fold(o.add)), "folded"))
        assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))


def _outputs(c, mut=None):
    """[(name, value, bound)] of everything the case's call writes"""
    out = []
    if c.op == "fwd":
        ys, bs = PC.def_fwd(c, mut)
        out += [(k, y, b) for k, y, b in zip(("oa", "ob"), ys, bs)]
    if c.has_gx:
        ys, bs = PC.def_gx(c, mut)
        out += [(k, y, b) for k, y, b in zip(("gxa", "gxb"), ys, bs)]
    if c.has_dw:
        dw, db, bdw, bdb = PC.def_wgrad(c, 0, mut)
        out += [("dw", dw, bdw), ("db", db, bdb)]
    return out


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_case_is_discriminating(c):
    """on the case's own inputs every wrong definition that can show on it (taps transposed, w[o][0] / w[o][1] swapped, w[0] / w[1] swapped, zero
    for reflect padding, clamp for reflect in the ring's mask, `add` in the ring, residual before the activation) is further than ten times the
    case's tolerance from the true one, and the true one is alive: reverting any of them into the definitions fails the GPU sweep"""
    true = _outputs(c)
    for name, y, bound in true:
        assert float(np.abs(y).max()) > 0, f"{c.id}: {name} is all zero"
        assert np.all(bound >= 0) and np.all(np.isfinite(bound))
        if c.op == "fwd" and c.relu and c.res == "none":
            frac = float((y > 0).mean())
            assert 0.1 <= frac <= 0.9, f"{c.id}: {frac:.2f} of {name} is positive"
    if c.has_gx and c.mask_bits:
        o = PC.operands(c)
        frac = float((o.a > 0).mean())
        assert 0.2 <= frac <= 0.8
    muts = c.mutations()
    assert len(muts) >= 2
    for mut in muts:
        worst = 0.0
        for (name, y, bound), (_, ym, _) in zip(true, _outputs(c, mut)):
            d = np.abs(ym - y)
            worst = max(worst, float(np.max(d / np.maximum(bound, 1e-300) * (d > 0))))
        assert worst > 10, f"{c.id}: {mut} is only {worst:.2f} x the tolerance away from the true definition"


def test_the_table_covers_what_it_claims():
    for dtype in PC.DTYPES:
        cs = [c for c in CASES if c.dtype == dtype]
        # ---- tile edges of the 16 x 16 tiles: image domain (fwd, wgrad), stored domain (dgrad, bwd); every entry point, h and w
        for op in ("fwd", "wgrad", "dgrad", "bwd"):
            for v in PC.TILE_EDGES:
                for axis in (0, 1):
                    assert any(c.op == op and (c.h, c.w)[axis] == v for c in cs), (dtype, op, v, axis)
            # the edges really are edges: a plane one short of, exactly at and one past a tile in the domain the kernel tiles
            e = 2 if op in ("dgrad", "bwd") else 0
            for axis in (0, 1):
                ext = {(c.h, c.w)[axis] + e for c in cs if c.op == op}
                assert {PC.PT - 1, PC.PT, PC.PT + 1} | ({2 * PC.PT, 2 * PC.PT + 1} if e else {2 * PC.PT - 1}) <= ext, (dtype, op, axis, sorted(ext))
            assert any(c.op == op and c.h == 2 for c in cs) and any(c.op == op and c.w == 2 for c in cs)          # every row / column a reflect source
            assert any(c.op == op and c.h >= 4 * c.w and c.h > 64 for c in cs) and any(c.op == op and c.w >= 4 * c.h and c.w > 64 for c in cs)
            # ---- channel-block geometry
            assert {1, 3, 8} <= {c.cb for c in cs if c.op == op}
            assert any(c.op == op and c.pair for c in cs) and any(c.op == op and not c.pair for c in cs)
            assert {1, 2} <= {c.nout for c in cs if c.op == op}
            # ---- persistence: more tiles than persistent blocks (some blocks walk two tiles, others one) and fewer
            if op in ("wgrad", "bwd"):
                big = [c for c in cs if c.op == op and c.tiles > PC.PERSISTENT_BLOCKS]
                assert big and all(c.tiles < 2 * PC.PERSISTENT_BLOCKS and c.tiles_per_block == 2 for c in big)
                assert any(c.op == op and c.tiles < PC.PERSISTENT_BLOCKS and c.tiles_per_block == 1 for c in cs)
                assert all(set(c.accumulate) == {0, 1} for c in cs if c.op == op)
        # ---- the strip forward's 32 x 32 tiles and 4-wide strips, under both settings of the switch
        if dtype == "bf16":
            for strip in (1, 0):
                for v in PC.STRIP_EDGES:
                    assert any(c.op == "fwd" and c.strip == strip and c.w == v for c in cs), (strip, v)
                assert {PC.FT - 1, PC.FT, PC.FT + 1} <= {c.h for c in cs if c.op == "fwd" and c.strip == strip}
        # ---- forward variants: the full cross product at one shape; the LDS-window residual (operands) on the strip kernel
        for strip in ((1, 0) if dtype == "bf16" else (1,)):
            have = {(c.nout, c.relu, c.bias, c.res) for c in cs if c.op == "fwd" and c.strip == strip and c.note == "all"}
            assert have == set(PC.FWD_VARIANTS)
        # ---- gx variants
        have = {(c.nout, c.mask, c.add, c.g) for c in cs if c.op == "dgrad" and c.note == "all"}
        assert have == set(PC.GX_VARIANTS)
        have = {(c.nout, c.mask, c.add, c.g) for c in cs if c.op == "bwd" and c.note == "all"}
        assert have == {v for v in PC.GX_VARIANTS if v[2] != "raw"}
        assert not any(c.op == "bwd" and c.add == "raw" for c in cs), "mmif_pairconv_bwd refuses an unfolded add (tests/test_host_cpu.py)"
        assert any(c.op == "dgrad" and c.add == "raw" for c in cs), "mmif_pairconv_dgrad takes an unfolded halo-1 add"
        have = {(c.nout, c.g) for c in cs if c.op == "wgrad"}
        assert have == set(PC.WG_VARIANTS), "mmif_pairconv_wgrad with h0, folded and unfolded g"
        for op in ("dgrad", "bwd"):
            m8 = {c.mask for c in cs if c.op == op and c.cb == 8}
            assert {"none", "all", "b67", "alt"} <= m8, (op, m8)
        assert Case("dgrad", dtype, 1, 8, 4, 4, mask="b67").mask_bits == 0b11000000 and Case("dgrad", dtype, 1, 8, 4, 4, mask="alt").mask_bits == 0x5a
        assert Case("dgrad", dtype, 1, 3, 4, 4, mask="alt").mask_bits == 0b010 and Case("dgrad", dtype, 1, 3, 4, 4, mask="all").mask_bits == 0b111


def test_depth_of_the_weight_gradient_chains():
    """D at the two ends of the table, spelled out (see Case.wgrad_depth)"""
    small = Case("wgrad", "f32", 2, 1, 2, 2, 2, g="h0")                      # 2 tiles, 2 blocks
    assert small.tiles == 2 and small.wgrad_depth("dw") == 4 + 1 + 6 + 2 + 1 + 6 + 4 and small.wgrad_depth("db") == 3 + 1 + 6 + 2 + 1 + 6 + 4
    n, cb, h, w = PC.BIG
    big = Case("bwd", "bf16", n, cb, h, w, 2)
    assert big.tiles == 2080 and big.wgrad_depth("dw") == 16 + 0 + 6 + 2 + 8 + 6 + 4 == big.wgrad_depth("db")
    assert dataclasses.replace(big, dtype="f32").wgrad_depth("dw") == 8 + 1 + 6 + 2 + 8 + 6 + 4
    assert dataclasses.replace(small, g="raw").wgrad_depth("dw") == small.wgrad_depth("dw") + 3
