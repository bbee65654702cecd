"""Every kernel path of the generic 3x3 / 1x1 ConvLayer against its fp64 definition (tests/conv_cases.py), element-wise, with derived bounds.

Each case first proves where it goes: the library's own dispatch, asked through mmif_conv2d_route for the device's compute-unit count
(conv_cases.route), must give the case's label (a mismatch fails, it never skips).  Outputs are pre-filled with a sentinel; nothing outside the written view
may change (neighbouring channel blocks of a wider buffer, the zero ring of a folded gradient).

Bounds.  bf16 outputs, per element (conv_cases.bf16_bound):  |got - ref| <= 2^-8 A + (K + 2) 2^-24 S.
  A = sum of the magnitudes of the values the path stores in bf16 on the way to the element (one rounding each):
    * forward, padded-domain dgrad, fused-fold dgrad (conv_dma / thin_async with org 1, bwd_pair, bwd_wide, dgrad_dup): the fp32 accumulator
      (+ bias / old value, mask applied) is rounded ONCE when stored:                                 r = 1, A = |ref|
    * folded call on a kernel that writes the padded domain, then the stand-alone fold kernel: every padded-domain value is stored in bf16
      (r = 1 each), the fold sums up to four of them in fp32 and stores the sum (one more):           A = fold(|padded values|) + |ref|
    * the masked copies of dgrad_dup are bit-copies of the rounded output:                            r = 1, A = |ref|
  S = the same convolution on |operands| (+ |b| or |old|), K = products accumulated in fp32 (bf16 x bf16 products are exact in fp32).
fp32 tensors and dw / db: the bars the suite already holds against fp64, max-normalised: 1e-4 (test_conv_fp32_vs_golden,
test_ragged_channel_groups_on_equals_off); x3 forward 3 * max(err of the fp32 FMA kernel, 2e-7) and x3 backward (two bf16 pieces) 2e-5
(test_x3_forward_vs_fp64_definition); dw additionally per tap plane (u, v), normalised by that plane's own maximum.
"""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import conv_cases as CC
from conv_cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 3.0            # bf16-exact sentinel of everything a call must not touch
RATIOS = {}           # family -> [max err / bound, max err, count]: printed by the last test
DERIVED = set()       # families held to the derived bf16 bound (the others: bars the suite already holds)


def _td(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _bt(a, c, h, w, halo, tdtype, slot=(0, 0), fill=SENT, flags=0):
    """blocked device tensor holding a [n, c, h+2*halo, w+2*halo] array in channel blocks slot[0].. of a buffer with slot[0] / slot[1] further
    blocks before / after (filled with `fill`, as are the pad channels of a ragged last block when a is None); returns (view, whole)"""
    from mmif import tensor as T
    n, cb = (a.shape[0] if a is not None else None), CC.cdiv(c, 8)
    cbt = slot[0] + cb + slot[1]
    hs, ws = h + 2 * halo, w + 2 * halo
    full = np.full((n, cbt * 8, hs, ws), fill, np.float32)
    full[:, slot[0] * 8:(slot[0] + cb) * 8] = 0.0
    full[:, slot[0] * 8:slot[0] * 8 + c] = a
    buf = torch.from_numpy(np.ascontiguousarray(full.reshape(n, cbt, 8, hs, ws).transpose(0, 1, 3, 4, 2))).to(tdtype).to(DEV)
    whole = T.BT(buf, n, h, w, halo, cbt, 0, cbt, T._CODE[tdtype], flags)
    view = T.BT(buf, n, h, w, halo, cbt, slot[0], cb, T._CODE[tdtype], flags)
    return view, whole


def _np(whole):
    b = whole.buf.float().cpu().numpy()
    n, cbt, hs, ws, _ = b.shape
    return b.transpose(0, 1, 4, 2, 3).reshape(n, cbt * 8, hs, ws).astype(np.float64)


def _split(whole, c, slot):
    """(the view's real channels, everything outside the view)"""
    a = _np(whole)
    lo, hi = slot[0] * 8, (slot[0] + CC.cdiv(c, 8)) * 8
    return a[:, lo:lo + c], np.concatenate((a[:, :lo], a[:, hi:]), axis=1)


def _record(family, err, bound):
    r = float((err / np.maximum(bound, 1e-300)).max()) if np.ndim(bound) else float(err / bound)
    e = RATIOS.setdefault(family, [0.0, 0.0, 0])
    e[0], e[1], e[2] = max(e[0], r), max(e[1], float(np.max(err))), e[2] + 1
    return r


def _check_bf16(c, family, got, ref, A, S, what):
    err = np.abs(got - ref)
    bound = CC.bf16_bound(c, A, S)
    bad = err > bound
    r = _record(family, err, bound)
    DERIVED.add(family)
    print(f"{c.id} {what}: max err {err.max():.3e}, max err / bound {r:.3f}")
    assert not bad.any(), f"{c.id} {what}: {int(bad.sum())} elements beyond the bound, worst err/bound {r:.3f} at {np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)}"


def _check_norm(c, family, got, ref, bar, what):
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    _record(family, e, bar)
    print(f"{c.id} {what}: max err / max|ref| {e:.3e} (bar {bar:.1e})")
    assert e <= bar, f"{c.id} {what}: {e:.3e} > {bar:.1e}"


def _check_dw(c, family, dw, db, accumulate, bar):
    dw_ref, db_ref = CC.def_wgrad(c, accumulate)
    _check_norm(c, family, dw, dw_ref, bar, f"dw acc={accumulate}")
    _check_norm(c, family, db, db_ref, bar, f"db acc={accumulate}")
    for u in range(c.k):
        for v in range(c.k):
            _check_norm(c, family + " tap", dw[:, :, u, v], dw_ref[:, :, u, v], bar, f"dw[{u}][{v}] acc={accumulate}")


_switches = CC.switches


def _setup(c):
    from mmif import tensor as T
    from mmif import _lib as L
    o = CC.operands(c)
    wt = torch.from_numpy(o.w32).to(DEV)
    pk = T.PackedWeights(c.cout, c.cin, c.k, DEV, L.BF16 if c.dtype == "bf16" else L.F32)
    pk.pack(wt)
    impl = {"mfma": L.IMPL_MFMA, "x3": L.IMPL_X3, "valu": L.IMPL_VALU}[c.impl]
    return o, wt, pk, impl


def _family(c):
    return f"{c.label} {c.op}{' folded' if c.fold else ''}"


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_route(c, m=None, a=None):
    ncu = _num_cus()
    got = c.expected(0, m, a)          # 0: the compute units the library's launches count
    assert got == c.label, f"{c.id}: meant for {c.label}, but with {ncu} compute units the dispatch takes {got}"


def _onto_route(c, m, a):
    """the accumulate-onto form of the case's call is taken (by the thin asynchronous kernel, folding in its tiles), switches at their defaults"""
    r = dataclasses.replace(c, op="dgrad_onto", switches=()).route(0, m, a)
    return r is not None and r.name.startswith("thin_async") and r.org == 1


def _fp32_bar(c):
    return 1e-4 if c.impl == "valu" else 2e-5          # x3 backward kernels: two bf16 pieces per operand


# ------------------------------------------------------------------------------------------------------------------------------ forward
FWD = [c for c in CASES if c.op == "fwd"]


@pytest.mark.parametrize("c", FWD, ids=lambda c: c.id)
def test_forward_equals_definition(c):
    """x3: in each operand format of its forward kernels (two scaled fp16 pieces, three / two bf16 pieces)"""
    from mmif import engine as E
    from mmif import tensor as T
    from mmif import _lib as L
    _assert_route(c)
    o, wt, pk, impl = _setup(c)
    b = torch.from_numpy(o.b.astype(np.float32)).to(DEV)
    x, _ = _bt(o.x, c.cin, c.h, c.w, 0, _td(c), fill=0.0)
    ref, S = CC.def_fwd(c)
    prev = L.lib.mmif_get_x3_forward_pieces()
    try:
        for pieces in ((16, 3, 2) if c.impl == "x3" else (None,)):
            if pieces is not None:      # process wide, read when the operand image is packed
                E.set_x3_forward_pieces(pieces)
                pk.pack(wt)
            y, ywhole = _bt(np.full((c.n, c.cout, c.h, c.w), SENT), c.cout, c.h, c.w, 0, _td(c), c.slot)
            with _switches(c.sw):
                T.conv_fwd(x, wt, b, y, c.cin, c.cout, c.k, c.relu, pk, impl)
                if c.impl == "x3":      # the bar of test_x3_forward_vs_fp64_definition is relative to the fp32 FMA kernel on the same case
                    yv, yvwhole = _bt(np.full((c.n, c.cout, c.h, c.w), SENT), c.cout, c.h, c.w, 0, _td(c))
                    T.conv_fwd(x, wt, b, yv, c.cin, c.cout, c.k, c.relu, pk, L.IMPL_VALU)
                torch.cuda.synchronize()
            got, outside = _split(ywhole, c.cout, c.slot)
            assert outside.size == 0 or bool((outside == SENT).all()), f"{c.id}: channel blocks next to the output slot were written"
            if c.dtype == "bf16":
                _check_bf16(c, _family(c), got, ref, np.abs(ref), S, "y")       # r = 1: the output rounding
            elif c.impl == "valu":
                _check_norm(c, _family(c), got, ref, 1e-4, "y")
            else:
                ev = float(np.abs(_split(yvwhole, c.cout, (0, 0))[0] - ref).max() / np.abs(ref).max())
                _check_norm(c, f"{_family(c)} pieces={pieces}", got, ref, 2e-5 if pieces == 2 else 3 * max(ev, 2e-7), f"y pieces={pieces}")
    finally:
        E.set_x3_forward_pieces(prev)


# ------------------------------------------------------------------------------------------------------------------------------ dgrad
DGRAD = [c for c in CASES if c.op in ("dgrad", "dgrad_onto")]


def _fused(c):
    """the kernel folds the reflect halo itself (interior tiles + fold steps): one output rounding"""
    return c.fold and c.h >= 4 and c.w >= 4 and (c.label.startswith("conv_dma") or c.label.startswith("thin_async"))


@pytest.mark.parametrize("c", DGRAD, ids=lambda c: c.id)
def test_input_gradient_equals_definition(c):
    from mmif import tensor as T
    from mmif import _lib as L
    o, wt, pk, impl = _setup(c)
    cbm = (1 << CC.cdiv(c.cin, 8)) - 1
    flags = L.T_FOLDED if (c.gy_halo and c.gy_folded) else 0
    gy, _ = _bt(o.gp, c.cout, c.h, c.w, c.gy_halo, _td(c), fill=0.0, flags=flags)
    x, _ = _bt(o.x, c.cin, c.h, c.w, 0, _td(c), fill=0.0)
    hx = c.gx_halo
    slot = (1, 1)
    old = CC.ring_zero(o.old) if (c.fold and hx) else o.old
    for m, a in c.bits:
        m, a = m & cbm, a & cbm
        _assert_route(c, m, a)
        gx, gxwhole = _bt(old, c.cin, c.h, c.w, hx, _td(c), slot)
        onto = c.op == "dgrad_onto"
        if onto:
            gold, goldwhole = gx, gxwhole
            fresh = CC.ring_zero(np.full(old.shape, 5.0))        # the previous contents of gx itself must not enter
            gx, gxwhole = _bt(fresh, c.cin, c.h, c.w, hx, _td(c), slot)
            assert T.dgrad_onto_supported(gy, gx, c.cin, c.cout, c.k), f"{c.id}: the library declines the accumulate-onto form here"
            assert _onto_route(c, m, a), f"{c.id}: dgrad_onto_supported disagrees with the route query"
        elif c.label.startswith("thin_async") and c.fold:
            assert T.dgrad_onto_supported(gy, gx, c.cin, c.cout, c.k) and _onto_route(c, m, a), f"{c.id}: dgrad_onto_supported disagrees with the route query"
        elif c.label.startswith("mfma<3") and c.fold and c.dtype == "bf16" and not c.sw and c.gy_folded and c.gy_halo:
            assert not T.dgrad_onto_supported(gy, gx, c.cin, c.cout, c.k) and not _onto_route(c, m, a), f"{c.id}: dgrad_onto_supported disagrees with the route query"
        with _switches(c.sw):
            if onto:
                T.conv_dgrad_onto(gy, x if m else None, gold, gx, c.cin, c.cout, c.k, m, a, pk)
            else:
                T.conv_dgrad(gy, wt, x if m else None, gx, c.cin, c.cout, c.k, m, a, pk, impl, fold=c.fold)
            torch.cuda.synchronize()
        got, outside = _split(gxwhole, c.cin, slot)
        assert bool((outside == SENT).all()), f"{c.id}: channel blocks next to gx's view were written (their halo ring included)"
        if onto:
            assert np.array_equal(_np(goldwhole)[:, 8:8 + c.cin], old), f"{c.id}: gx_old was written"
        ref, S, A_fold = CC.def_dgrad(c, m, a)
        what = f"gx mask={m:#x} acc={a:#x}"
        if c.fold and hx and c.k == 3:
            ring = got.copy()
            ring[:, :, 1:-1, 1:-1] = 0
            assert float(np.abs(ring).max()) == 0.0, f"{c.id} {what}: the halo ring must stay zero"
        if c.dtype == "bf16":
            # fused fold / padded domain / 1x1: one rounding of |ref|; dgrad + stand-alone fold: the folded padded values, then the sum
            A = np.abs(ref) if (A_fold is None or _fused(c)) else A_fold + np.abs(ref)
            _check_bf16(c, _family(c), got, ref, A, S, what)
        else:
            _check_norm(c, _family(c), got, ref, _fp32_bar(c), what)


# ------------------------------------------------------------------------------------------------------------------------------ wgrad
WGRAD = [c for c in CASES if c.op == "wgrad"]


@pytest.mark.parametrize("c", WGRAD, ids=lambda c: c.id)
def test_weight_gradient_equals_definition(c):
    from mmif import tensor as T
    from mmif import _lib as L
    _assert_route(c)
    o, wt, pk, impl = _setup(c)
    gy, _ = _bt(o.gp, c.cout, c.h, c.w, c.gy_halo, _td(c), fill=0.0, flags=L.T_FOLDED)
    x, _ = _bt(o.x, c.cin, c.h, c.w, 0, _td(c), fill=0.0)
    ws = torch.empty(T.wgrad_workspace_bytes(c.cin, c.cout, c.k) // 4 + 1, dtype=torch.float32, device=DEV)
    bar = 1e-4 if c.impl != "x3" else 2e-5
    for acc in c.accumulate:
        dw = torch.from_numpy(o.dw_old.astype(np.float32)).to(DEV)
        db = torch.from_numpy(o.db_old.astype(np.float32)).to(DEV)
        with _switches(c.sw):
            T.conv_wgrad(x, gy, dw, db, c.cin, c.cout, c.k, ws, bool(acc), impl)
            torch.cuda.synchronize()
        _check_dw(c, _family(c), dw.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64), acc, bar)


# ------------------------------------------------------------------------------------------------------------------------------ one-call backward
BWD = [c for c in CASES if c.op in ("bwd_pair", "bwd_wide")]


@pytest.mark.parametrize("c", BWD, ids=lambda c: c.id)
def test_one_call_backward_equals_definition(c):
    """mmif_conv2d_reflect_bwd_pair / _bwd_wide straight against the definitions of gx (folded, masked, nothing accumulated), dw and db;
    bwd_wide also as its two halves in two calls (phase bits)"""
    from mmif import tensor as T
    from mmif import _lib as L
    o, wt, pk, impl = _setup(c)
    cbm = (1 << CC.cdiv(c.cin, 8)) - 1
    gy, _ = _bt(o.gp, c.cout, c.h, c.w, 1, _td(c), fill=0.0, flags=L.T_FOLDED)
    x, _ = _bt(o.x, c.cin, c.h, c.w, 0, _td(c), fill=0.0)
    ws = torch.empty(T.wgrad_workspace_bytes(c.cin, c.cout, c.k) // 4 + 1, dtype=torch.float32, device=DEV)
    signs = torch.full((T.bwd_wide_signs_bytes(c.n, c.cin, c.h, c.w) + 64,), 0xa5, dtype=torch.uint8, device=DEV)
    bar = 1e-4 if c.impl != "x3" else 2e-5
    slot = (1, 1)
    for m, _a in c.bits:
        m &= cbm
        _assert_route(c, m, 0)
        ref, S, _parts = CC.def_dgrad(dataclasses.replace(c, fold=True), m, 0, old=np.zeros_like(o.old))
        for acc in c.accumulate:
            for phased in ((False, True) if c.phases else (False,)):
                gx, gxwhole = _bt(CC.ring_zero(np.full(o.old.shape, 5.0)), c.cin, c.h, c.w, 1, _td(c), slot)
                dw = torch.from_numpy(o.dw_old.astype(np.float32)).to(DEV)
                db = torch.from_numpy(o.db_old.astype(np.float32)).to(DEV)
                if c.op == "bwd_pair":
                    T.conv_bwd_pair(gy, x, gx, dw, db, c.cin, c.cout, c.k, pk, ws, bool(acc))
                elif phased:
                    T.conv_bwd_wide(gy, x, gx, dw, db, c.cin, c.cout, c.k, pk, m, ws, signs, acc | 2)
                    T.conv_bwd_wide(gy, x, gx, dw, db, c.cin, c.cout, c.k, pk, m, ws, signs, 4)
                else:
                    T.conv_bwd_wide(gy, x, gx, dw, db, c.cin, c.cout, c.k, pk, m, ws, signs, acc)
                torch.cuda.synchronize()
                got, outside = _split(gxwhole, c.cin, slot)
                assert bool((outside == SENT).all()), f"{c.id}: channel blocks next to gx's view were written"
                ring = got.copy()
                ring[:, :, 1:-1, 1:-1] = 0
                assert float(np.abs(ring).max()) == 0.0, f"{c.id}: the halo ring must stay zero"
                what = f"gx mask={m:#x} acc={acc} phased={phased}"
                if c.dtype == "bf16":
                    _check_bf16(c, _family(c) + " gx", got, ref, np.abs(ref), S, what)      # fused fold: r = 1
                else:
                    _check_norm(c, _family(c) + " gx", got, ref, bar, what)
                _check_dw(c, _family(c), dw.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64), acc, bar)
    assert bool((signs[-64:] == 0xa5).all()), f"{c.id}: bytes behind the sign map were written"


DUP = [c for c in CASES if c.op == "dgrad_dup"]


@pytest.mark.parametrize("c", DUP, ids=lambda c: c.id)
def test_dgrad_with_masked_copies_equals_definition(c):
    """mmif_conv2d_reflect_dgrad_folded_dup: its own output = fold(dgrad), unmasked; blocks 6, 7 and 14, 15 of the 16-block copy tensor =
    channels 48..63 of it masked by [F > 0] of F's blocks 6, 7 and 14, 15; the copy tensor's other blocks and its ring untouched"""
    from mmif import tensor as T
    from mmif import _lib as L
    _assert_route(c)
    o, wt, pk, impl = _setup(c)
    gy, _ = _bt(o.gp, c.cout, c.h, c.w, 1, _td(c), fill=0.0, flags=L.T_FOLDED)
    Fm, _ = _bt(o.F, 128, c.h, c.w, 0, _td(c), fill=0.0)
    gx, gxwhole = _bt(CC.ring_zero(np.full(o.old.shape, 5.0)), c.cin, c.h, c.w, 1, _td(c), (1, 1))
    GF, GFwhole = _bt(CC.ring_zero(np.full((c.n, 128, c.h + 2, c.w + 2), SENT)), 128, c.h, c.w, 1, _td(c))
    assert T.conv_dgrad_dup_supported(gy, gx, c.cin, c.cout, c.k)
    T.conv_dgrad_dup(gy, gx, c.cin, c.cout, c.k, pk, GF, Fm, 3)
    torch.cuda.synchronize()
    got, outside = _split(gxwhole, c.cin, (1, 1))
    assert bool((outside == SENT).all())
    ref, S, _ = CC.def_dgrad(c, 0, 0, old=np.zeros_like(o.old))
    _check_bf16(c, _family(c), got, ref, np.abs(ref), S, "gx")
    gf = _np(GFwhole)
    want_untouched = CC.ring_zero(np.full(gf.shape, SENT))
    for blocks in (slice(0, 48), slice(64, 112)):
        assert np.array_equal(gf[:, blocks], want_untouched[:, blocks]), "other blocks of the copy tensor were written"
    for lo in (48, 112):
        keep = np.zeros((c.n, 16, c.h + 2, c.w + 2))
        keep[:, :, 1:-1, 1:-1] = o.F[:, lo:lo + 16] > 0
        assert float(np.abs(gf[:, lo:lo + 16] * (1 - keep))[:, :, 1:-1, 1:-1].max()) == 0.0
        _check_bf16(c, _family(c) + " copies", gf[:, lo:lo + 16], ref[:, 48:64] * keep, np.abs(ref[:, 48:64]) * keep, S[:, 48:64], f"copy at {lo}")
        assert np.array_equal(gf[:, lo:lo + 16], got[:, 48:64] * keep), "a masked copy is the rounded output itself where the mask passes"


def test_zz_report_error_over_bound_per_family():
    """prints the measured maximum of every family as a fraction of its bound ($MMIF_SWEEP_REPORT: also as JSON).  A family below 1 % of its
    bound would have a bound that pins nothing."""
    for k in sorted(RATIOS):
        r, e, n = RATIOS[k]
        print(f"{k:48s} max err/bound {r:8.4f}   max err {e:.3e}   checks {n}")
    path = os.environ.get("MMIF_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)
    loose = [k for k in sorted(DERIVED) if RATIOS[k][0] < 0.01]
    assert not loose, f"bounds that pin nothing (max error below 1 % of the bound): {loose}"
