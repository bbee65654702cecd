"""Every case of tests/image_cases.py through the mmif.tensor wrappers of the image-side layers (csrc/conv_image.hip, csrc/image_bwd.hip): the
exact family bit for bit against the float64 definition, the real-valued family under the derived per-element bound (image_cases.bound: no
figure in this file was taken from a device run).  Every call also checks what it must NOT touch -- the other blocks of a wider buffer,
the sentinels around fp32 outputs -- and that a second call on the same operands gives the same bits."""
import numpy as np
import pytest
import torch

import image_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GARBAGE = -5.0            # what an output holds before the call where the call must overwrite it
SENTINEL = -777.25        # around fp32 outputs
PAD = 64


def _groups(cases):
    """the cases as a few test items (the suite's item count grows by tens, not by hundreds): one per data family and dtype, the long walk alone"""
    g = {}
    for c in cases:
        g.setdefault("long" if c.note == "long" else f"{c.family}-{c.dtype}", []).append(c)
    return [pytest.param(v, id=k) for k, v in g.items()]


def _sweep(cases, run):
    """every case of the item, whatever the earlier ones did: the failure names each case that missed.  Anything but a failed assertion (a
    HIP error) ends the item at once"""
    missed = []
    for c in cases:
        try:
            run(c)
        except AssertionError as e:
            missed.append(f"{c.id}: {str(e).splitlines()[0] if str(e) else 'assertion failed'}")
    assert not missed, f"{len(missed)} of {len(cases)} cases failed:\n" + "\n".join(missed)


def _td(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def blocked(c, a, halo=0, flags=0):
    """BT view (c.view) on a fresh buffer: a [n, 8 cb, hs, ws] in the view's blocks, FILL in the others"""
    from mmif import tensor as T
    n, C, hs, ws = a.shape
    cb = C // 8
    buf = torch.full((n, c.cb_total, hs, ws, 8), IC.FILL, dtype=torch.float64)
    buf[:, c.cb_off:c.cb_off + cb] = torch.from_numpy(np.ascontiguousarray(a)).reshape(n, cb, 8, hs, ws).permute(0, 1, 3, 4, 2)
    buf = buf.to(_td(c)).to(DEV)
    return T.BT(buf, n, hs - 2 * halo, ws - 2 * halo, halo, c.cb_total, c.cb_off, cb, T._CODE[_td(c)], flags)


def unblocked(t):
    """the view's contents as float64 [n, 8 cb, hs, ws]; the other blocks must still hold FILL"""
    b = t.buf.double().cpu()
    others = torch.cat([b[:, :t.cb_off], b[:, t.cb_off + t.cb:]], 1)
    assert bool((others == IC.FILL).all()), "a block outside the view was written"
    n, _, hs, ws, _ = b.shape
    return b[:, t.cb_off:t.cb_off + t.cb].permute(0, 1, 4, 2, 3).reshape(n, t.cb * 8, hs, ws).numpy()


class Guarded:
    """an fp32 output inside a larger sentinel-filled allocation"""

    def __init__(self, init):
        init = np.ascontiguousarray(init, dtype=np.float32)
        self.whole = torch.full((2 * PAD + init.size,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.whole[PAD:PAD + init.size].view(init.shape)
        self.t.copy_(torch.from_numpy(init))

    def get(self):
        w = self.whole.cpu()
        assert bool((w[:PAD] == SENTINEL).all()) and bool((w[-PAD:] == SENTINEL).all()), "a sentinel around an fp32 output was overwritten"
        return self.t.double().cpu().numpy()


def compare(c, got, ref, S, K, out_dtype, what, allow_zero=False):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64) + 0.0
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{c.id} {what}: non-finite output (poisoned pad lanes?)"
    assert allow_zero or np.abs(ref).max() > 0, f"{c.id} {what}: all-zero reference"      # (bias sums and masked maps of a few pixels may vanish)
    if c.family == "exact":
        IC.exact_condition(S, out_dtype, f"{c.id} {what}")
        g, r = got.astype(np.float32), ref.astype(np.float32)      # (bf16 values convert exactly: equal fp32 bits = equal bf16 bits)
        bad = g.view(np.int32) != r.view(np.int32)
        assert not bad.any(), f"{c.id} {what}: {int(bad.sum())} of {bad.size} elements differ from the exact result, first at " \
                              f"{tuple(np.argwhere(bad)[0])}: got {g[bad][0]!r}, exact {r[bad][0]!r}"
        return
    err, bnd = np.abs(got - ref), IC.bound(ref, S, K, out_dtype)
    bad = err > bnd
    assert not bad.any(), f"{c.id} {what}: {int(bad.sum())} of {bad.size} elements beyond the derived bound, worst err / bound = " \
                          f"{float((err / np.maximum(bnd, 1e-300)).max()):.3g} (err {float(err[bad].max()):.3e})"


def _ws(c):
    from mmif import tensor as T
    return torch.empty(T.image_wgrad_workspace_bytes(c.c, c.k) // 4 + 1, dtype=torch.float32, device=DEV)


def _twice(run):
    """run() -> tuple of torch tensors: a second call on the same operands is bit-identical"""
    a = run()
    b = run()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32), y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)), \
            "two calls on the same operands differ"
    return a


def _run_in_fwd(c):
    from mmif import tensor as T
    o = IC.operands(c)
    ref, S, K = IC.def_in_fwd(c)
    img, w, b = f32(o.img), f32(o.w), f32(o.b)
    out = []

    def run():
        y = blocked(c, np.full(ref.shape, GARBAGE))
        T.image_in_fwd(img, w, b, y, c.c, c.k, c.relu)
        out.append(y)
        return (y.buf,)
    _twice(run)
    compare(c, unblocked(out[0]), ref, S, K, c.dtype, "y")


def _wgrad_runs(c, call, definition):
    o = IC.operands(c)
    ws = _ws(c)
    for acc in c.accumulate:
        dw_ref, db_ref, Sw, Sb, K = definition(c, acc)
        out = []

        def run():
            dw, db = Guarded(o.dw_old), Guarded(o.db_old)      # non-zero old values: accumulate = 0 must overwrite them
            call(dw.t, db.t, ws, bool(acc))
            out.append((dw, db))
            return dw.whole, db.whole
        _twice(run)
        compare(c, out[0][0].get(), dw_ref, Sw, K, "f32", f"dw(accumulate={acc})")
        compare(c, out[0][1].get(), db_ref, Sb, K, "f32", f"db(accumulate={acc})", allow_zero=True)


def _run_in_wgrad(c):
    from mmif import _lib, tensor as T
    o = IC.operands(c)
    img = f32(o.img)
    gy = blocked(c, o.gp, c.halo, _lib.T_FOLDED if (c.halo and c.folded) else 0)
    _wgrad_runs(c, lambda dw, db, ws, acc: T.image_in_wgrad(img, gy, dw, db, c.c, c.k, ws, acc), IC.def_in_wgrad)
    unblocked(gy)


def _run_out_fwd(c):
    from mmif import tensor as T
    o = IC.operands(c)
    ref, S, K = IC.def_out_fwd(c)
    x, w, b = blocked(c, o.x), f32(o.w), f32(o.b)
    out = []

    def run():
        img = Guarded(np.full(ref.shape, GARBAGE))
        T.image_out_fwd(x, w, b, img.t, c.c, c.k, c.relu)
        out.append(img)
        return (img.whole,)
    _twice(run)
    compare(c, out[0].get(), ref, S, K, "f32", "img")


def _run_out_dgrad(c):
    from mmif import tensor as T
    o = IC.operands(c)
    gimg, yimg, w, x = f32(o.gimg), f32(o.yimg), f32(o.w), blocked(c, o.x)
    view_bits = (1 << c.cb) - 1
    for m, a in c.bits:
        m, a = m & view_bits, a & view_bits
        ref, S, K = IC.def_out_dgrad(c, m, a)
        out = []

        def run():
            gx = blocked(c, o.old, c.halo)
            T.image_out_dgrad(gimg, yimg, w, x if m else None, gx, c.c, c.k, m, a)
            out.append(gx)
            return (gx.buf,)
        _twice(run)
        compare(c, unblocked(out[0]), ref, S, K, c.dtype, f"gx(mask={m:#x},accum={a:#x})", allow_zero=m != 0)


def _run_out_wgrad(c):
    from mmif import tensor as T
    o = IC.operands(c)
    x, gimg, yimg = blocked(c, o.x), f32(o.gimg), f32(o.yimg)
    _wgrad_runs(c, lambda dw, db, ws, acc: T.image_out_wgrad(x, gimg, yimg, dw, db, c.c, c.k, ws, acc), IC.def_out_wgrad)
    unblocked(x)


def _gx_init(c):
    """gx of the fused backward on entry: a zero ring (the contract), an interior the call must overwrite"""
    a = np.zeros((c.n, 16, c.h + 2, c.w + 2))
    a[:, :, 1:-1, 1:-1] = GARBAGE
    return a


def _run_out_bwd(c):
    from mmif import tensor as T
    o = IC.operands(c)
    x, gimg, yimg, w = blocked(c, o.x), f32(o.gimg), f32(o.yimg), f32(o.w)
    assert T.image_out_bwd_supported(x, c.c, c.k)
    ws = _ws(c)
    for acc in c.accumulate:
        gx_ref, Sx, Kx, dw_ref, db_ref, Sw, Sb, K = IC.def_out_bwd(c, acc)
        out = []

        def run():
            gx, dw, db = blocked(c, _gx_init(c), 1), Guarded(o.dw_old), Guarded(o.db_old)
            T.image_out_bwd(x, gimg, yimg, w, gx, dw.t, db.t, c.c, c.k, ws, bool(acc))
            out.append((gx, dw, db))
            return gx.buf, dw.whole, db.whole
        _twice(run)
        gx, dw, db = out[0]
        got = unblocked(gx)
        ring = got.copy()
        ring[:, :, 1:-1, 1:-1] = 0
        assert not ring.any(), "the ring of gx must stay zero"
        compare(c, got, gx_ref, Sx, Kx, "bf16", f"gx(accumulate={acc})")
        compare(c, dw.get(), dw_ref, Sw, K, "f32", f"dw(accumulate={acc})")
        compare(c, db.get(), db_ref, Sb, K, "f32", f"db(accumulate={acc})", allow_zero=True)


def _run_bwd_vs_three(c):
    """the fused launch against the three it replaces, on integers: the fold's extra bf16 rounding vanishes, all three outputs agree bit for bit"""
    from mmif import tensor as T
    o = IC.operands(c)
    x, gimg, yimg, w = blocked(c, o.x), f32(o.gimg), f32(o.yimg), f32(o.w)
    ws = _ws(c)
    gx1, dw1, db1 = blocked(c, np.zeros((c.n, 16, c.h + 2, c.w + 2)), 1), Guarded(o.dw_old), Guarded(o.db_old)
    T.image_out_bwd(x, gimg, yimg, w, gx1, dw1.t, db1.t, c.c, c.k, ws)
    gx2, dw2, db2 = blocked(c, np.full((c.n, 16, c.h + 2, c.w + 2), GARBAGE), 1), Guarded(o.dw_old), Guarded(o.db_old)
    T.image_out_wgrad(x, gimg, yimg, dw2.t, db2.t, c.c, c.k, ws)
    T.image_out_dgrad(gimg, yimg, w, x, gx2, c.c, c.k, 3, 0)
    gx2.fold_halo_()
    torch.cuda.synchronize()
    a, b = unblocked(gx1), unblocked(gx2)
    assert np.abs(a).max() > 0 and not a[:, :, 0].any() and not a[:, :, -1].any() and not a[:, :, :, 0].any() and not a[:, :, :, -1].any()
    assert torch.equal(gx1.buf.view(torch.int16), gx2.buf.view(torch.int16)), f"gx differs at {int((a != b).sum())} elements"
    assert torch.equal(dw1.whole.view(torch.int32), dw2.whole.view(torch.int32)) and np.abs(dw1.get()).max() > 0, "dw"
    assert torch.equal(db1.whole.view(torch.int32), db2.whole.view(torch.int32)), "db"


# ------------------------------------------------------------------------------------------------------------------------------
# one parametrised test per entry point; an item runs every case of its family and dtype (tests/image_cases.py: CASES)
# ------------------------------------------------------------------------------------------------------------------------------
def _of(entry):
    return _groups([c for c in IC.CASES if c.entry == entry])


@pytest.mark.parametrize("cases", _of("in_fwd"))
def test_image_in_fwd(cases):
    _sweep(cases, _run_in_fwd)


@pytest.mark.parametrize("cases", _of("in_wgrad"))
def test_image_in_wgrad(cases):
    _sweep(cases, _run_in_wgrad)


@pytest.mark.parametrize("cases", _of("out_fwd"))
def test_image_out_fwd(cases):
    _sweep(cases, _run_out_fwd)


@pytest.mark.parametrize("cases", _of("out_dgrad"))
def test_image_out_dgrad(cases):
    _sweep(cases, _run_out_dgrad)


@pytest.mark.parametrize("cases", _of("out_wgrad"))
def test_image_out_wgrad(cases):
    _sweep(cases, _run_out_wgrad)


@pytest.mark.parametrize("cases", _of("out_bwd"))
def test_image_out_bwd(cases):
    _sweep(cases, _run_out_bwd)


@pytest.mark.parametrize("cases", _groups(IC.BWD_VS_THREE))
def test_image_out_bwd_equals_wgrad_dgrad_fold_bit_for_bit(cases):
    _sweep(cases, _run_bwd_vs_three)
