"""The image-side layers' fp64 definitions (tests/image_cases.py) against torch's float64 autograd of F.pad(mode='reflect') + conv2d (+ relu),
the accumulate-then-mask order against a hand-written example, the exact family's representability condition for every case, and the case
list against the library's own plan (mmif_conv2d_image_plan: pure host code, no GPU).  tests/test_gpu_image_sweep.py runs the cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_cases as IC
from conv_cases import ALL, M5A, M33
from oracle import fusion_oracle as O

TOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.abs(b).max() > 0, f"{what}: all-zero reference"
    assert np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max()), (what, np.abs(a - b).max())


def _autograd(x, w, b, g0):
    """y, dL/dx, dL/dw, dL/db of L = sum(g0 * (b + conv2d(reflect_pad(x), w))) in float64"""
    xt, wt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    bt = torch.from_numpy(b if b is not None else np.zeros(w.shape[0])).requires_grad_(True)
    p = w.shape[2] // 2
    y = F.conv2d(F.pad(xt, (p,) * 4, mode="reflect") if p else xt, wt, bt)
    (y * torch.from_numpy(g0)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


SHAPES = [(3, 2, 5, 7), (3, 1, 2, 2), (3, 2, 17, 33), (1, 2, 5, 7), (1, 1, 1, 5), (3, 1, 4, 4)]


@pytest.mark.parametrize("k,n,h,w", SHAPES)
@pytest.mark.parametrize("big", [False, True], ids=["numpy", "torch"])
def test_the_three_operators_equal_autograd(k, n, h, w, big):
    """conv_fwd / conv_wgrad / conv_dgrad_padded, both the numpy loops and the one-conv2d form the long-walk case uses"""
    rng = np.random.default_rng(k * 1000 + h * 10 + w)
    for cin, cout in ((1, 12), (12, 1)):
        x, wt, b = rng.standard_normal((n, cin, h, w)), rng.standard_normal((cout, cin, k, k)), rng.standard_normal(cout)
        g = rng.standard_normal((n, cout, h, w))
        y, dx, dw, db = _autograd(x, wt, b, g)
        _close(IC.conv_fwd(x, wt, b, big), y, "fwd")
        gw, gb = IC.conv_wgrad(x, wt.shape, g, big)
        _close(gw, dw, "dw")
        _close(gb, db, "db")
        _close(O.reflect_pad_adjoint(IC.conv_dgrad_padded(g, wt, big), k // 2), dx, "dx")


def _pick(entry, **kw):
    out = [c for c in IC.CASES if c.entry == entry and c.family == "real" and c.dtype == "f32" and all(getattr(c, a) == v for a, v in kw.items())]
    assert out, (entry, kw)
    return out


@pytest.mark.parametrize("c", _pick("in_fwd", h=17) + _pick("in_fwd", h=2) + _pick("in_fwd", k=1, h=1), ids=lambda c: c.id)
def test_image_in_fwd_definition(c):
    o = IC.operands(c)
    y, _, _, _ = _autograd(o.img[:, None], o.w, o.b, np.ones((c.n, c.c, c.h, c.w)))
    ref, S, K = IC.def_in_fwd(c)
    _close(ref[:, :c.c], np.maximum(y, 0) if c.relu else y, "y")
    assert not ref[:, c.c:].any() and not S[:, c.c:].any(), "pad lanes of the view are written as zero"
    assert (S[:, :c.c] >= np.abs(ref[:, :c.c]) - 1e-12).all() and K == c.k * c.k + 1


@pytest.mark.parametrize("c", _pick("out_fwd", h=17) + _pick("out_fwd", h=2) + _pick("out_fwd", k=1, h=1), ids=lambda c: c.id)
def test_image_out_fwd_definition(c):
    o = IC.operands(c)
    y, _, _, _ = _autograd(o.x[:, :c.c], o.w, o.b, np.ones((c.n, 1, c.h, c.w)))
    ref, S, K = IC.def_out_fwd(c)
    _close(ref, (np.maximum(y, 0) if c.relu else y)[:, 0], "img")
    assert (S >= np.abs(ref) - 1e-12).all() and K == c.c * c.k * c.k + 1
    if c.c % 8:
        assert np.abs(o.x[:, c.c:]).min() > 0.9 * IC.POISON and np.abs(ref).max() < 1e6, "poisoned pad lanes never reach the result"


@pytest.mark.parametrize("c", _pick("in_wgrad", h=17) + _pick("in_wgrad", h=2) + _pick("in_wgrad", k=1, h=1), ids=lambda c: c.id)
def test_image_in_wgrad_definition(c):
    """the three gradient states: the loss reads the layer's output directly (halo 0 / folded) or through the next layer's reflect padding"""
    o = IC.operands(c)
    xt, wt = torch.from_numpy(o.img[:, None]), torch.from_numpy(o.w).requires_grad_(True)
    bt = torch.zeros(c.c, dtype=torch.float64, requires_grad=True)
    p = c.k // 2
    y = F.conv2d(F.pad(xt, (p,) * 4, mode="reflect") if p else xt, wt, bt)
    gp = torch.from_numpy(o.gp[:, :c.c])
    if c.halo and not c.folded:
        y = F.pad(y, (1, 1, 1, 1), mode="reflect")
    elif c.halo:
        assert not o.gp[:, :c.c, 0].any() and not o.gp[:, :c.c, :, -1].any(), "a folded gradient has a zero ring"
        gp = gp[:, :, 1:-1, 1:-1]
    (y * gp).sum().backward()
    dw, db, Sw, Sb, K = IC.def_in_wgrad(c, 0)
    _close(dw, wt.grad.numpy(), "dw")
    _close(db, bt.grad.numpy(), "db")
    dw1, db1, _, _, K1 = IC.def_in_wgrad(c, 1)
    _close(dw1 - o.dw_old, dw, "accumulate dw")
    _close(db1 - o.db_old, db, "accumulate db")
    assert K1 == K + 1 and K == c.n * ((c.h + 2) * (c.w + 2) if (c.halo and not c.folded) else c.h * c.w)


@pytest.mark.parametrize("c", _pick("out_wgrad", h=17) + _pick("out_wgrad", h=2) + _pick("out_wgrad", k=1, h=1), ids=lambda c: c.id)
def test_image_out_wgrad_definition(c):
    o = IC.operands(c)
    g0 = IC.g0_of(o)
    if c.relu and o.yimg.size >= 64:
        assert (o.yimg < 0).any() and (o.yimg == 0).any() and ((g0[:, 0] != 0) <= (o.yimg > 0)).all(), "the > 0 mask sees negatives and zeros"
    _, _, gw, gb = _autograd(o.x[:, :c.c], o.w, o.b, g0)
    dw, db, _, _, K = IC.def_out_wgrad(c, 0)
    _close(dw, gw, "dw")
    _close(db, gb, "db")
    dw1, db1, _, _, _ = IC.def_out_wgrad(c, 1)
    _close(dw1 - o.dw_old, dw, "accumulate dw")
    _close(db1 - o.db_old, db, "accumulate db")


@pytest.mark.parametrize("c", _pick("out_dgrad", h=17, halo=1) + _pick("out_dgrad", h=2) + _pick("out_dgrad", k=1, h=1), ids=lambda c: c.id)
def test_image_out_dgrad_definition(c):
    """unmasked: folding the stored domain gives autograd's dL/dx; masked at the reflected source: folding gives dL/dx [x > 0];
    accumulate adds the old contents before the mask; lanes >= cin hold the (masked) old value or zero"""
    o = IC.operands(c)
    _, dx, _, _ = _autograd(o.x[:, :c.c], o.w, o.b, IC.g0_of(o))
    ref, S, K = IC.def_out_dgrad(c, 0, 0)
    fold = (lambda a: O.reflect_pad_adjoint(a, 1)) if (c.halo and c.h > 1) else (lambda a: a[:, :, c.halo:c.halo + c.h, c.halo:c.halo + c.w])
    if c.k == 1 and c.halo:
        assert not ref[:, :, 0].any() and not ref[:, :, :, 0].any(), "a 1x1 layer scatters nothing onto the ring"
        fold = lambda a: a[:, :, 1:-1, 1:-1]      # noqa: E731
    _close(fold(ref[:, :c.c]), dx, "dx")
    assert not ref[:, c.c:].any() and K == c.k * c.k + 1
    full = (1 << c.cb) - 1
    masked, _, _ = IC.def_out_dgrad(c, full, 0)
    _close(fold(masked[:, :c.c]), dx * (o.x[:, :c.c] > 0), "dx masked")
    both, S2, _ = IC.def_out_dgrad(c, full, full)
    xs = IC.reflect_pad(o.x, c.halo)
    np.testing.assert_array_equal(both, (ref + o.old) * (xs > 0) + 0.0)
    np.testing.assert_array_equal(S2, S + np.abs(o.old))
    if c.cb >= 2:      # block-wise bits
        part, _, _ = IC.def_out_dgrad(c, 0b01, 0b10)
        np.testing.assert_array_equal(part[:, :8], masked[:, :8])
        np.testing.assert_array_equal(part[:, 8:16], (ref + o.old)[:, 8:16])


def test_accumulate_then_mask_order_by_hand():
    """one pixel, one block: the scatter gives 5, gx held -7, x = 0 there.  accumulate first, then mask: (5 + -7) [0 > 0] = 0 -- not
    5 [0 > 0] + -7 = -7; with x = 2: -2; a -0.0 activation masks like 0"""
    val, old = np.full((1, 8, 1, 1), 5.0), np.full((1, 8, 1, 1), -7.0)
    assert (IC.apply_bits(val, old, np.zeros((1, 8, 1, 1)), 1, 1) == 0.0).all()
    assert (IC.apply_bits(val, old, np.full((1, 8, 1, 1), 2.0), 1, 1) == -2.0).all()
    assert (IC.apply_bits(val, old, np.full((1, 8, 1, 1), -0.0), 1, 0) == 0.0).all()
    assert (IC.apply_bits(val, old, np.zeros((1, 8, 1, 1)), 0, 1) == -2.0).all() and (IC.apply_bits(val, old, None, 0, 0) == 5.0).all()


@pytest.mark.parametrize("c", [c for c in IC.CASES if c.entry == "out_bwd" and c.family == "real"][:4], ids=lambda c: c.id)
def test_image_out_bwd_definition(c):
    o = IC.operands(c)
    _, dx, gw, gb = _autograd(o.x, o.w, o.b, IC.g0_of(o))
    gx, Sx, Kx, dw, db, _, _, _ = IC.def_out_bwd(c, 0)
    _close(gx[:, :, 1:-1, 1:-1], dx * (o.x > 0), "gx")
    ring = gx.copy()
    ring[:, :, 1:-1, 1:-1] = 0
    assert not ring.any(), "the ring stays zero"
    _close(dw, gw, "dw")
    _close(db, gb, "db")
    assert set(np.unique(Kx[:, :, 1:-1, 1:-1])) == {9.0, 18.0, 36.0} and Kx[0, 0, 2, 2] == 36 and Kx[0, 0, 1, 2] == 18


def test_bound_and_bf16_spacing():
    assert IC.half_spacing_bf16(1.0) == 2.0 ** -8 and IC.half_spacing_bf16(1.99) == 2.0 ** -8 and IC.half_spacing_bf16(2.0) == 2.0 ** -7
    assert IC.half_spacing_bf16(0.0) == 0.0 and IC.half_spacing_bf16(255.0) == 0.5
    v = np.abs(np.random.default_rng(0).standard_normal(1000)) * 10
    assert (np.abs(O.bf16_round(v) - v.astype(np.float32)) <= IC.half_spacing_bf16(v)).all()
    assert (IC.half_spacing_bf16(v) <= 2.0 ** -8 * v).all()
    ref, S = np.array([3.0]), np.array([10.0])
    assert IC.bound(ref, S, 10, "f32")[0] == 10 * 2.0 ** -24 * 10 + 2.0 ** -24 * 3
    assert IC.bound(ref, S, 10, "bf16")[0] == 10 * 2.0 ** -24 * 10 + 2.0 ** -7


def _case_groups():
    g = {}
    for c in IC.CASES:
        g.setdefault(f"{c.entry}-{c.family}-{c.dtype}", []).append(c)
    return [pytest.param(v, id=k) for k, v in g.items()]


@pytest.mark.parametrize("cases", _case_groups())
def test_references_are_exact_where_claimed_and_never_vacuous(cases):
    """exact family: integers whose |terms| stay inside the output type's gap-free range -- the float64 reference is then the exact result of
    ANY summation order, and an integer.  Both families: no reference the sweep relies on is all zero.  (One item per entry, family and dtype;
    the failure names the case.)"""
    missed = []
    for c in cases:
        try:
            _references_of(c)
        except AssertionError as e:
            missed.append(f"{c.id}: {str(e).splitlines()[0] if str(e) else 'assertion failed'}")
    assert not missed, "\n".join(missed)


def _references_of(c):
    o = IC.operands(c)
    ex = c.family == "exact"
    if ex:
        for a in (o.img, o.x[:, :c.c] if o.x is not None else None, o.w, o.b, o.gp[:, :c.c] if o.gp is not None else None, o.gimg, o.yimg, o.old,
                  o.dw_old, o.db_old):
            assert a is None or (a == np.round(a)).all()
        if o.x is not None:
            z = o.x[:, :c.c] == 0
            assert 0.3 < z.mean() < 0.5 or z.size < 200, z.mean()
            assert np.signbit(o.x[:, :c.c][z]).any() or z.sum() < 24, "some zeros are negative"
    refs = list(IC.references(c))
    assert len(refs) == {"in_fwd": 1, "out_fwd": 1, "out_dgrad": len(c.bits), "out_bwd": 3 * len(c.accumulate)}.get(c.entry, 2 * len(c.accumulate))
    for what, ref, S, K, out_dtype, allow_zero in refs:
        assert allow_zero or np.abs(ref).max() > 0, what
        assert (S >= np.abs(ref) - 1e-9).all() and np.min(K) >= 0, what
        if ex:
            IC.exact_condition(S, out_dtype, f"{c.id} {what}")
            assert (ref == np.round(ref)).all(), what
            assert out_dtype == "f32" or np.abs(ref).max() <= (216 if c.entry == "out_bwd" else 85), what


def test_exact_condition_refuses_what_is_not_exact():
    IC.exact_condition(np.array([256.0]), "bf16")
    IC.exact_condition(np.array([2.0 ** 24 - 1]), "f32")
    for S, t in ((257.0, "bf16"), (2.0 ** 24, "f32")):
        with pytest.raises(AssertionError):
            IC.exact_condition(np.array([S]), t)


# ------------------------------------------------------------------------------------------------------------------------------
# the case list against the library's plan
# ------------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_is_reached_in_every_dtype_it_supports():
    names = {}
    for c in IC.CASES:
        p = c.plan()
        assert p is not None, f"{c.id}: the library would refuse this case"
        names.setdefault(p.name, set()).add(c.family)
    missing = [n for n in IC.REQUIRED_NAMES if names.get(n) != {"exact", "real"}]
    assert not missing, f"kernels without a case in both data families: {missing}"
    assert set(names) == set(IC.REQUIRED_NAMES), sorted(set(names) ^ set(IC.REQUIRED_NAMES))
    # the nine kernels: 5 templates x 2 dtypes x 2 kernel sizes + the two persistent 16-channel kernels + the fp32 tiled one
    assert len(IC.REQUIRED_NAMES) == 23
    # every entry has every mechanism the issue lists
    for e in IC.ENTRIES:
        cs = [c for c in IC.CASES if c.entry == e]
        assert {c.view for c in cs} == {(0, 0), (1, 4), (8, 16)}, e
        assert {c.c for c in cs} == ({16} if e == "out_bwd" else {8, 12, 16, 24, 64}), e
        assert {c.k for c in cs} == ({3} if e == "out_bwd" else {1, 3}), e
        assert {c.relu for c in cs} == {False, True} or e == "in_wgrad", e
    assert {(c.halo, c.folded, c.k) for c in IC.CASES if c.entry == "in_wgrad"} >= {(0, True, 3), (1, True, 3), (1, False, 3), (0, True, 1), (1, True, 1)}
    assert {(c.halo, c.k) for c in IC.CASES if c.entry == "out_dgrad"} == {(1, 3), (1, 1), (0, 1)}
    assert all(set(c.bits) == {(M5A, M33), (ALL, ALL), (0, 0), (M33, 0)} for c in IC.CASES if c.entry == "out_dgrad")
    assert {(c.relu, c.bias) for c in IC.CASES if c.entry in ("in_fwd", "out_fwd") and c.c == 16} == {(a, b) for a in (False, True) for b in (False, True)}


def test_tile_seams_and_the_persistent_walk_are_what_the_cases_claim():
    def pl(entry, dtype, shape, c=16, k=3, halo=0):
        n, h, w = shape
        return IC.plan(entry, dtype, c, k, IC.cdiv(c, 8), n, h, w, halo)
    # 16 x 16 tiles; dgrad tiles the stored domain
    for shape, t, td in zip(IC.T16, (1, 1, 12, 2, 12), (4, 1, 12, 6, 12)):
        assert pl("in_fwd", "bf16", shape).tiles == t and pl("out_fwd", "f32", shape).tiles == t, shape
        assert pl("out_dgrad", "bf16", shape, halo=1).tiles == td, shape
    assert pl("out_dgrad", "bf16", (1, 16, 16), k=1, halo=0).tiles == 1
    # 8 x 32 tiles
    for shape, t in zip(IC.T8X32, (1, 4, 1 * 2, 4, 9, 9)):
        for entry in ("out_fwd", "out_bwd"):
            p = pl(entry, "bf16", shape)
            assert (p.name, p.tiles) == ("image_out_fwd16" if entry == "out_fwd" else "image_out_bwd16", t), (shape, p)
    # the persistent walk: G is a multiple of 8 from 8 on (XCD bands of tiles // 8 or one more), the plain walk below
    for (n, h, w), G in zip(IC.WALK, (1, 7, 8, 8, 8, 16)):
        for entry in ("out_fwd", "out_bwd"):
            p = pl(entry, "bf16", (n, h, w))
            assert (p.tiles, p.G) == (n, G), (entry, n, p)
    # the long walk
    pb, pf = pl("out_bwd", "bf16", IC.LONG), pl("out_fwd", "bf16", IC.LONG)
    assert pb.tiles == pf.tiles == 3658 and pb.tiles % 8 != 0 and (pb.G, pf.G) == (512, 1024)
    band = pb.tiles // 8                         # the shortest XCD band, shared by G / 8 blocks
    assert band // (pb.G // 8) >= 7 and band % (pb.G // 8) != 0, "every bwd16 block owns >= 7 tiles, and not all the same number"
    assert band // (pf.G // 8) >= 3 and band % (pf.G // 8) != 0, "every fwd16 block owns >= 3 tiles, and not all the same number"
    for entry in ("in_wgrad", "out_wgrad"):
        p = pl(entry, "bf16", IC.LONG)
        assert p.G == 512 and p.tiles > p.G and p.slices == 16, "the weight-gradient blocks stride over the pixels"
    long_ = [c for c in IC.CASES if c.note == "long"]
    assert {c.entry for c in long_} == {"out_fwd", "out_bwd", "out_wgrad", "in_wgrad"} and all(c.family == "exact" for c in long_)
    # weight gradients: one block per 256 pixels up to 512
    assert pl("out_wgrad", "f32", (1, 16, 16)).G == 1 and pl("in_wgrad", "f32", (2, 17, 33)).G == 5


def test_the_plan_refuses_what_the_entries_refuse():
    from mmif._lib import lib
    assert IC.plan("in_fwd", "bf16", 16, 5, 2, 1, 8, 8) is None and b"ksize must be 1 or 3" in lib.mmif_last_error()
    assert IC.plan("in_fwd", "bf16", 17, 3, 2, 1, 8, 8) is None
    assert IC.plan("out_fwd", "bf16", 16, 3, 2, 1, 1, 8) is None and b"h,w >= 2" in lib.mmif_last_error()
    assert IC.plan("out_fwd", "bf16", 16, 1, 2, 1, 1, 8) is not None
    assert IC.plan("out_dgrad", "bf16", 16, 3, 2, 1, 8, 8, halo=0) is None
    assert IC.plan("out_bwd", "f32", 16, 3, 2, 1, 8, 8) is None and IC.plan("out_bwd", "bf16", 16, 3, 2, 1, 3, 8) is None
    # a 16-channel weight gradient on a 3-block view: the kernel would lay out two groups, the reduce reads one
    for entry in ("in_wgrad", "out_wgrad"):
        assert IC.plan(entry, "bf16", 16, 3, 3, 1, 8, 8) is None and b"16-channel groups" in lib.mmif_last_error()
        assert IC.plan(entry, "bf16", 24, 3, 3, 1, 8, 8) is not None and IC.plan(entry, "bf16", 8, 3, 1, 1, 8, 8) is not None
