"""tests/nest_cases.py without a GPU: its fp64 definitions of the blocked glue kernels against torch's float64 autograd of the plain module
chains and against the arrays the reference wrote into tests/golden/f4_blocks.npz; the case table shown to hold every axis value, state
combination, tie and zero configuration it claims, every attention denominator clearly in or clearly out of the clamp regime, every stride
case past the grid cap; and every listed wrong definition shown to differ from the true one by more than ten bounds on the cases it applies to."""
import collections
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nest_cases as NC
from nest_cases import CASES, Case
from oracle import fusion_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f4_blocks.npz")
LIVE = [c for c in CASES if not c.stride]


def _nerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    return t.requires_grad_(True) if grad else t


def _first(k, **kw):
    for c in LIVE:
        if c.k == k and all(getattr(c, a) == v for a, v in kw.items()):
            return c
    raise AssertionError((k, kw))


# ------------------------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("c", [c for c in LIVE if c.k == "pool_bwd" and c.dtype == "f32" and c.g == "h0" and not c.acc and not c.mask], ids=lambda c: c.id)
def test_pool_equals_maxpool2d_autograd(c):
    o = NC.operands(c)
    x = _t(o["x"], True)
    y = nn.MaxPool2d(2, 2)(x)
    assert _nerr(O.maxpool2x2_fwd(o["x"])[0], y.detach().numpy()) == 0
    y.backward(_t(o["g"]))
    assert _nerr(NC.pool_bwd_on(o["x"], o["g"]), x.grad.numpy()) <= 1e-12
    assert np.array_equal(NC.embed(x.grad.numpy()), NC.define(c)[0].want)


@pytest.mark.parametrize("h,w", NC.UP_SOURCES)
def test_upsample_equals_upsample_reflectionpad_autograd(h, w):
    """nn.Upsample(scale_factor=2, 'nearest') then nn.ReflectionPad2d((l, r, t, b)) with l = dw // 2, t = dh // 2, every admissible target;
    the index-map form the mutations are written on is the same function"""
    rng = np.random.default_rng(h * 16 + w)
    for dh, dw in NC._diffs(h, w):
        H, W = 2 * h + dh, 2 * w + dw
        xn, gn = rng.standard_normal((2, 3, h, w)), rng.standard_normal((2, 3, H, W))
        x = _t(xn, True)
        y = nn.ReflectionPad2d((dw // 2, dw - dw // 2, dh // 2, dh - dh // 2))(nn.Upsample(scale_factor=2, mode="nearest")(x))
        assert _nerr(NC.up_fwd_on(xn, H, W), y.detach().numpy()) == 0
        y.backward(_t(gn))
        assert _nerr(NC.up_bwd_on(gn, h, w), x.grad.numpy()) <= 1e-12
        iy, ix = NC.up_map(H, h, dh), NC.up_map(W, w, dw)
        assert np.array_equal(xn[:, :, iy][:, :, :, ix], y.detach().numpy())
        assert _nerr(np.einsum("nchw,hi,wj->ncij", gn, NC.up_onehot(H, h, dh), NC.up_onehot(W, w, dw)), x.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("mode", NC.ELEM_MODES)
@pytest.mark.parametrize("same", [False, True])
def test_element_fusion_equals_torch_autograd(mode, same):
    c = _first("elem_bwd", dtype="f32", mode=mode, g="h0", mask=0, same=same)
    o = NC.operands(c)
    a = _t(o["a"], True)
    b = a if same else _t(o["b"], True)
    y = torch.max(a, b) if mode == "max" else (a + b if mode == "sum" else (a + b) / 2)
    assert _nerr(O.element_fusion(o["a"], o["b"], mode), y.detach().numpy()) <= 1e-12
    y.backward(_t(o["g"]))
    ga, gb = (d.want for d in NC.define(c))
    if same:
        assert _nerr(ga + gb, a.grad.numpy()) <= 1e-12
    else:
        assert _nerr(ga, a.grad.numpy()) <= 1e-12 and _nerr(gb, b.grad.numpy()) <= 1e-12
        if mode == "max":
            assert ((o["a"] == o["b"]) & (o["a"] > 0)).any() and ((o["a"] == 0) & (o["b"] == 0)).any()


def _torch_attention(a, b, mode):
    """core/fusion.py restated: l1 spatial pooling, avg channel pooling, w = w1 / clamp(w1 + w2, min=eps), 'sca' the mean of the branches"""
    def weighted(w1, w2):
        w = w1 / (w1 + w2).clamp(min=1e-7)
        return w * a + (1 - w) * b
    sp = weighted(a.abs().sum(1, keepdim=True), b.abs().sum(1, keepdim=True))
    ch = weighted(a.mean((2, 3), keepdim=True), b.mean((2, 3), keepdim=True))
    return {"sa": sp, "ca": ch, "sca": (sp + ch) / 2}[mode]


@pytest.mark.parametrize("c", [c for c in LIVE if c.k == "attn_bwd" and c.dtype == "f32" and c.note == "all" and c.view and not c.acc] +
                         [c for c in LIVE if c.k == "attn_bwd" and c.dtype == "bf16" and c.h * c.w > 64 and not c.acc], ids=lambda c: c.id)
def test_attention_equals_torch_autograd(c):
    o = NC.operands(c)
    a, b = _t(o["a"], True), _t(o["b"], True)
    y = _torch_attention(a, b, c.mode)
    g = NC.logical(o["g"], c.g)
    fwd = NC.attn_fwd_on(o["a"], o["b"], c.mode)
    assert _nerr(fwd, y.detach().numpy()) <= 1e-12 and _nerr(fwd, O.attention_fusion(o["a"], o["b"], c.mode)) <= 1e-12
    y.backward(_t(g))
    ga, gb = NC.attn_bwd_on(o["a"], o["b"], g, c.mode)
    assert _nerr(ga, a.grad.numpy()) <= 1e-12 and _nerr(gb, b.grad.numpy()) <= 1e-12
    oa, ob = O.attention_fusion_bwd(o["a"], o["b"], g, c.mode)
    assert _nerr(ga, oa) <= 1e-12 and _nerr(gb, ob) <= 1e-12
    wa, wb = (d.want for d in NC.define(c))
    assert np.array_equal(NC.interior(wa), ga) and np.array_equal(NC.interior(wb), gb)
    assert (wa[:, :, 0] == NC.SENT).all() and (wb[:, :, :, -1] == NC.SENT).all()


@pytest.mark.parametrize("h,w", [(2, 2), (2, 5), (3, 3), (4, 3), (5, 7)])
def test_raw_kind_equals_autograd_through_reflect_pad(h, w):
    rng = np.random.default_rng(h * 8 + w)
    stored = rng.standard_normal((2, 8, h + 2, w + 2))
    x = _t(rng.standard_normal((2, 8, h, w)), True)
    (F.pad(x, (1, 1, 1, 1), mode="reflect") * _t(stored)).sum().backward()
    assert _nerr(NC.logical(stored, "raw"), x.grad.numpy()) <= 1e-12
    assert np.array_equal(NC.logical(stored, "folded"), stored[:, :, 1:-1, 1:-1]) and NC.logical(stored[:, :, 1:-1, 1:-1], "h0").shape == (2, 8, h, w)
    # an axis of extent 1 has no reflect source: its halo is dropped, the other axis folds as usual
    thin = rng.standard_normal((1, 8, 3, w + 2))
    want = thin[:, :, 1:2, 1:-1].copy()
    want[:, :, :, 1] += thin[:, :, 1:2, 0]
    want[:, :, :, w - 2] += thin[:, :, 1:2, w + 1]
    assert np.array_equal(NC.fold(thin), want) and np.array_equal(NC.fold(thin.transpose(0, 1, 3, 2)), want.transpose(0, 1, 3, 2))
    assert np.array_equal(NC.fold(thin[:, :, :, :3]), thin[:, :, 1:2, 1:2])


@pytest.mark.parametrize("k", ["relu_mask", "elem_bwd"])
def test_stored_domain_kernels_commute_with_the_fold(k):
    """masking the stored halo-1 array by the REFLECTED activation, then folding, is masking the folded gradient: what the engine relies on"""
    for c in LIVE:
        if c.k != k or c.g != "raw" or c.dtype != "f32" or (k == "elem_bwd" and not c.mask):
            continue
        o = NC.operands(c)
        outs = NC.define(c)
        if k == "relu_mask":
            assert _nerr(NC.fold(outs[0].want), NC.fold(o["g"]) * (o["x"] > 0)) <= 1e-12
        else:
            da, db = NC.elem_weights(o["a"], o["b"], c.mode, 1)
            assert _nerr(NC.fold(outs[0].want), NC.fold(o["g"]) * da) <= 1e-12 and _nerr(NC.fold(outs[1].want), NC.fold(o["g"]) * db) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------ golden
def test_definitions_reproduce_the_reference_arrays():
    """tests/golden/f4_blocks.npz holds what the reference's modules gave (float32) on the closed-form operands"""
    ref = np.load(GOLDEN)
    x, gy = O.closed_form_signed((1, 8, 10, 14), 0.77), O.closed_form_signed((1, 8, 5, 7), 0.31)
    assert np.array_equal(O.maxpool2x2_fwd(x)[0], ref["maxpool__y"]) and np.array_equal(NC.pool_bwd_on(x, gy), ref["maxpool__dx"])
    x, gy = O.closed_form_signed((1, 8, 4, 6), 0.57), O.closed_form_signed((1, 8, 9, 13), 0.41)
    assert np.array_equal(NC.up_fwd_on(x, 9, 13), ref["upsample__y"])
    assert _nerr(NC.up_bwd_on(gy.astype(np.float64), 4, 6), ref["upsample__dx"]) <= 1e-6
    s = (2, 16, 6, 10)
    a, b, g = (O.closed_form_signed(s, p).astype(np.float64) for p in (0.15, 1.25, 2.35))
    for mode in NC.ATTN_MODES:
        assert _nerr(NC.attn_fwd_on(a, b, mode), ref[f"attn_{mode}__y"]) <= 1e-5
        ga, gb = NC.attn_bwd_on(a, b, g, mode)
        assert _nerr(ga, ref[f"attn_{mode}__da"]) <= 1e-5 and _nerr(gb, ref[f"attn_{mode}__db"]) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------------------ the table
def test_the_table_covers_what_it_claims():
    assert {c.k for c in CASES} == set(NC.KERNELS)
    for dtype in NC.DTYPES:
        cs = [c for c in LIVE if c.dtype == dtype]
        for k in NC.KERNELS:
            ks = [c for c in cs if c.k == k]
            assert {1, 2, 3} <= {c.n for c in ks}, (k, dtype)
            assert {1, 2, 3} <= {c.cb for c in ks}, (k, dtype)
            assert any(c.view for c in ks) and any(not c.view for c in ks), (k, dtype)
            assert any(c.n > 1 and c.cb > 1 for c in ks), (k, dtype)
        # ---- every (kernel, dtype, gradient kind, accumulate, mask) the entry points take
        for k in ("pool_bwd", "up_bwd"):
            assert {(c.g, c.acc, c.mask) for c in cs if c.k == k} == set(NC.BWD_VARIANTS), (k, dtype)
        for mode in NC.ATTN_MODES:
            for inputs in ("relu", "signed"):
                assert {(c.g, c.acc, c.cached) for c in cs if c.k == "attn_bwd" and c.mode == mode and c.inputs == inputs} == \
                    {(g, acc, cached) for g in NC.KINDS for acc in (0, 1) for cached in (False, True)}, (dtype, mode, inputs)
                assert any(c.k == "attn_fwd" and c.mode == mode and c.inputs == inputs for c in cs)
        for mode in NC.ELEM_MODES:
            assert {(c.g, c.mask) for c in cs if c.k == "elem_bwd" and c.mode == mode} == {(g, m) for g in NC.KINDS for m in (0, 1)}
            assert any(c.k == "elem_fwd" and c.mode == mode and c.same for c in cs) and any(c.k == "elem_bwd" and c.mode == mode and c.same for c in cs)
        assert {c.g for c in cs if c.k == "relu_mask"} == set(NC.KINDS) == {c.g for c in cs if c.k == "to_nchw"}
        assert {c.g for c in cs if c.k == "to_blocked"} == {"h0", "folded"} == {c.g for c in cs if c.k == "zero"}
        for k in ("to_blocked", "to_nchw"):
            assert {c.c for c in cs if c.k == k} == set(NC.CONV_CHANNELS), k
            assert any(c.k == k and c.cb * 8 - c.c >= 8 for c in cs), "a view wider than the channels need"
        # ---- pool shapes
        for k in ("pool_fwd", "pool_bwd"):
            for v in (2, 3, 4, 5, 9):
                assert any(c.k == k and c.h == v for c in cs) and any(c.k == k and c.w == v for c in cs), (k, v)
            assert any(c.k == k and (c.h, c.w) == (2, 70) for c in cs) and any(c.k == k and (c.h, c.w) == (70, 3) for c in cs)
        for gh in (1, 2, 3):
            assert any(c.k == "pool_bwd" and c.g == "raw" and c.ghw[0] == gh for c in cs) and any(c.k == "pool_bwd" and c.g == "raw" and c.ghw[1] == gh for c in cs)
        # ---- up shapes: every source extent, every diff per axis independently, raw gradients at the target size, the largest pads
        for k in ("up_fwd", "up_bwd"):
            for v in (1, 2, 3, 4, 6):
                assert any(c.k == k and c.h == v for c in cs) and any(c.k == k and c.w == v for c in cs), (k, v)
            for src in NC.UP_FULL:
                assert {(c.dh, c.dw) for c in cs if c.k == k and (c.h, c.w) == src} == set(NC._diffs(*src)), (k, src)
            assert {(c.dh, c.dw) for c in cs if c.k == k} == {(i, j) for i in range(4) for j in range(4)}
            assert all(0 <= c.dh < 2 * c.h and 0 <= c.dw < 2 * c.w for c in cs if c.k == k)
        assert any(c.k == "up_bwd" and c.g == "raw" and c.dh == 3 and c.dw == 3 for c in cs)
        assert any(c.k == "up_bwd" and c.dh // 2 >= 1 for c in cs), "upsample_bwd_kernel's candidate list with top >= 1"
        # ---- attention plane sizes around the 256-thread slices and the 32 x 256 partition
        for k in ("attn_fwd", "attn_bwd"):
            assert {1, 255, 256, 257, 8191, 8192, 8193, 16385} <= {c.h * c.w for c in cs if c.k == k}, k
    # ---- the stride cases: one per kernel, one dtype each, really past the cap.  GRID_CAP_ITEMS = 8192 blocks x 256 threads is grid_for() of
    # csrc/nest.hip (csrc/misc.hip caps at 4096 blocks, so its kernels take a second trip too)
    assert NC.GRID_CAP_ITEMS == 8192 * 256
    stride = [c for c in CASES if c.stride]
    assert sorted(c.k for c in stride) == sorted(NC.KERNELS)
    for c in stride:
        assert c.items > NC.GRID_CAP_ITEMS and c.items < 1.01 * NC.GRID_CAP_ITEMS, (c.id, c.items)
        assert c.mutations() == [] and c.n == 1 and c.cb == 1
    assert all(c.dtype == "bf16" for c in stride if c.k in ("pool_fwd", "up_bwd"))
    assert all(c.items < 20000 * c.cb for c in LIVE), "everything but the stride cases stays small"


def test_ties_and_zeros_are_in_the_operands():
    ties, nz_ties, mixed = collections.Counter(), collections.Counter(), 0
    for c in LIVE:
        if c.k != "pool_bwd":
            continue
        o = NC.operands(c)
        t, z, m = NC.pool_tie_counts(o["x"])
        ties.update(t)
        nz_ties.update(z)
        mixed += m
        assert (o["x"] >= 0).all() and (o["x"] == 0).any(), "a ReLU output with exact zeros"
    assert all(ties[j] > 100 for j in (2, 3, 4)) and all(nz_ties[j] > 0 for j in (2, 3)) and mixed > 50, (ties, nz_ties, mixed)
    dead_pixels = dead_channels = negative_channels = partial_zero = 0
    for c in LIVE:
        if c.k not in ("attn_fwd", "attn_bwd"):
            continue
        o = NC.operands(c)
        a, b = o["a"], o["b"]
        if c.inputs == "relu":
            d = int(((np.abs(a) + np.abs(b)).sum(1) == 0).sum())
            assert d > 0 and (a[:, 2] == 0).all() and (b[:, 2] == 0).all(), c.id
            dead_pixels += d
            dead_channels += 1
            partial_zero += int(((a == 0).any(1) & (np.abs(a).sum(1) > 0)).sum())
            assert (a >= 0).all() and (b >= 0).all()
        else:
            s, sa = (a + b).sum((2, 3)), (np.abs(a) + np.abs(b)).sum((2, 3))
            negative_channels += int((s <= -0.1 * sa).sum())
            assert (a < 0).any() and (b < 0).any()
    assert dead_pixels > 1000 and dead_channels > 50 and negative_channels > 50 and partial_zero > 1000
    both_zero = equal_nonzero = 0
    for c in LIVE:
        if c.k == "elem_bwd" and c.mode == "max" and not c.same:
            o = NC.operands(c)
            both_zero += int(((o["a"] == 0) & (o["b"] == 0)).sum())
            equal_nonzero += int(((o["a"] == o["b"]) & (o["a"] != 0)).sum())
    assert both_zero > 100 and equal_nonzero > 100


@pytest.mark.parametrize("c", [c for c in LIVE if c.k in ("attn_fwd", "attn_bwd")], ids=lambda c: c.id)
def test_attention_denominators_are_clearly_in_or_out_of_the_clamp_regime(c):
    """every denominator (spatial: per pixel; channel: per (n, channel), on the means) is either exactly 0 or at most -0.1 x its sum of absolute
    terms, or at least 2^-6 x that sum and 2^10 eps: fp32 rounding of the sums cannot flip the `>= eps` branch on any case"""
    o = NC.operands(c)
    for s, sabs in NC.conditioning(o["a"], o["b"]):
        clamped = (s == 0) | (s <= -0.1 * sabs)
        live = (s >= 2.0 ** -6 * sabs) & (s >= 2.0 ** 10 * NC.EPS)
        assert bool((clamped ^ live).all()), f"{c.id}: {int((~(clamped ^ live)).sum())} denominators in between"


# ------------------------------------------------------------------------------------------------------------------------------ mutations
def _separation(c, mut, true):
    worst = 0.0
    for o, m in zip(true, NC.define(c, mut)):
        d = np.abs(m.want - o.want)
        worst = max(worst, float(np.max(d / np.maximum(o.bound, 1e-300) * (d > 0))))
    return worst


def test_every_case_is_alive_and_lists_its_mutations():
    for c in LIVE:
        for o in NC.define(c):
            defined = o.want != NC.SENT
            assert o.want.shape == o.bound.shape and np.isfinite(o.want).all() and np.isfinite(o.bound).all() and (o.bound >= 0).all(), c.id
            assert (o.bound[~defined] == 0).all(), c.id
            assert c.k == "zero" or float(np.abs(o.want[defined]).max()) > 0, f"{c.id}: {o.name} is all zero"
            if c.exact:
                assert not o.bound.any(), c.id
        assert set(c.mutations()) <= set(NC.MUTATIONS)


@pytest.mark.parametrize("mut", NC.MUTATIONS)
def test_mutation_is_separated_by_more_than_ten_bounds(mut):
    """the wrong definition differs from the true one by more than ten times the case's own bound on (nearly) every case that lists it: the
    GPU sweep fails if the kernel, or the definition, is changed into it"""
    cases = [c for c in LIVE if mut in c.mutations()]
    assert len(cases) >= 4, f"{mut}: no case can show it"
    for dtype in NC.DTYPES:
        assert any(c.dtype == dtype for c in cases)
    missed = [c.id for c in cases if _separation(c, mut, NC.define(c)) <= 10]
    print(f"{mut}: separated on {len(cases) - len(missed)} of {len(cases)} cases; not on {missed}")
    assert len(missed) <= 0.05 * len(cases), (mut, missed)


def test_rounding_counts_spelled_out():
    """K at the ends of the table (see Case.K)"""
    assert NC.fold_roundings(1, 1) == 0 and NC.fold_roundings(2, 5) == 3 and NC.fold_roundings(3, 3) == 8 and NC.fold_roundings(1, 3) == 2
    assert Case("attn_fwd", "f32", 1, 1, 4, 4, mode="sa").K() == (2 * 7 + 2) + 4
    assert Case("attn_fwd", "f32", 1, 1, 4, 4, mode="ca").K() == (2 * (1 + 6 + 4 + 32) + 5) + 4
    assert Case("attn_fwd", "f32", 1, 2, 5, 3277, mode="sca").K() == (2 * 15 + 2 + 4) + (2 * (3 + 42) + 5 + 4) + 1
    assert Case("attn_bwd", "f32", 1, 1, 4, 4, mode="sa", g="raw").K() == 16 + 24 + 3 + 5 + 2
    assert Case("attn_bwd", "f32", 1, 1, 4, 4, mode="ca", g="h0").K() == 91 + (3 + 42) + 0 + 5 + 3
    assert Case("pool_bwd", "f32", 1, 1, 6, 6, g="raw").K() == 8 and Case("pool_bwd", "f32", 1, 1, 6, 6, g="folded").K() == 0
    c = Case("up_bwd", "f32", 1, 1, 2, 2, dh=3, dw=3)
    assert NC.up_candidates(c).max() == 16 and NC.up_candidates(c).sum() == 49
