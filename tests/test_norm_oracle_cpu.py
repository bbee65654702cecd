"""tests/norm_cases.py without a GPU: its fp64 definitions of csrc/norm.hip's entry points against torch's float64 nn.BatchNorm2d (train and
eval), nn.GroupNorm(c, c) and the five activations through autograd, against oracle.fusion_oracle.norm_act_fwd / _bwd and the arrays of
tests/golden/f13_n4_norm.npz; the case table shown to hold every axis value it claims, every planted tie counted in the stored operands, no
bound beyond 1e-4 of its output's scale (the labelled ill-conditioned cases apart), and every listed wrong definition shown to differ from
the true one by more than ten bounds."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import norm_cases as NC
from norm_cases import CASES
from oracle import fusion_oracle as O
from test_oracle_golden import F13_CASES, f13_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f13_n4_norm.npz")
NORM = [c for c in CASES if c.ep in ("norm_fwd", "norm_bwd")]


def _nerr(a, b, scale=0.0):
    """max error relative to the largest reference value, or to `scale` where the output is a difference of larger terms (dx)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), scale, 1e-300)) if a.size else 0.0


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    return t.requires_grad_(True) if grad else t


def _torch_act(act, slope):
    return [nn.Identity(), nn.ReLU(), nn.LeakyReLU(slope), nn.Tanh(), nn.ReLU6()][act]


def _torch_norm(c, o, eps, mom):
    if c.kind == 2:
        mod = nn.GroupNorm(c.c, c.c, eps=eps).double()
    else:
        mod = nn.BatchNorm2d(c.c, eps=eps, momentum=mom, track_running_stats=o["running"] is not None).double()
        if o["running"] is not None:
            mod.running_mean.copy_(_t(o["running"][0]))
            mod.running_var.copy_(_t(o["running"][1]))
        mod.train(c.kind == 0)
    with torch.no_grad():
        mod.weight.copy_(_t(o["gamma"]) if o["gamma"] is not None else torch.ones(c.c, dtype=torch.float64))
        mod.bias.copy_(_t(o["beta"]) if o["beta"] is not None else torch.zeros(c.c, dtype=torch.float64))
    return mod


# ------------------------------------------------------------------------------------------------------------------------------ torch
@pytest.mark.parametrize("c", [c for c in NORM if not (c.kind == 0 and c.m == 1)], ids=lambda c: c.id)
def test_definition_equals_torch_float64_autograd(c):
    """forward, running buffers and all three gradients.  The backward definition takes y and stats as given: it is fed the float64 forward
    torch itself ran (no rounding to fp32, hence no planted tie), on every case's x, gamma, beta and gy."""
    o = NC.operands(c)
    eps, mom, slope = c.scalars()
    mod, act = _torch_norm(c, o, eps, mom), _torch_act(c.act, slope)
    x = _t(o["x"], True)
    y = act(mod(x))
    f = NC.fwd_on(o["x"], o["gamma"], o["beta"], c.kind, c.act, eps, slope, o["running"], mom)
    assert _nerr(f["y"], y.detach().numpy()) <= 1e-12
    if c.kind == 0 and o["running"] is not None:
        assert _nerr(f["running_mean"], mod.running_mean.numpy()) <= 1e-12 and _nerr(f["running_var"], mod.running_var.numpy()) <= 1e-12
    gy = o.get("gy")
    if gy is None:
        gy = np.random.default_rng(5).standard_normal(c.shape)
    y.backward(_t(gy))
    r = NC.bwd_on(o["x"], f["y"], gy, f["mean"], f["rstd"], o["gamma"], c.kind, c.act, slope)
    tol = 1e-12
    assert _nerr(r["dx"], x.grad.numpy(), NC.dx_scale(c, o["gamma"], f["rstd"], r)) <= tol
    # (dgamma = sum dz xhat with xhat of order 1: an exactly-zero want, at m = 1, is measured against sum |dz|)
    assert _nerr(r["dgamma"], mod.weight.grad.numpy(), float(np.abs(r["dz"]).sum((0, 2, 3)).max()) if c.m == 1 else 0.0) <= tol and _nerr(r["dbeta"], mod.bias.grad.numpy()) <= 1e-12
    if c.act in (1, 4):          # selections agree bit for bit: the same elements pass
        assert np.array_equal(NC.act_dydz(f["y"], c.act, slope) != 0, (y.detach().numpy() > 0) & ((y.detach().numpy() < 6) | (c.act == 1)))


def _torch_act_bwd(gy, y, act, slope):
    """torch's own backward kernels of the five activations, from the output y"""
    A = torch.ops.aten
    if act == 1:
        return A.threshold_backward(gy, y, 0.0)
    if act == 2:
        return A.leaky_relu_backward(gy, y, slope, True)
    if act == 3:
        return A.tanh_backward(gy, y)
    if act == 4:
        return A.hardtanh_backward(gy, y, 0.0, 6.0)
    return gy


@pytest.mark.parametrize("c", [c for c in NORM if c.ep == "norm_bwd" and c.plant != "ties"], ids=lambda c: c.id)
def test_backward_definition_on_the_stored_forward_equals_torch(c):
    """the path the GPU sweep takes: the STORED fp32 x, y, gy, stats, gamma go into torch's own float64 backward kernels (the activation's
    backward from y, aten.native_batch_norm_backward with save_mean / save_invstd = the stored stats, aten.native_group_norm_backward with
    the stored mean / rstd) on every backward case without a planted tie.  Eval mode takes its statistics from the running buffers: it is
    handed the running_var whose 1 / sqrt(var + eps) is the stored rstd."""
    o = NC.operands(c)
    eps, _, slope = c.scalars()
    x, y, gy = _t(o["x"]), _t(o["y"]), _t(o["gy"])
    w = _t(o["gamma"]) if o["gamma"] is not None else None
    mean, rstd = _t(o["mean"]), _t(o["rstd"])
    dz = _torch_act_bwd(gy, y, c.act, slope)
    if c.kind == 2:
        if w is None:          # (the group-norm kernel wants a weight to form dgamma: a NULL gamma is a gamma of ones)
            w = torch.ones(c.c, dtype=torch.float64)
        dx, dg, db = torch.ops.aten.native_group_norm_backward(dz, x, mean.reshape(c.n, c.c), rstd.reshape(c.n, c.c), w, c.n, c.c, c.hw, c.c,
                                                               [True, True, True])
    else:
        rm, rv = mean.reshape(-1), (1.0 / rstd.reshape(-1) ** 2 - eps)
        dx, dg, db = torch.ops.aten.native_batch_norm_backward(dz, x, w, rm, rv, mean.reshape(-1), rstd.reshape(-1), c.kind == 0, eps,
                                                               [True, True, True])
    r = NC.bwd_on(o["x"], o["y"], o["gy"], o["mean"], o["rstd"], o["gamma"], c.kind, c.act, slope)
    assert _nerr(r["dx"], dx.numpy(), NC.dx_scale(c, o["gamma"], o["rstd"], r)) <= 1e-12
    sabs = float(np.abs(r["dz"]).sum((0, 2, 3)).max())
    assert _nerr(r["dbeta"], db.numpy(), sabs if c.m == 1 else 0.0) <= 1e-12
    assert _nerr(r["dgamma"], dg.numpy(), sabs if (c.m == 1 or c.hw <= 2) else 0.0) <= 1e-12
    wants = {d.name: d.want for d in NC.define(c)}          # and define() hands the GPU sweep exactly these arrays
    assert np.array_equal(wants["dx"], r["dx"]) and (not c.dgamma or np.array_equal(wants["dgamma"], r["dgamma"]))


@pytest.mark.parametrize("act", range(5))
def test_activation_alone_equals_torch(act):
    for c in CASES:
        if c.ep != "act_bwd" or c.act != act or c.count == 0:
            continue
        o = NC.operands(c)
        slope = c.scalars()[2]
        x = _t(o["x"], True)
        y = _torch_act(act, slope)(x)
        want = NC.act_fwd(o["x"], act, slope)
        if act in (0, 1, 4):
            assert np.array_equal(want, y.detach().numpy())
        assert _nerr(want, y.detach().numpy()) <= 1e-12
        y.backward(_t(o["gy"]))
        assert _nerr(o["gy"] * NC.act_dydz(want, act, slope), x.grad.numpy()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------ oracle, golden
@pytest.mark.parametrize("c", [c for c in NORM if c.ep == "norm_bwd" and c.gamma and c.slope == 0.2 and not c.plant and c.m > 1], ids=lambda c: c.id)
def test_definition_agrees_with_the_numpy_oracle(c):
    """oracle.fusion_oracle.norm_act_fwd / _bwd compute in float32 past the statistics: agreement to that precision"""
    o = NC.operands(c)
    eps, mom, slope = c.scalars()
    kind, act = ("bn", "bn_eval", "gn")[c.kind], (None, "relu", "leaky", "tanh", "relu6")[c.act]
    x32, g32 = o["x"].astype(np.float32), o["gamma"].astype(np.float32)
    b32 = o["beta"].astype(np.float32) if o["beta"] is not None else np.zeros(c.c, np.float32)
    running = [a.astype(np.float32) for a in o["running"]] if o["running"] is not None else None
    y, cache = O.norm_act_fwd(x32, g32, b32, kind, act, eps, running, mom)
    f = NC.fwd_on(o["x"], o["gamma"], o["beta"], c.kind, c.act, eps, slope, o["running"], mom)
    assert _nerr(f["y"], y) <= 2e-5
    if c.kind == 0 and running is not None:
        assert _nerr(f["running_mean"], running[0]) <= 1e-6 and _nerr(f["running_var"], running[1]) <= 1e-6
    gy32 = o["gy"].astype(np.float32)
    dx, dg, db = O.norm_act_bwd(cache, y, gy32, g32)
    r = NC.bwd_on(o["x"], y.astype(np.float64), o["gy"], f["mean"], f["rstd"], o["gamma"], c.kind, c.act, slope)
    assert _nerr(r["dx"], dx, NC.dx_scale(c, o["gamma"], f["rstd"], r)) <= 2e-5 and _nerr(r["dgamma"], dg) <= 2e-5 and _nerr(r["dbeta"], db) <= 2e-5


@pytest.mark.parametrize("case", F13_CASES, ids=[c[0] for c in F13_CASES])
def test_definition_reproduces_the_recorded_reference_arrays(case):
    """tests/golden/f13_n4_norm.npz holds what the reference's ConvLayer(norm, act) gave in float32: the convolution in front comes from the
    numpy oracle, the norm + activation and its gradients from the definitions here"""
    name, cin, cout, k, stride, transposed, norm, act, train, N, H, W = case
    g = np.load(GOLDEN)
    P = f13_params(case)
    w, b = P["layers.0.weight"], P["layers.0.bias"]
    x = O.closed_form_signed((N, cin, H, W), 0.5, 1.0)
    z = O.conv_transpose2d_fwd(x, w, b, stride, k // 2, 1, False) if transposed else O.conv2d_general_fwd(x, w, b, stride, k // 2, True, False)
    z = z.astype(np.float64)
    a = {None: 0, "relu": 1, "leaky": 2, "tanh": 3}[act]
    slope = float(np.float32(0.2))
    if norm is None:
        y = NC.act_fwd(z, a, slope)
        assert _nerr(y, g[name + "_y"]) <= 3e-6
        return
    kind = 2 if norm == "gn" else (0 if train else 1)
    gamma, beta = P["layers.1.weight"].astype(np.float64), P["layers.1.bias"].astype(np.float64)
    running = (P["layers.1.running_mean"].astype(np.float64), P["layers.1.running_var"].astype(np.float64)) if norm == "bn" else None
    f = NC.fwd_on(z, gamma, beta, kind, a, 1e-5, slope, running, 0.1)
    assert _nerr(f["y"], g[name + "_y"]) <= 3e-6
    gy = O.closed_form_signed(f["y"].shape, 1.5, 1.0).astype(np.float64)
    r = NC.bwd_on(z, f["y"], gy, f["mean"], f["rstd"], gamma, kind, a, slope)
    assert _nerr(r["dgamma"], g[name + "_dp_layers.1.weight"]) <= 3e-6 and _nerr(r["dbeta"], g[name + "_dp_layers.1.bias"]) <= 3e-6
    if norm == "bn" and train:
        assert _nerr(f["running_mean"], g[name + "_buf_layers.1.running_mean"]) <= 3e-6
        assert _nerr(f["running_var"], g[name + "_buf_layers.1.running_var"]) <= 3e-6
    # dx of the norm, carried through the oracle's convolution backward to the recorded input gradient
    dz = r["dx"].astype(np.float32)
    zz = z.astype(np.float32)
    dx = (O.conv_transpose2d_bwd(x, w, zz, dz, stride, k // 2, 1, False) if transposed else O.conv2d_general_bwd(x, w, zz, dz, stride, k // 2, True, False))[0]
    assert np.abs(dx - g[name + "_dx"]).max() <= 3e-6 * max(1.0, np.abs(g[name + "_dx"]).max())


# ------------------------------------------------------------------------------------------------------------------------------ the table
def test_the_table_covers_what_it_claims():
    assert {c.ep for c in CASES} == set(NC.EPS)
    for ep in ("norm_fwd", "norm_bwd"):
        cs = [c for c in CASES if c.ep == ep]
        assert {(c.kind, c.act) for c in cs} == {(k, a) for k in range(3) for a in range(5)}, ep
        assert {c.hw for c in cs} == set(NC.HW) == {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000}, ep
        assert {c.c for c in cs} == set(NC.CHANNELS) == {1, 3, 256, 257} and {c.n for c in cs} == {1, 2, 3}, ep
        assert all(c.hw <= 65 for c in cs if c.c == 257)
        assert {c.eps for c in cs} == set(NC.EPSILONS) and {c.slope for c in cs if c.act == 2} == set(NC.SLOPES), ep
        for kind in (0, 2):
            assert any(c.plant == "const" and c.kind == kind and c.eps == e for c in cs for e in NC.EPSILONS), (ep, kind)
        assert any(c.kind == 0 and c.m == 1 for c in cs) and any(c.kind == 2 and c.m == 1 and c.n > 1 for c in cs), ep
        assert any(c.offset for c in cs) and any(not c.offset for c in cs)
    fw = [c for c in CASES if c.ep == "norm_fwd"]
    assert sum(NC.gn_given_running(c) for c in fw) >= 3 and any(c.kind == 2 and not NC.gn_given_running(c) for c in fw)
    assert all(NC.operands(c)["running"] is not None for c in fw if NC.gn_given_running(c))
    for kind in range(3):
        assert {(c.gamma, c.beta) for c in fw if c.kind == kind} == {(True, True), (False, False), (False, True), (True, False)}, kind
    assert {c.momentum for c in fw if c.kind == 0 and c.running} == set(NC.MOMENTA) == {0.1, 1.0, 0.0}
    assert {c.momentum for c in fw if c.kind == 0 and not c.running} == set(NC.MOMENTA)
    assert sum(c.plant == "illcond" for c in fw) == 2
    bw = [c for c in CASES if c.ep == "norm_bwd"]
    for kind in range(3):
        assert {(c.gamma, c.dgamma, c.dbeta) for c in bw if c.kind == kind} >= {(False, True, True), (True, False, True), (True, True, False), (False, False, False)}
        assert {c.act for c in bw if c.kind == kind and c.plant == "ties"} == {1, 2, 3, 4}, kind
    for ep in ("staged_fwd", "staged_bwd"):
        cs = [c for c in CASES if c.ep == ep]
        assert {c.act for c in cs} == set(range(5)) and all(c.n == sum(NC.RANKS) == 3 and c.kind == 0 for c in cs) and NC.RANKS == (1, 2)
        assert {257, 1000} <= {c.hw for c in cs} and {1, 257} <= {c.c for c in cs} and any(not c.gamma for c in cs)
        assert any(c.offset for c in cs)
    assert any(c.ep == "staged_fwd" and not c.running for c in CASES) and any(c.ep == "staged_bwd" and not c.dgamma and c.dbeta for c in CASES)
    for ep in ("act_fwd", "act_bwd"):
        assert {(c.act, c.count) for c in CASES if c.ep == ep} == {(a, n) for a in range(5) for n in NC.COUNTS}
        assert NC.COUNTS == (0, 1, 255, 256, 257, 1000) and any(c.offset for c in CASES if c.ep == ep)


def test_planted_values_are_in_the_stored_operands():
    seen = {1: 0, 2: 0, 3: 0, 4: 0}
    for c in CASES:
        o = NC.operands(c)
        if c.plant == "ties":
            counts = NC.tie_counts(o["y"], c.act)
            assert set(counts) == {repr(v) for v in NC.TIES[c.act]} and all(n >= 2 for n in counts.values()), (c.id, counts)
            tied = np.isin(o["y"], NC.TIES[c.act])
            assert (np.abs(o["gy"][tied]) >= 0.5).sum() >= 6, c.id          # each with a gradient that shows
            seen[c.act] += 1
        if c.plant == "const":
            f = NC.fwd_on(o["x"], o["gamma"], o["beta"], c.kind, c.act, *c.scalars()[::2], o["running"], c.scalars()[1])
            eps = c.scalars()[0]
            assert (f["var"] == 0).sum() >= 1 and np.isclose(f["rstd"][f["var"] == 0], 1 / np.sqrt(eps), rtol=1e-15).all(), c.id
            assert (o["x"][0, 1] == o["x"][0, 1, 0, 0]).all() and o["x"][0, 1, 0, 0] != 0
            if not c.fwd:
                assert np.isclose(o["rstd"].reshape(-1, c.c)[0, 1], 1 / np.sqrt(eps), rtol=1e-7)
        if c.plant == "illcond":
            ax = (2, 3) if c.kind == 2 else (0, 2, 3)
            ratio = np.abs(o["x"].mean(ax)) / o["x"].std(ax)
            assert (ratio > 700).all() and (ratio < 1500).all(), (c.id, ratio)
    assert all(n >= 4 for n in seen.values()), seen
    # -0.0 really is stored as -0.0
    c = next(c for c in CASES if c.ep == "norm_bwd" and c.plant == "ties" and c.act == 1)
    y = NC.operands(c)["y"]
    assert (np.signbit(y) & (y == 0)).sum() >= 2 and (~np.signbit(y) & (y == 0)).sum() >= 2


def test_m_equals_one_is_defined_as_the_header_says():
    for c in CASES:
        if c.ep not in ("norm_fwd", "norm_bwd") or c.m != 1 or c.kind == 1:
            continue
        o = NC.operands(c)
        eps, mom, slope = c.scalars()
        outs = {d.name: d.want for d in NC.define(c)}
        if c.fwd:
            beta = np.broadcast_to(o["beta"].reshape(1, c.c, 1, 1), c.shape)
            assert np.array_equal(outs["y"], NC.act_fwd(beta, c.act, slope))
            assert np.allclose(outs["stats"][:, 1], 1 / np.sqrt(eps), rtol=1e-15) and np.array_equal(outs["stats"][:, 0], o["x"].reshape(-1))
            if c.kind == 0:
                assert np.array_equal(outs["running_var"], (1 - mom) * o["running"][1])          # the biased value, 0: no m / (m - 1)
        else:
            assert not outs["dx"].any() and outs["dbeta"].any()


# ------------------------------------------------------------------------------------------------------------------------------ bounds, mutations
def test_every_case_is_alive_and_no_bound_is_vacuous():
    for c in CASES:
        outs = NC.define(c)
        assert set(c.mutations()) <= set(NC.MUTATIONS)
        alive = False
        for o in outs:
            assert o.want.shape == np.shape(o.bound) and np.isfinite(o.want).all() and np.isfinite(o.bound).all() and (np.asarray(o.bound) >= 0).all(), (c.id, o.name)
            if o.exact:
                assert not np.asarray(o.bound).any()
            if not o.want.size:
                continue
            alive |= bool(o.want.any())
            scale = max(float(np.abs(o.want).max()), o.scale)
            if c.plant != "illcond":
                assert float(np.max(o.bound)) <= 1e-4 * scale, (c.id, o.name, float(np.max(o.bound)), scale)
        assert alive or (c.ep.startswith("act") and c.count <= 1), c.id
    assert NC.TANH_ULP == 2 * NC.TANH_ULP_MEASURED


def _separation(c, mut, true):
    worst = 0.0
    for o, m in zip(true, NC.define(c, mut)):
        if o.want.size:
            d = np.abs(m.want - o.want)
            worst = max(worst, float(np.max(d / np.maximum(o.bound, 1e-300) * (d > 0))))
    return worst


@pytest.mark.parametrize("mut", NC.MUTATIONS)
def test_mutation_is_separated_by_more_than_ten_bounds(mut):
    """the wrong definition differs from the true one by more than ten times the case's own bound on the cases that list it: the GPU sweep
    fails if the kernel, or the definition, is changed into it"""
    cases = [c for c in CASES if mut in c.mutations()]
    assert len(cases) >= 2, f"{mut}: no case can show it"
    missed = [c.id for c in cases if _separation(c, mut, NC.define(c)) <= 10]
    print(f"{mut}: separated on {len(cases) - len(missed)} of {len(cases)} cases; not on {missed}")
    assert len(missed) < len(cases) and len(missed) <= 0.25 * len(cases), (mut, missed)
