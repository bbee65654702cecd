"""tests/optim_cases.py without a GPU: its fp64 definition of mmif_clip_adam_step against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in
float64 over one, two and three consecutive steps (the NaN and +inf gradients included) and against oracle.fusion_oracle.clip_grad_norm /
adam_step; the case table shown to hold every axis value it claims, no clip quotient near enough to 1 for fp32 rounding to flip the branch,
no bound beyond 1e-4 of its output's scale, and every listed wrong definition shown to differ from the true one by more than ten bounds."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import optim_cases as OC
from optim_cases import CASES
from oracle import fusion_oracle as O

SMALL = [c for c in CASES if c.numel <= 262145]


def _same(a, b, tol=1e-12):
    """non-finite values in the same places, the finite ones to `tol` of the largest"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape
    if not (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))):
        return False
    fin = np.isfinite(a)
    return not fin.any() or float(np.abs(a[fin] - b[fin]).max()) <= tol * max(float(np.abs(b[fin]).max()), 1e-300)


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_definition_equals_torch_clip_grad_norm_and_adam(c):
    """three consecutive steps from the case's state and step count, fresh gradients of the case's kind at every step"""
    o = OC.operands(c)
    p = torch.nn.Parameter(torch.from_numpy(o["p"].copy()))
    opt = torch.optim.Adam([p], lr=OC.LR, betas=(OC.B1, OC.B2), eps=OC.ADAM_EPS)
    opt.state[p] = {"step": torch.tensor(float(c.step - 1)), "exp_avg": torch.from_numpy(o["m"].copy()), "exp_avg_sq": torch.from_numpy(o["v"].copy())}
    st = dict(p=o["p"], m=o["m"], v=o["v"])
    rng = np.random.default_rng(c.numel)
    for k in range(3):
        g = o["g"] if k == 0 else OC.f32(o["g"] * rng.uniform(0.5, 1.5, c.numel))
        p.grad = torch.from_numpy(g * c.grad_scale)
        if c.max_norm > 0:
            norm = torch.nn.utils.clip_grad_norm_([p], c.max_norm)
        else:
            norm = p.grad.norm()
        opt.step()
        r = OC.adam_on(st["p"], g, st["m"], st["v"], c.step + k, c.max_norm, c.grad_scale)
        assert _same(r["norm"], norm.item()), (k, r["norm"], norm.item())
        assert _same(r["p"], p.detach().numpy()) and _same(r["m"], opt.state[p]["exp_avg"].numpy()) and _same(r["v"], opt.state[p]["exp_avg_sq"].numpy()), k
        st = dict(p=r["p"], m=r["m"], v=r["v"])
    if c.special == "nan" and c.max_norm > 0:
        assert np.isnan(st["p"]).all() and np.isnan(st["m"]).all()          # the whole state is poisoned, as in torch
    if c.special == "nan" and c.max_norm <= 0:
        assert np.isnan(st["p"]).sum() == 1
    if c.special == "inf":
        first = OC.adam_on(o["p"], o["g"], o["m"], o["v"], c.step, c.max_norm, c.grad_scale)
        assert first["coef"] == 0 and np.isnan(first["p"]).sum() == 1 and np.isinf(first["norm"])


@pytest.mark.parametrize("c", [c for c in SMALL if not c.special and c.clip != "off"], ids=lambda c: c.id)
def test_definition_agrees_with_the_numpy_oracle(c):
    """oracle.fusion_oracle.clip_grad_norm + adam_step work on float32 arrays: agreement to that precision"""
    o = OC.operands(c)
    G = OrderedDict(w=(o["g"] * c.grad_scale).astype(np.float32))
    P = OrderedDict(w=o["p"].astype(np.float32))
    st = O.AdamState(P)
    st.m["w"], st.v["w"], st.t = o["m"].astype(np.float32), o["v"].astype(np.float32), c.step - 1
    norm = O.clip_grad_norm(G, c.max_norm)
    O.adam_step(P, G, st, lr=OC.LR, betas=(OC.B1, OC.B2), eps=OC.ADAM_EPS)
    r = OC.adam_on(o["p"], o["g"], o["m"], o["v"], c.step, c.max_norm, c.grad_scale)
    assert abs(norm - r["norm"]) <= 1e-6 * r["norm"]
    assert _same(st.m["w"], r["m"], 1e-5) and _same(st.v["w"], r["v"], 1e-5)
    assert float(np.abs(P["w"] - r["p"]).max()) <= 1e-5 * float(np.abs(r["upd"]).max()) + 2 ** -24 * float(np.abs(r["p"]).max())


def test_the_table_covers_what_it_claims():
    assert OC.NUMELS == (1, 255, 256, 257, 262143, 262144, 262145, 3 * 262144 + 17) and OC.ADAM_PARTIALS * 256 == 262144
    for numel in OC.NUMELS:
        cs = [c for c in CASES if c.numel == numel and not c.special]
        assert {c.clip for c in cs} == set(OC.CLIPS), numel
    assert any(c.blocks == 1024 and c.numel > 262144 and c.Ks() > Case_small_Ks() for c in CASES)
    plain = [c for c in CASES if not c.special]
    assert {c.step for c in plain} == {1, 2, 1000} and {c.grad_scale for c in plain} == {1.0, 0.5, 0.125}
    for clip in OC.CLIPS:
        assert {c.grad_scale for c in plain if c.clip == clip} == {1.0, 0.5, 0.125}, clip
        assert any(c.moments for c in plain if c.clip == clip)
    assert any(not c.moments for c in plain) and any(not c.norm_out for c in plain) and any(c.offset for c in plain) and any(not c.offset for c in plain)
    assert {c.special for c in CASES if c.special} == set(OC.SPECIALS)
    assert any(c.special == sp and c.numel > 262144 for c in CASES for sp in OC.SPECIALS)
    for c in plain:
        o = OC.operands(c)
        r = OC.adam_on(o["p"], o["g"], o["m"], o["v"], c.step, c.max_norm, c.grad_scale)
        assert abs(r["norm"] / c.target_norm - 1) < 1e-6, c.id
        if c.clip == "off":
            assert c.max_norm == 0 and r["coef"] == 1
            continue
        # the quotient is clearly on one side of 1: at least a hundred times the fp32 error of the norm away
        assert abs(r["q"] - 1) > 100 * (c.Ks() / 2 + 6) * OC.U, (c.id, r["q"])
        assert (r["coef"] < 1) == (c.clip in ("above", "near_hi", "tiny")), c.id
        if c.clip.startswith("near"):
            assert abs(r["norm"] / 5.0 - 1) < 1e-3
        if c.clip == "tiny":
            assert abs(c.max_norm - 1e-5) < 1e-11 and 0.85 < r["coef"] < 0.95          # 1e-5 / (1e-5 + 1e-6): the + 1e-6 shows
    for c in CASES:
        o = OC.operands(c)
        if c.special == "zero":
            assert not o["g"].any() and not o["m"].any()
            assert all(np.array_equal(d.want, o[k]) and not d.bound.any() for d, k in zip(OC.define(c)[:3], ("p", "m", "v")))
        if c.special == "stretch":
            s = OC.stretch(c)
            outs = OC.define(c)
            assert not o["g"][s].any() and not o["m"][s].any() and not o["v"][s].any() and o["g"].any()
            assert np.array_equal(outs[0].want[s], o["p"][s]) and not outs[0].bound[s].any()          # bit-identical: optim.py's unused parameters
            assert (outs[0].want != o["p"]).sum() == c.numel - (s.stop - s.start)
        if c.special in ("nan", "inf"):
            assert (~np.isfinite(o["g"])).sum() == 1


def Case_small_Ks():
    return OC.Case(256).Ks()


def test_bounds_are_finite_and_not_vacuous():
    for c in CASES:
        for d in OC.define(c):
            fin = np.isfinite(d.want)
            assert d.want.shape == d.bound.shape and np.isfinite(d.bound).all() and (d.bound >= 0).all() and not d.bound[~fin].any(), (c.id, d.name)
            if fin.any() and np.abs(d.want[fin]).max() > 0:
                assert float(d.bound[fin].max()) <= 1e-4 * float(np.abs(d.want[fin]).max()), (c.id, d.name)
    assert OC.Case(3 * 262144 + 17).Ks() == 4 + 10 + 4 + 10 and OC.Case(1).Ks() == 1 + 10 + 1 + 10


def _separation(c, mut, true):
    worst = 0.0
    for o, m in zip(true, OC.define(c, mut)):
        if not np.array_equal(np.isfinite(o.want), np.isfinite(m.want)):
            return np.inf
        fin = np.isfinite(o.want)
        d = np.abs(m.want[fin] - o.want[fin])
        if d.size:
            worst = max(worst, float(np.max(d / np.maximum(o.bound[fin], 1e-300) * (d > 0))))
    return worst


@pytest.mark.parametrize("mut", OC.MUTATIONS)
def test_mutation_is_separated_by_more_than_ten_bounds(mut):
    cases = [c for c in CASES if mut in c.mutations()]
    assert len(cases) >= 3, f"{mut}: no case can show it"
    missed = [c.id for c in cases if _separation(c, mut, OC.define(c)) <= 10]
    print(f"{mut}: separated on {len(cases) - len(missed)} of {len(cases)} cases; not on {missed}")
    assert len(missed) < len(cases) and len(missed) <= 0.25 * len(cases), (mut, missed)
