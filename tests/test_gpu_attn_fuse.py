"""attention_fusion, spatial_fusion and channel_fusion on the fused kernels of csrc/attn_fuse.hip, through the public functions with autograd:

  * $MMIF_ATTN_FUSE=hip against =torch (the tensor-level composition) on the same tie-free tensors: each route lies within the tolerance of
    tests/attn_fuse_cases.py (8 x the float32 numpy evaluation's error of that case, combination and term) of the float64 definition;
  * golden F27 (the reference's own code in float64, planted ties included) through the public functions;
  * UNFusion, SEDRFuse and MyFusion(fusion_mode='wavg') forward + backward take the new route (spied on the mmif.tensor wrappers).

The three combinations that the blocked 'l1' / 'avg' kernels (mmif_fuse_attn_*) keep -- 'sa' / 'ca' / 'sca' with the default poolings -- are not
routed here and are left to their own tests.
"""
import numpy as np
import pytest
import torch

import attn_fuse_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _blocked_route(combo):
    mode, sm, cm = combo
    return mode != "wavg" and sm == "l1" and cm == "avg"


def _public(fn, arrs):
    """(out, d1, d2) of a public fusion function on the GPU in float32, gradients of sum(out * g)"""
    t1, t2, g = arrs
    a = torch.from_numpy(np.array(t1)).to(DEV).requires_grad_(True)
    b = torch.from_numpy(np.array(t2)).to(DEV).requires_grad_(True)
    out = fn(a, b)
    (out * torch.from_numpy(np.array(g)).to(DEV)).sum().backward()
    return {"out": out.detach().cpu().numpy(), "d1": a.grad.cpu().numpy(), "d2": b.grad.cpu().numpy()}


def _fusion_fn(combo):
    import core.fusion as CF
    mode, sm, cm = combo
    if sm == AC.SEDR:
        return CF.softmax_l1_fusion
    return lambda a, b: CF.attention_fusion(a, b, mode, sm, cm)


def _spy(monkeypatch):
    from mmif import tensor as T
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = T.attn_fuse_fwd, T.attn_fuse_bwd

    def spy_fwd(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def spy_bwd(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(T, "attn_fuse_fwd", spy_fwd)
    monkeypatch.setattr(T, "attn_fuse_bwd", spy_bwd)
    return calls


@pytest.mark.parametrize("name", ["n3c16_5x13", "n2c3_25x40"])
def test_hip_route_against_the_composition(name, monkeypatch):
    arrs = AC.inputs(name)
    calls = _spy(monkeypatch)
    for combo in AC.COMBOS:
        if _blocked_route(combo):
            continue
        ref, tol = AC.reference(name, combo)
        res = {}
        for impl in ("hip", "torch"):
            monkeypatch.setenv("MMIF_ATTN_FUSE", impl)
            before = dict(calls)
            res[impl] = _public(_fusion_fn(combo), arrs)
            took = (calls["fwd"] - before["fwd"], calls["bwd"] - before["bwd"])
            assert took == ((1, 1) if impl == "hip" else (0, 0)), (combo, impl, took)
            figs = {k: AC.err(res[impl][k], ref[k]) for k in ("out", "d1", "d2")}
            print(f"{name} {combo} {impl}: " + "  ".join(f"{k} {v:.2e} (tol {tol[k]:.1e})" for k, v in figs.items()))
            for k, v in figs.items():
                assert v <= tol[k], (name, combo, impl, k, v, tol[k])


def test_spatial_and_channel_fusion_without_softmax(monkeypatch):
    import core.fusion as CF
    name = "n3c16_5x13"
    arrs = AC.inputs(name)
    calls = _spy(monkeypatch)
    rows = [(("sa", sm, "avg"), (lambda a, b, sm=sm: CF.spatial_fusion(a, b, sm, softmax=False))) for sm in AC.SPATIAL]
    rows += [(("ca", "l1", cm), (lambda a, b, cm=cm: CF.channel_fusion(a, b, cm, softmax=False))) for cm in AC.CHANNEL]
    for combo, fn in rows:
        ref, tol = AC.reference(name, combo)
        for impl in ("hip", "torch"):
            monkeypatch.setenv("MMIF_ATTN_FUSE", impl)
            before = calls["fwd"]
            res = _public(fn, arrs)
            assert calls["fwd"] - before == (1 if impl == "hip" else 0), (combo, impl)
            for k in ("out", "d1", "d2"):
                v = AC.err(res[k], ref[k])
                print(f"{combo} {impl} {k}: {v:.2e} (tol {tol[k]:.1e})")
                assert v <= tol[k], (combo, impl, k, v, tol[k])
    # softmax=True stays a composition
    monkeypatch.setenv("MMIF_ATTN_FUSE", "hip")
    before = calls["fwd"]
    _public(lambda a, b: CF.spatial_fusion(a, b, "l2"), arrs)
    _public(lambda a, b: CF.channel_fusion(a, b, "max"), arrs)
    assert calls["fwd"] == before


def test_invalid_switch_raises(monkeypatch):
    import core.fusion as CF
    monkeypatch.setenv("MMIF_ATTN_FUSE", "triton")
    a = torch.ones(1, 2, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="MMIF_ATTN_FUSE"):
        CF.attention_fusion(a, a, "wavg")


def test_golden_through_the_public_functions(monkeypatch):
    monkeypatch.setenv("MMIF_ATTN_FUSE", "hip")
    gold = np.load(AC.F27)
    arrs = AC.inputs("gold")
    calls = _spy(monkeypatch)
    n = 0
    for combo in AC.COMBOS:
        if _blocked_route(combo):
            continue
        _, tol = AC.reference("gold", combo)
        res = _public(_fusion_fn(combo), arrs)
        n += 1
        for k in ("out", "d1", "d2"):
            v = AC.err(res[k], gold["|".join(combo) + "|" + k])
            print(f"F27 {combo} {k}: {v:.2e} (tol {tol[k]:.1e})")
            assert v <= tol[k], (combo, k, v, tol[k])
    assert calls["fwd"] == n and calls["bwd"] == n


@pytest.mark.parametrize("name,kwargs,levels", [("UNFusion", {}, 4), ("SEDRFuse", {}, 1), ("MyFusion", {"fusion_mode": "wavg"}, None)])
def test_models_take_the_fused_route(name, kwargs, levels, monkeypatch):
    import core.model as M
    monkeypatch.setenv("MMIF_ATTN_FUSE", "hip")
    calls = _spy(monkeypatch)
    torch.manual_seed(7)
    m = getattr(M, name)(**kwargs).to(DEV)
    i1, i2 = torch.rand(1, 1, 32, 32, device=DEV), torch.rand(1, 1, 32, 32, device=DEV)
    out = m(i1, i2)
    out.sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())
    assert any(p.grad is not None and p.grad.abs().max() > 0 for p in m.parameters())
    print(f"{name}: attn_fuse_fwd x {calls['fwd']}, attn_fuse_bwd x {calls['bwd']}")
    assert calls["fwd"] >= 1 and calls["fwd"] == calls["bwd"]
    if levels is not None:
        assert calls["fwd"] == levels
