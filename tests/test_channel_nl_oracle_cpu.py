"""The oracles of the channel non-local kernels and of the fusion join, checked on the CPU before any kernel is held to them
(tests/channel_nl_cases.py; the GPU side is tests/test_gpu_channel_nl_sweep.py and tests/test_gpu_channel_nl.py):

  * the float64 restatement equals golden F26 (the reference's own code, float64 autograd) to 1e-12;
  * the term-wise pieces sum to the restatement to 1e-13;
  * every applicable mutant lies at least 20 sweep tolerances from the truth, so a kernel inside the tolerance is none of them;
  * in every non-tie case the two extremum gaps (transpose twin ignored) are >= 1e-4 of hi - lo and >= 100 float32 energy errors, so that the
    kernels' float32 energies cannot move the argmin / argmax, and no case has to skip its d check;
  * the mirror of the kernels' tile geometry shows every 16-channel tile count at its lowest and highest C, and a case past the chunk cap;
  * the join's float64 definition, clamp rule included, equals torch float64 autograd on planted clamp-regime elements.
"""
import numpy as np
import pytest
import torch

import channel_nl_cases as CC


def rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", list(CC.CASES))
def test_restatement_matches_the_golden(name):
    gold = np.load(CC.F26)
    x, g = CC.inputs(name), CC.upstream(name)
    ref = CC.channel_f64(x, g)
    idx = CC.sample_index(x.size)
    ey, ed = rel(ref["y"].reshape(-1)[idx], gold[f"{name}|y"]), rel(ref["dx"].reshape(-1)[idx], gold[f"{name}|dx"])
    print(f"F26 {name}: restatement vs reference float64  y {ey:.2e}  dx {ed:.2e}")
    assert ey <= 1e-12 and ed <= 1e-12
    assert abs(ref["lo"] - gold[f"{name}|lo"]) <= 1e-12 * abs(ref["hi"]) and abs(ref["hi"] - gold[f"{name}|hi"]) <= 1e-12 * abs(ref["hi"])


@pytest.mark.parametrize("name", list(CC.CASES))
def test_model_cases_have_no_near_tie(name):
    t = CC.channel_terms_f64(CC.inputs(name), CC.upstream(name))
    assert t["gap_lo"] >= CC.MIN_GAP and t["gap_hi"] >= CC.MIN_GAP, (name, t["gap_lo"], t["gap_hi"])


@pytest.mark.parametrize("c", CC.SWEEP, ids=lambda c: c.name)
def test_pieces_sum_to_the_restatement(c):
    x, g, ref, _ = CC.reference(c.name)
    full = CC.channel_f64(x, g)
    ey = rel(ref["a"] + x.astype(np.float64), full["y"])
    ed = rel(g.astype(np.float64) + ref["tA"] + ref["tB"] + ref["tR"], full["dx"])
    print(f"{c.name}: pieces vs restatement  y {ey:.2e}  dx {ed:.2e}")
    assert ey <= 1e-13 and ed <= 1e-13
    assert np.array_equal(ref["e"], ref["e"].transpose(0, 2, 1))
    assert c.kc == CC.kc_for(c.shape[1])


@pytest.mark.parametrize("c", CC.SWEEP, ids=lambda c: c.name)
def test_mutants_lie_far_outside_the_tolerance(c):
    _, _, ref, dist = CC.reference(c.name)
    tol = CC.tolerances(c.name)
    applicable = {"no_tA"} if c.shape[1] == 1 else set(CC.MUTANTS_A + CC.MUTANTS_D)
    assert set(dist) == applicable
    for k, v in sorted(dist.items()):
        q = "a" if k in CC.MUTANTS_A else "d"
        margin = v / tol[q] if tol[q] > 0 else float("inf")
        print(f"{c.name}: mutant {k} at {v:.2e} = {margin:.0f} tolerances of {q} ({tol[q]:.2e})")
        assert v >= CC.MUTANT_MARGIN * tol[q], (c.name, k, v, tol[q])


@pytest.mark.parametrize("c", CC.SWEEP, ids=lambda c: c.name)
def test_extrema_are_safe_from_float32_energies(c):
    _, _, ref, _ = CC.reference(c.name)
    f = CC.float32_errors(c.name)          # (asserts that both float32 evaluations find the extrema where float64 does)
    print(f"{c.name}: gaps {ref['gap_lo']:.2e} {ref['gap_hi']:.2e}  float32 energy error {f['scalars']:.2e}  yardstick {f}")
    if c.tie == "zero":
        assert ref["lo"] == 0.0 and ref["pos_lo"] == (0, 0, CC.ZERO_CHANNEL)
        assert ref["gap_lo"] == 0.0
        assert ref["gap_hi"] >= CC.MIN_GAP and ref["gap_hi"] >= CC.GAP_OVER_ERR * f["scalars"]
    elif c.tie == "dup":
        assert ref["gap_lo"] == 0.0 and ref["gap_hi"] == 0.0 and ref["pos_lo"][0] == 0 and ref["pos_hi"][0] == 0
        assert ref["pos_lo2"] == (1,) + ref["pos_lo"][1:] and ref["pos_hi2"] == (1,) + ref["pos_hi"][1:]
    else:
        for k in ("gap_lo", "gap_hi"):
            assert ref[k] >= CC.MIN_GAP and ref[k] >= CC.GAP_OVER_ERR * f["scalars"], (c.name, k, ref[k], f["scalars"])


def test_sweep_covers_the_tile_geometry():
    cs = {c.shape[1] for c in CC.SWEEP}
    for kc in CC.KC_SET:
        lo, hi = CC.kc_range(kc)
        assert CC.kc_for(lo) == kc and CC.kc_for(hi) == kc and (lo == 1 or CC.kc_for(lo - 1) != kc) and (hi == 256 or CC.kc_for(hi + 1) != kc)
        assert lo in cs and hi in cs, (kc, lo, hi)
    ns = {c.shape[2] * c.shape[3] for c in CC.SWEEP}
    assert {1, 3, 5, 63, 64, 65} <= ns
    over = CC.BY_NAME["chunks_over_cap"]
    tiles, chunks, tpc = CC.chunks_for(over.shape[0], over.shape[2] * over.shape[3])
    assert tiles > CC.chunk_cap(over.shape[0]) and tpc >= 2 and chunks <= CC.chunk_cap(over.shape[0]) and chunks * tpc >= tiles > (chunks - 1) * tpc
    tiles, chunks, tpc = CC.chunks_for(2, 33 * 65)
    assert (tiles, chunks, tpc) == (34, 34, 1)
    assert any(c.shape[0] * c.shape[1] == 2 for c in CC.SWEEP) and any(c.shape[1] == 256 and c.shape[2] * c.shape[3] == 1 for c in CC.SWEEP)
    assert any(c.shape[1] > 128 for c in CC.SWEEP)     # more row tiles than one gram block has waves


def test_scaled_cases_put_the_extrema_into_different_samples():
    hi_samples = {CC.reference(n)[2]["pos_hi"][0] for n in ("scale_312", "scale_123")}
    assert hi_samples == {0, 2}


# ------------------------------------------------------------------------------------------------------------------------------ the join
def _torch_join(mode, arrs, g, eps):
    t1, t2, s1, s2, c1, c2 = (torch.from_numpy(a.copy()).requires_grad_(True) for a in arrs)

    def wf(x1, x2, w1, w2):                       # reference core/fusion.py:32-35
        w = w1 / (w1 + w2).clamp_(min=eps)
        return w * x1 + (1.0 - w) * x2

    fs, fc = wf(t1, t2, s1, s2), wf(t1, t2, c1, c2)
    out = {"sa": lambda: fs, "ca": lambda: fc, "sca": lambda: (fs + fc) / 2.0, "wavg": lambda: wf(fs, fc, fs, fc)}[mode]()
    (out * torch.from_numpy(g)).sum().backward()
    grads = [t.grad.numpy() if t.grad is not None else None for t in (t1, t2, s1, s2, c1, c2)]
    return out.detach().numpy(), grads


@pytest.mark.parametrize("mode", CC.FUSION_MODES)
def test_join_definition_equals_torch_float64_autograd(mode):
    eps = 1e-7
    arrs = list(CC.join_inputs(300, 4401, np.float64, eps))     # planted at the float64 clamp: a + b negative, zero, exactly eps, just above it
    g = arrs.pop()
    assert arrs[2][2] + arrs[3][2] == eps and arrs[2][3] + arrs[3][3] > eps
    out_t, grads_t = _torch_join(mode, arrs, g, eps)
    out, grads = CC.join_def(mode, *arrs, g, dt=np.float64, eps=eps)
    used = {"sa": (0, 1, 2, 3), "ca": (0, 1, 4, 5), "sca": range(6), "wavg": range(6)}[mode]
    assert np.allclose(out, out_t, rtol=1e-13, atol=0)
    for k in range(6):
        if k in used:
            assert np.allclose(grads[k], grads_t[k], rtol=1e-12, atol=1e-300), (mode, k, np.abs(grads[k] - grads_t[k]).max())
        else:
            assert grads[k] is None
    # the clamp rule itself, on the planted elements of the spatial pair: gradient reaches b only through a + b, i.e. where a + b >= eps
    if mode in ("sa", "sca", "wavg"):
        ds2 = grads[3]
        assert ds2[0] == 0.0 and ds2[1] == 0.0 and ds2[2] != 0.0 and ds2[3] != 0.0
        assert grads_t[3][0] == 0.0 and grads_t[3][1] == 0.0 and grads_t[3][2] != 0.0 and grads_t[3][3] != 0.0


def test_join_float32_clamp_sits_at_float32_eps():
    """float32 torch clamps at float32(1e-7): the element planted exactly there passes gradient, as in the kernels' rule"""
    arrs = list(CC.join_inputs(8, 4402))
    g = arrs.pop()
    _, grads_t = _torch_join("sa", arrs, g, 1e-7)
    _, grads = CC.join_def("sa", *arrs, g, dt=np.float32)
    assert float(arrs[2][2]) + float(arrs[3][2]) == float(CC.EPS32)
    for k in (2, 3):
        assert np.array_equal(grads[k][:4] != 0, grads_t[k][:4] != 0), (k, grads[k][:4], grads_t[k][:4])
    assert grads[3][0] == 0.0 and grads[3][1] == 0.0 and grads[3][2] != 0.0 and grads[3][3] != 0.0


def test_fusion_golden_is_the_join_of_the_restated_maps():
    """the whole layer in float64: both 'nl' maps restated, joined by join_def, equals the reference's attention_fusion to 1e-12 (values only:
    the gradients through the maps are held on the GPU against the fixture itself)"""
    from nonlocal_cases import nonlocal_f64
    gold = np.load(CC.F26)
    t1, t2, _ = CC.fusion_inputs()
    s1, s2 = nonlocal_f64(t1)["y"], nonlocal_f64(t2)["y"]
    c1, c2 = CC.channel_f64(t1)["y"], CC.channel_f64(t2)["y"]
    idx = CC.sample_index(t1.size)
    for mode in CC.FUSION_MODES:
        sp, ch = mode != "ca", mode != "sa"
        out = CC.join_def(mode, t1, t2, s1 if sp else None, s2 if sp else None, c1 if ch else None, c2 if ch else None, eps=1e-7)
        e = rel(out.reshape(-1)[idx], gold[f"fusion_{mode}|out"])
        print(f"F26 fusion {mode}: join of the restated maps vs reference float64 {e:.2e}")
        assert e <= 1e-12


def test_abi_declares_the_new_entry_points():
    """header, ctypes table and library agree on the five entry points (the library loads without a GPU)"""
    import os
    from mmif import _lib
    hdr = open(os.path.join(os.path.dirname(CC.HERE), "include", "mmif.h")).read()
    for name in ("mmif_nonlocal_channel_workspace", "mmif_nonlocal_channel_fwd", "mmif_nonlocal_channel_bwd", "mmif_fuse_join_fwd", "mmif_fuse_join_bwd"):
        assert name in _lib.SIGNATURES and f" {name}(" in hdr and getattr(_lib.lib, name) is not None, name
    assert _lib.lib.mmif_nonlocal_channel_workspace(1, 1, 4, 4) == 0 and _lib.lib.mmif_nonlocal_channel_workspace(2, 112, 16, 24) > 0
    assert _lib.lib.mmif_fuse_join_fwd(None, None, None, None, None, None, None, 2, 8, None) == -1      # refused before any launch
