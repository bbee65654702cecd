"""The definition the kernels of csrc/attn_fuse.hip are held to (tests/attn_fuse_cases.py), checked on the CPU before any kernel meets it
(the GPU side is tests/test_gpu_attn_fuse_sweep.py and tests/test_gpu_attn_fuse.py):

  * the float64 definition equals torch float64 autograd of the literal composition (the reference's ops: norm, max(dim), avg_pool2d, max_pool2d,
    clamp_) to 1e-12 for every one of the 5 x 2 x 4 + SEDRFuse combinations, ties, zero vectors, zero planes and clamp-regime elements included;
  * it equals golden F27, the reference's own code in float64, to 1e-12;
  * every mutant lies at least 20 tolerances from the definition in every case built for it; no case is excluded;
  * the float32 evaluation of the signed case is well conditioned for the combinations the table lists;
  * the case table covers the kernels' geometry;
  * the C ABI has the entry points and refuses bad arguments before any launch.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_fuse_cases as AC

EPS64 = 1e-7


def _torch_eval(t1, t2, g, mode, sm, cm):
    """the reference's composition, literally (core/fusion.py:32-126, core/model.py:271-281), in float64 with autograd"""
    a = torch.from_numpy(np.asarray(t1, np.float64)).requires_grad_(True)
    b = torch.from_numpy(np.asarray(t2, np.float64)).requires_grad_(True)

    def wf(x1, x2, w1, w2):
        w = w1 / (w1 + w2).clamp_(min=EPS64)
        return w * x1 + (1.0 - w) * x2

    def spool(x):
        if sm == "sum":
            return x.sum(dim=1, keepdim=True)
        if sm == "mean":
            return x.mean(dim=1, keepdim=True)
        if sm == "l1":
            return x.norm(p=1, dim=1, keepdim=True)
        if sm == "l2":
            return x.norm(p=2, dim=1, keepdim=True)
        if sm == "linf":
            return x.max(dim=1, keepdim=True)[0]
        tmp = torch.abs(x)
        return (torch.softmax(tmp, dim=1) * tmp).sum(dim=1, keepdim=True)

    def cpool(x):
        k = tuple(x.shape[2:])
        return F.avg_pool2d(x, kernel_size=k) if cm == "avg" else F.max_pool2d(x, kernel_size=k)

    sp, ch = AC.uses(mode)
    fs = wf(a, b, spool(a), spool(b)) if sp else None
    fc = wf(a, b, cpool(a), cpool(b)) if ch else None
    out = {"sa": lambda: fs, "ca": lambda: fc, "sca": lambda: (fs + fc) / 2.0, "wavg": lambda: wf(fs, fc, fs, fc)}[mode]()
    (out * torch.from_numpy(np.asarray(g, np.float64))).sum().backward()
    return out.detach().numpy(), a.grad.numpy(), b.grad.numpy()


def _rel(got, ref):
    top = np.abs(ref).max()
    return float(np.abs(got - ref).max() / top) if top > 0 else float(np.abs(got).max())


TORCH_CASES = ("n1c1_1x1", "n1c3_8x8", "n3c16_5x13", "n2c5_7x9_ties", "eps", "gold")


@pytest.mark.parametrize("name", TORCH_CASES)
def test_definition_equals_torch_float64_autograd(name):
    t1, t2, g = AC.inputs(name)
    worst = 0.0
    for combo in AC.COMBOS:
        ref = AC.evaluate(t1, t2, g, *combo, dt=np.float64, eps=EPS64)
        out, d1, d2 = _torch_eval(t1, t2, g, *combo)
        e = max(_rel(ref["out"], out), _rel(ref["d1"], d1), _rel(ref["d2"], d2))
        worst = max(worst, e)
        assert e <= 1e-12, (name, combo, e)
    print(f"{name}: definition vs torch float64 autograd over {len(AC.COMBOS)} combinations, worst {worst:.2e}")


def test_signed_case_equals_torch_and_is_well_conditioned():
    c = AC.BY_NAME["signed"]
    t1, t2, g = AC.inputs(c.name)
    assert (t1.sum(axis=1) + t2.sum(axis=1) < 0).any() and (t1.sum(axis=1) + t2.sum(axis=1) > 0).any()
    for combo in c.combos:
        ref = AC.evaluate(t1, t2, g, *combo, dt=np.float64, eps=EPS64)
        out, d1, d2 = _torch_eval(t1, t2, g, *combo)
        assert max(_rel(ref["out"], out), _rel(ref["d1"], d1), _rel(ref["d2"], d2)) <= 1e-12, combo
        _, tol = AC.reference(c.name, combo)
        print(f"signed {combo}: tolerances " + "  ".join(f"{k} {v:.1e}" for k, v in tol.items()))
        assert max(tol.values()) <= 1e-4, (combo, tol)        # the float32 evaluation keeps five digits in every element: well conditioned


def test_definition_equals_the_golden():
    gold = np.load(AC.F27)
    t1, t2, g = AC.inputs("gold")
    worst = 0.0
    for combo in AC.COMBOS:
        ref = AC.evaluate(t1, t2, g, *combo, dt=np.float64, eps=EPS64)
        key = "|".join(combo)
        for k in ("out", "d1", "d2"):
            e = _rel(ref[k].reshape(-1), gold[f"{key}|{k}"])
            worst = max(worst, e)
            assert e <= 1e-12, (combo, k, e)
    print(f"F27: definition vs the reference's float64 autograd over {len(AC.COMBOS)} combinations, worst {worst:.2e}")


@pytest.mark.parametrize("mutant", AC.MUTANTS)
def test_mutants_lie_far_outside_the_tolerance(mutant):
    assert set(AC.MUTANT_CASES) == set(AC.MUTANTS)
    rows = AC.MUTANT_CASES[mutant]
    assert rows
    for name, combo in rows:
        m = AC.mutant_margin(name, combo, mutant)
        print(f"mutant {mutant} in {name} {combo}: {m:.0f} tolerances")
        assert m >= AC.MUTANT_MARGIN, (mutant, name, combo, m)


def test_eps_case_sits_on_the_clamp():
    """the planted pools land exactly below / on / above float32(1e-7) in float32 AND float64, for the modes the table claims"""
    t1, t2, g = AC.inputs("eps")
    below, on, above = (np.float32(a) + np.float32(b) for a, b in AC.EPS_PAIRS)
    assert below < AC.EPS32 == on < above
    for dt in (np.float32, np.float64):
        for sm, px in (("sum", 0), ("l1", 0), ("l2", 0), ("linf", 0), ("mean", 3)):
            r = AC.evaluate(t1, t2, g, "sa", sm, "avg", dt=dt)
            got = (r["s1"] + r["s2"])[0, px:px + 3]
            assert got[0] == below and got[1] == on and got[2] == above, (dt, sm, got)
        for cm, b in (("max", 1), ("avg", 2)):
            r = AC.evaluate(t1, t2, g, "ca", "l1", cm, dt=dt)
            got = (r["c1"] + r["c2"])[b, :3]
            assert got[0] == below and got[1] == on and got[2] == above, (dt, cm, got)


def test_table_covers_the_geometry():
    shapes = {c.shape for c in AC.CASES}
    assert {s[0] for s in shapes} >= {1, 2, 3} and {s[1] for s in shapes} >= {1, 2, 3, 16, 17, 257}
    assert {(s[2], s[3]) for s in shapes} >= {(1, 1), (1, 63), (8, 8), (5, 13), (15, 17), (257, 1), (25, 40), (300, 300)}
    tiles = lambda s: -(-(s[2] * s[3]) // AC.TILE)
    p, e = AC.BY_NAME["pool_cap"].shape, AC.BY_NAME["elem_cap"].shape
    assert p[0] * tiles(p) > AC.POOL_GRID_CAP and e[0] * e[1] * tiles(e) > AC.ELEM_GRID_CAP and -(-(e[0] * e[1]) // 4) > AC.POOL_GRID_CAP
    ks = {s: AC.chunks_for(s[1], s[2] * s[3]) for s in shapes}
    assert ks[(3, 16, 5, 13)] == (2, 8) and ks[(2, 17, 15, 17)] == (3, 6) and ks[(1, 257, 257, 1)] == (33, 8) and ks[(2, 40, 64, 65)] == (5, 8)
    assert ks[(2, 3, 25, 40)] == (1, 3) and ks[(1, 2, 300, 300)] == (1, 2)          # one chunk: the pools leave the pooling pass finished
    assert any(k > 1 and s[1] % cpc for s, (k, cpc) in ks.items())                   # a ragged last chunk
    assert p[0] * tiles(p) * ks[p][0] > AC.POOL_GRID_CAP
    assert any((s[2] * s[3]) % 4 for s in shapes) and any((s[2] * s[3]) % 4 == 0 and (s[2] * s[3]) % AC.TILE for s in shapes)
    assert any(c.offset % 4 for c in AC.CASES)
    assert len(AC.COMBOS) == 41 and all(c.combos is None or set(c.combos) <= set(AC.COMBOS) for c in AC.CASES)
    t1, t2, _ = AC.inputs("n2c5_7x9_ties")
    for x in (t1, t2):
        flat = x.reshape(2, 5, -1)
        assert (flat[0, 4] == 0).all() and (flat[:, :, -1] == 0).all() and (flat[1, 0] == flat[1, 0].max()).sum() == 3
        assert flat[0, 0, 3] == flat[0, 3, 3] == flat[0, :, 3].max()


def test_abi_declares_the_entry_points_and_refuses_bad_arguments():
    """header, ctypes table and library agree (the library loads without a GPU); every refusal comes before any launch"""
    from mmif import _lib
    lib = _lib.lib
    hdr = open(os.path.join(os.path.dirname(AC.HERE), "include", "mmif.h")).read()
    for name in ("mmif_attn_fuse_workspace", "mmif_attn_fuse_fwd", "mmif_attn_fuse_bwd"):
        assert name in _lib.SIGNATURES and f" {name}(" in hdr and getattr(lib, name) is not None, name
    assert len(_lib.SIGNATURES["mmif_attn_fuse_fwd"][1]) == 19 and len(_lib.SIGNATURES["mmif_attn_fuse_bwd"][1]) == 21
    assert lib.mmif_attn_fuse_workspace(2, 5, 7, 9, 3, 4, 1) > 0
    for bad in ((2, 0, 7, 9, 3, 4, 1), (0, 5, 7, 9, 3, 4, 1), (65536, 5, 7, 9, 3, 4, 1), (2, 65536, 7, 9, 3, 4, 1), (2, 5, 0, 9, 3, 4, 1),
                (2, 5, 32768, 32768, 3, 4, 1), (2, 5, 7, 9, 4, 4, 1), (2, 5, 7, 9, -1, 4, 1), (2, 5, 7, 9, 3, 6, 1), (2, 5, 7, 9, 3, 4, 2)):
        assert lib.mmif_attn_fuse_workspace(*bad) == 0, bad
    # host memory stands in for the device pointers: nothing may be launched, and nothing is
    bufs = [np.zeros(2 * 5 * 7 * 9, np.float32) for _ in range(12)]
    p = [ctypes.c_void_p(b.ctypes.data) for b in bufs]
    need = lib.mmif_attn_fuse_workspace(2, 5, 7, 9, 3, 4, 1)
    dims = (2, 5, 7, 9)
    fwd = lambda t1, t2, out, pools, dims, codes, ws=p[9], nbytes=need: lib.mmif_attn_fuse_fwd(t1, t2, out, *pools, *dims, *codes, ws, nbytes, None)
    all6, none6 = p[3:9], [None] * 6
    assert fwd(None, p[1], p[2], all6, dims, (3, 4, 1)) == -1                              # NULL tensors
    assert fwd(p[0], p[1], None, all6, dims, (3, 4, 1)) == -1
    assert fwd(p[0], p[1], p[2], all6, dims, (3, 4, 1), ws=None) == -1
    assert fwd(p[0], p[1], p[2], all6, dims, (4, 4, 1)) == -1                              # a mode out of range
    assert fwd(p[0], p[1], p[2], all6, dims, (3, 6, 1)) == -1
    assert fwd(p[0], p[1], p[2], all6, dims, (3, 4, 2)) == -1
    assert fwd(p[0], p[1], p[2], all6, dims, (0, 4, 1)) == -1                              # 'sa' given channel pools
    assert fwd(p[0], p[1], p[2], [None, None] + p[5:9], dims, (2, 4, 1)) == -1             # 'sca' without spatial pools
    assert fwd(p[0], p[1], p[2], all6, dims, (3, 4, 0)) == -1                              # positions given to 'avg'
    assert fwd(p[0], p[1], p[2], p[3:7] + [None, None], dims, (3, 4, 1)) == -1             # 'max' without positions
    assert fwd(p[0], p[1], p[2], all6, (2, 0, 7, 9), (3, 4, 1)) == -1                      # c = 0
    assert fwd(p[0], p[1], p[2], all6, dims, (3, 4, 1), nbytes=need - 4) == -3             # a short workspace
    assert lib.mmif_attn_fuse_bwd(p[0], p[1], *none6, p[10], p[2], p[11], *dims, 3, 4, 1, p[9], need, None) == -1
    assert lib.mmif_attn_fuse_bwd(p[0], p[1], *all6, None, p[2], p[11], *dims, 3, 4, 1, p[9], need, None) == -1
    assert lib.mmif_attn_fuse_bwd(p[0], p[1], *all6, p[10], p[2], p[11], *dims, 3, 4, 1, p[9], need - 4, None) == -3
    assert all(not b.any() for b in bufs)
