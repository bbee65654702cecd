"""Golden F21 on the CPU: the numpy float64 restatement of spatial_pooling(x, 'nl') in tests/nonlocal_cases.py (explicit backward
formulas, the ones csrc/nonlocal.hip implements) against the reference's own float64 results, the tie guard of every case, and the
argument validation of the three mmif_nonlocal_spatial_* entry points (which runs before any launch, so it needs no GPU)."""
import ctypes
import os

import numpy as np
import pytest

import nonlocal_cases as NC


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(NC.F21) <= 802015, "f21_nonlocal.npz must not outgrow the largest older fixture (f3_conv.npz)"
    return np.load(NC.F21)


@pytest.mark.parametrize("name", list(NC.CASES))
def test_numpy_restatement_meets_the_reference_fixture(golden, name):
    x, g = NC.inputs(name), NC.upstream(name)
    assert x.min() >= 0 and x.max() > 0
    o = NC.nonlocal_f64(x, g)
    idx = NC.sample_index(x.size)
    for key in ("y", "dx"):
        ref = golden[f"{name}|{key}"]
        assert ref.shape == idx.shape and np.abs(ref).max() > 0
        err = np.abs(o[key].reshape(-1)[idx] - ref).max() / np.abs(ref).max()
        assert err <= 1e-10, (name, key, err)
    assert abs(o["lo"] - golden[f"{name}|lo"]) <= 1e-12 * abs(o["hi"]) and abs(o["hi"] - golden[f"{name}|hi"]) <= 1e-12 * abs(o["hi"])


@pytest.mark.parametrize("name", list(NC.CASES))
def test_tie_guard_holds(name):
    """unique extrema (torch splits the gradient across ties: such inputs are not in the table) and a range that is not tiny"""
    o = NC.nonlocal_f64(NC.inputs(name))
    assert o["gap_lo"] > NC.TIE_GAP and o["gap_hi"] > NC.TIE_GAP, (name, o["gap_lo"], o["gap_hi"])
    assert o["hi"] - o["lo"] > 1e-3 * abs(o["hi"])


def test_m1_case_is_the_identity_plus_the_pooled_row():
    """M = 1: S == 1, so y = x + P whatever lo and hi are, and dZ == 0"""
    x = NC.inputs("m1")
    o = NC.nonlocal_f64(x, NC.upstream("m1"))
    assert np.allclose(o["y"], x.astype(np.float64) + NC.pool8(x.astype(np.float64)), rtol=0, atol=1e-14)


def test_scale2_case_couples_the_samples():
    """the global min / max runs over the batch: sample 0's attention term (y - x) alone differs from the one it gets inside the batch by
    far more than any fp32 tolerance used on this case"""
    x = NC.inputs("scale2")
    both, alone = NC.nonlocal_f64(x)["y"][0], NC.nonlocal_f64(x[:1])["y"][0]
    assert np.abs(both - alone).max() > 1e-3 * np.abs(both - x[0]).max()
    assert np.abs(both - alone).max() > 5e-4 * np.abs(both).max()


def test_nonlocal_c_abi_exists_and_validates_before_any_launch():
    from mmif._lib import SIGNATURES, lib
    for name in ("mmif_nonlocal_spatial_workspace", "mmif_nonlocal_spatial_fwd", "mmif_nonlocal_spatial_bwd"):
        assert name in SIGNATURES and hasattr(lib, name), name
    f = (ctypes.c_float * 64)()
    big = 1 << 30
    ws_fn, fwd, bwd = lib.mmif_nonlocal_spatial_workspace, lib.mmif_nonlocal_spatial_fwd, lib.mmif_nonlocal_spatial_bwd
    for n, c, h, w in ((1, 16, 7, 16), (1, 16, 16, 7), (1, 0, 16, 16), (1, 257, 16, 16), (0, 16, 16, 16)):
        assert ws_fn(n, c, h, w) == 0
        assert fwd(f, f, f, f, n, c, h, w, f, big, None) == -1
        assert b"h, w >= 8" in lib.mmif_last_error() and b"mmif_nonlocal_spatial_fwd" in lib.mmif_last_error()
        assert bwd(f, f, f, f, f, f, n, c, h, w, f, big, None) == -1
        assert b"mmif_nonlocal_spatial_bwd" in lib.mmif_last_error()
    assert fwd(None, f, f, f, 1, 16, 16, 16, f, big, None) == -1
    assert b"null pointer" in lib.mmif_last_error()
    assert fwd(f, f, f, f, 1, 16, 16, 16, None, big, None) == -1
    assert bwd(f, f, f, f, None, f, 1, 16, 16, 16, f, big, None) == -1
    assert b"null pointer" in lib.mmif_last_error()
    need = ws_fn(1, 16, 16, 16)
    assert need > 0
    assert fwd(f, f, f, f, 1, 16, 16, 16, f, need - 1, None) == -3
    assert bwd(f, f, f, f, f, f, 1, 16, 16, 16, f, need - 1, None) == -3
    assert b"workspace" in lib.mmif_last_error()
    assert ws_fn(4, 112, 64, 64) > ws_fn(2, 112, 64, 64) > ws_fn(1, 112, 64, 64) > 0
    assert ws_fn(1, 256, 8, 8) > 0 and ws_fn(1, 1, 8, 8) > 0
    # the capability itself: far below one energy tensor (N * M * 4 bytes) at the training shape
    assert ws_fn(1, 112, 256, 256) < 65536 * 1024 * 4 // 4


def test_cpu_tensors_keep_the_composition(monkeypatch):
    """CPU tensors (and shapes outside the kernels' limits) stay on the tensor-level composition, under either switch setting"""
    import torch
    from core.fusion import spatial_pooling
    x = NC.inputs("b3c7")
    ref = NC.nonlocal_f64(x)["y"]
    for impl in ("hip", "torch"):
        monkeypatch.setenv("MMIF_NONLOCAL", impl)
        y = spatial_pooling(torch.from_numpy(x), 'nl').numpy()
        assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max()
    monkeypatch.setenv("MMIF_NONLOCAL", "triton")
    with pytest.raises(ValueError, match="MMIF_NONLOCAL"):
        spatial_pooling(torch.from_numpy(x), 'nl')


# ------------------------------------------------------------------------------------------------------------------------------ the sweep table
# what makes tests/test_gpu_nonlocal_sweep.py mean something: the term-wise reference is the restatement, no extremum is a near-tie, every mutant
# lies far outside the tolerance, and the tolerance constants are what the float32 evaluation says they are
SWEEP_NAMES = [c.name for c in NC.SWEEP]
GAP_MIN = 1e-4         # and, per case, >= 100 x its own float32 energy error (4.6e-8 ... 2.1e-6 of hi - lo on this table)
MUTANT_FACTOR = 20.0


def test_sweep_names_are_unique_and_tolerances_positive():
    assert len(NC.BY_NAME) == len(NC.SWEEP)
    for c in NC.SWEEP:
        assert len(c.tol) == 4 and all(0 < t < 1e-4 for t in c.tol), c


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_terms_sum_to_the_restatement(name):
    x, g, ref, _ = NC.reference(name)
    full = NC.nonlocal_f64(x, g)
    dx = g.astype(np.float64) + ref["tB"] + ref["tC"] + ref["tD"] + ref["tR"]
    assert np.abs(dx - full["dx"]).max() <= 1e-13 * np.abs(full["dx"]).max()
    assert np.abs(x.astype(np.float64) + ref["a"] - full["y"]).max() <= 1e-13 * np.abs(full["y"]).max()
    assert abs(ref["lo"] - full["lo"]) <= 1e-13 * abs(full["hi"]) and abs(ref["hi"] - full["hi"]) <= 1e-13 * abs(full["hi"])
    assert np.array_equal(ref["d"], ref["tB"] + ref["tC"] + ref["tD"] + ref["tR"])
    assert ref["l"].shape == (x.shape[0], x.shape[2] * x.shape[3]) and (ref["l"] >= 1.0).all()       # Z >= 0: every exp is >= 1
    if not NC.BY_NAME[name].tie:
        assert abs(ref["gap_lo"] - full["gap_lo"]) <= 1e-12 and abs(ref["gap_hi"] - full["gap_hi"]) <= 1e-12


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_sweep_inputs_are_what_the_table_says(name):
    c = NC.BY_NAME[name]
    x, g, ref, _ = NC.reference(name)
    assert x.dtype == np.float32 and g.dtype == np.float32 and x.shape == c.shape == g.shape
    assert (x.min() < 0) == c.signed and g.min() < 0 < g.max()
    assert NC.kc_for(c.shape[1]) == c.kc and NC.jt_for(c.shape[2], c.shape[3]) == c.jt
    m = (c.shape[2] // 8) * (c.shape[3] // 8)
    assert ref["pos_lo"][2] < m and ref["pos_hi"][2] < m


def test_every_channel_width_is_swept_at_both_ends_and_the_key_loop_at_every_kind_of_tail():
    lowest = {1: 1, 2: 17, 4: 33, 7: 65, 8: 113, 12: 129, 16: 193}
    highest = {1: 16, 2: 32, 4: 64, 7: 112, 8: 128, 12: 192, 16: 256}
    for kc in lowest:
        assert NC.kc_for(lowest[kc]) == kc == NC.kc_for(highest[kc]) and (lowest[kc] == 1 or NC.kc_for(lowest[kc] - 1) < kc)
        cs = {c.shape[1] for c in NC.SWEEP if c.kc == kc}
        assert lowest[kc] in cs and highest[kc] in cs, (kc, sorted(cs))
    assert NC.kc_for(highest[16] + 1 - 1) == 16
    ms = {(c.shape[2] // 8) * (c.shape[3] // 8): c for c in NC.SWEEP}
    assert {1, 17, 32} <= set(ms)                                   # one key; a tile plus one key; exactly one pair
    ragged = [m for m, c in ms.items() if m > 32 and m % 32]       # a last pair that is partly (or, past 16 keys short, half) padding
    assert any(m % 32 <= 16 for m in ragged) and len(ragged) >= 3 and all(ms[m].jt == 4 for m in ragged)
    assert any(c.kc == 8 and c.jt == 4 for c in NC.SWEEP)
    assert any(c.signed and c.jt == 4 for c in NC.SWEEP) and any(c.shape[2] % 8 and c.shape[3] % 8 for c in NC.SWEEP)
    assert any((c.shape[2] * c.shape[3]) % 16 for c in NC.SWEEP)


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_gap_condition(name):
    """no extremum of a non-tie case is a near-tie; the zero-pixel cases tie in lo only; the duplicate case ties in both, exactly"""
    c = NC.BY_NAME[name]
    _, _, ref, _ = NC.reference(name)
    assert ref["hi"] - ref["lo"] > 1e-3 * max(abs(ref["hi"]), abs(ref["lo"]))
    if c.tie is None:
        assert ref["gap_lo"] >= GAP_MIN and ref["gap_hi"] >= GAP_MIN, (name, ref["gap_lo"], ref["gap_hi"])
    elif c.tie == "zero":
        assert ref["gap_lo"] == 0.0 and ref["gap_hi"] >= GAP_MIN
    else:
        assert ref["gap_lo"] == 0.0 and ref["gap_hi"] == 0.0


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_tolerance_constants_are_honest_and_every_mutant_is_far(name):
    c = NC.BY_NAME[name]
    _, _, ref, dist = NC.reference(name)
    live = NC.float32_errors(name)
    print(f"{name}: float32 errors a {live[0]:.2e} l {live[1]:.2e} d {live[2]:.2e} E {live[3]:.2e}; tolerances {c.tol}")
    for what, e, tol in zip(("a", "l", "d", "lo/hi/r"), live, c.tol):
        assert e <= tol / 4.0, (name, what, e, tol)
    if c.tie != "dup":          # the rule behind GAP_MIN, with this case's own energy error: the fp32 argmin / argmax provably is the fp64 one
        assert min(ref["gap_hi"], ref["gap_hi"] if c.tie else ref["gap_lo"]) >= 100.0 * live[3], (name, ref["gap_lo"], ref["gap_hi"], live[3])
    m = (c.shape[2] // 8) * (c.shape[3] // 8)
    assert set(dist) == ({"no_tC"} if m == 1 else set(NC.MUTANTS_A + NC.MUTANTS_D)), (name, sorted(dist))
    for k, v in dist.items():
        tol = c.tol[0] if k in NC.MUTANTS_A else c.tol[2]
        print(f"{name}: mutant {k} at {v:.3e} = {v / tol:.0f} x the tolerance")
        assert v >= MUTANT_FACTOR * tol, (name, k, v, tol)


def test_scaled_cases_put_the_maximum_where_they_say():
    last = NC.BY_NAME["scale_123"].shape[0] - 1
    assert NC.reference("scale_312")[2]["pos_hi"][0] == 0
    assert NC.reference("scale_123")[2]["pos_hi"][0] == last
    assert NC.reference("scale_123_signed")[2]["pos_hi"][0] == last
    assert NC.BY_NAME["scale_123_signed"].signed and not NC.BY_NAME["scale_123"].signed


@pytest.mark.parametrize("name", [c.name for c in NC.SWEEP if c.tie])
def test_tie_cases_tie_exactly_and_the_first_position_is_the_kernels_order(name):
    """The rule held here is the kernels' own (ties go to the smallest (sample, position), position = i * M + j), not torch's even split.  The
    ties are exact in float32 as well as float64: a zero query pixel's energies are sums of exact zeros, a bit-copied sample repeats every bit."""
    c = NC.BY_NAME[name]
    x, g, ref, _ = NC.reference(name)
    e = ref["e"]
    b, n, m = e.shape
    e32 = NC.nonlocal_terms_f32(x, g)["e"]
    for ee in (e, e32):
        for pos, tied in ((ref["pos_lo"], ee == ee.min()), (ref["pos_hi"], ee == ee.max())):
            bb, ii, jj = np.nonzero(tied)
            order = sorted(zip(bb.tolist(), (ii * m + jj).tolist()))       # (sample, i * M + j): the order csrc/nonlocal.hip documents
            assert (order[0][0], order[0][1] // m, order[0][1] % m) == pos
    lo_ties, hi_ties = int((e == e.min()).sum()), int((e == e.max()).sum())
    if c.tie == "zero":
        assert ref["lo"] == 0.0 and lo_ties == b * m and hi_ties == 1 and ref["pos_lo"] == (0, NC.ZERO_PIXEL, 0) and NC.ZERO_PIXEL != 0
        assert (e32 == 0).sum() == b * m and e32.min() == 0
    else:
        assert np.array_equal(x[0], x[1]) and lo_ties == 2 and hi_ties == 2 and ref["pos_lo"][0] == 0 and ref["pos_hi"][0] == 0
        assert np.array_equal(e32[0], e32[1])
        assert ref["pos_lo2"] == (1,) + ref["pos_lo"][1:] and ref["pos_hi2"] == (1,) + ref["pos_hi"][1:]    # the "second" mutant routes to sample 1
