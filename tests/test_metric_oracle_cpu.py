"""The fp64 metric oracle (oracle/metric_oracle.py) against golden F19, the reference's own fp64 values -- no GPU.  This is what makes
the oracle a valid yardstick for tests/test_gpu_metric_sweep.py at shapes and values F19 does not hold."""
import math

import numpy as np
import pytest

import metric_cases as MC
from oracle import metric_oracle as O

# relative tolerances, tighter than test_gpu_metric.TOL everywhere.  Largest errors measured against F19: 1.5e-15 (mi_norm), every
# other mirror and eval value <= 4.6e-16 or exact, viff_full 8.7e-8: the reference keeps that form's per-scale ratios in an fp32
# tensor, the oracle (and the kernels) in fp64.
RTOL = 1e-12
RTOL_KEY = {'viff_full': 2e-7, 'eval_viff': 2e-7}


@pytest.fixture(scope="module")
def f19():
    return MC.load_f19()


def assert_close(got, ref, tol, what):
    got, ref = float(got), float(ref)
    if math.isnan(ref) or math.isinf(ref):
        assert (math.isnan(got) and math.isnan(ref)) or got == ref, (what, got, ref)
        return
    assert abs(got - ref) <= tol * max(abs(ref), 1e-300), (what, got, ref, abs(got - ref) / max(abs(ref), 1e-300))


@pytest.mark.parametrize("case", list(MC.CASES))
def test_oracle_mirror_matches_f19(case, f19):
    """every mirror key of F19 (pooled over the batch for pooled2x256)"""
    a, b, f = MC.build(case, f19)
    got = O.mirror(a, b, f)
    want = [k for k in f19 if k.startswith(case + "|") and k.endswith("|64") and "|eval_" not in k]
    assert sorted(got) == sorted(k.split("|")[1] for k in want)
    for k, v in got.items():
        assert_close(v, f19[f"{case}|{k}|64"], RTOL_KEY.get(k, RTOL), f"{case} {k}")


@pytest.mark.parametrize("case", [c for c in MC.CASES if min(MC.CASES[c][1]) >= 41])
def test_oracle_eval_table_matches_f19(case, f19):
    """eval.py's 16 values of every sample"""
    a, b, f = MC.build(case, f19)
    got = O.eval_table(a, b, f)
    assert tuple(got) == O.FUSION_METRICS
    for k, v in got.items():
        assert v.shape == (a.shape[0],)
        for s in range(a.shape[0]):
            assert_close(v[s], f19[f"{case}|eval_{k}|{s}|64"], RTOL_KEY.get("eval_" + k, RTOL), f"{case} {k} sample {s}")


def test_oracle_histogram_semantics():
    """bin floor(v) on [0, 256), 256 -> bin 255, everything else (NaN, +-inf, < 0, > 256) dropped but counted in numel"""
    x = np.array([0.0, -0.0, 255.5, 256.0, np.nextafter(256.0, 0.0), 63.999, 64.0, -1e-30, 256.0001, np.nan, np.inf, -np.inf])
    h = O.hist(x)
    assert h.sum() == 7 and h[0] == 2 and h[255] == 3 and h[63] == 1 and h[64] == 1
    assert O.hist2(x, x).sum() == 7 and O.hist2(x, x)[255, 255] == 3
    assert O.entropy(np.full((1, 1, 4, 4), 100.5)) == 0.0
    assert math.isnan(O.mul_info(np.full((1, 1, 4, 4), 100.5), np.full((1, 1, 4, 4), 7.0), normalized=True))


@pytest.mark.parametrize("dist", MC.SWEEP_DISTS)
def test_sweep_inputs(dist):
    """the sweep generators are deterministic float32 and carry the features they are named for"""
    a, b, f = MC.sweep_triple(dist, 48, 49, 2, seed=3)
    a2, b2, f2 = MC.sweep_triple(dist, 48, 49, 2, seed=3)
    for x, y in ((a, a2), (b, b2), (f, f2)):
        assert x.dtype == np.float32 and x.shape == (2, 1, 48, 49) and np.array_equal(x, y, equal_nan=True)
    if dist == 'int':
        ga, _ = O.sobel(a)
        gf, _ = O.sobel(f)
        assert (ga == gf).sum() > 0 and np.array_equal(np.round(f), f)
    elif dist == 'ramp':
        g, al = (t.numpy() for t in O.sobel(a))
        h = math.pi / 2
        for lo, hi in ((0, h), (h, 2 * h), (-2 * h, -h), (-h, 0)):   # all four open quadrants
            assert ((al > lo) & (al < hi)).any(), (lo, hi)
        assert (np.abs(al) == h).any() and (g == 0).any()   # gx == 0 exactly, and zero gradients
    elif dist == 'flat':
        assert (O.sobel(f)[0] == 0).any() and (a == 0).any()
    elif dist == 'anti':
        assert O.cc(a, f) < -0.999
    elif dist == 'same':
        assert np.array_equal(a, b)
    elif dist == 'onebin':
        assert all((np.floor(x) == 100).all() for x in (a, b, f))
        assert math.isnan(O.mul_info(a, f, normalized=True))
    elif dist == 'edge':
        vals = set(np.concatenate([a.ravel(), f.ravel()]).tolist())
        assert {256.0, 64.0, 128.0, 192.0, 300.0, -3.5} <= vals
    x, y = MC.nonfinite_pair(33, 31, 2)
    assert np.isnan(x).any() and np.isinf(y).any()
