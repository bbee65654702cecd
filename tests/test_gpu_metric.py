"""Fusion-quality metrics (core/metric.py on csrc/metric.hip) against golden F19 -- the reference's own values in fp64."""
import math

import numpy as np
import pytest
import torch

import metric_cases as MC

pytestmark = pytest.mark.gpu

TOL = {'ssim': 1e-4, 'msssim': 1e-4, 'msssim_pad': 1e-4, 'viff': 2e-4, 'viff_full': 2e-4}   # everything else 1e-5
MIRROR = ['mean', 'std', 'ag', 'sf', 'mse', 'psnr', 'psnr_root', 'cc', 'scd', 'en', 'en_a', 'ce', 'mi', 'mi_norm', 'qabf', 'qabf_L1',
          'nabf', 'nabf_orig', 'labf', 'ssim', 'msssim', 'msssim_pad', 'qabf_full_q', 'qabf_full_n', 'qabf_full_l', 'viff', 'viff_full']


@pytest.fixture(scope="module")
def f19():
    return MC.load_f19()


def _dev(*xs):
    return [torch.from_numpy(x).cuda() for x in xs]


def assert_close(got, ref, tol, what):
    got, ref = float(got), float(ref)
    if math.isnan(ref) or math.isinf(ref):
        assert (math.isnan(got) and math.isnan(ref)) or got == ref, (what, got, ref)
        return
    assert abs(got - ref) <= tol * max(abs(ref), 1e-3), (what, got, ref, abs(got - ref) / max(abs(ref), 1e-12))


def mirror_values(M, a, b, f):
    v = {
        'mean': M.calc_mean(f), 'std': M.calc_std(f), 'ag': M.calc_ag(f), 'sf': M.calc_sf(f), 'mse': M.calc_mse(a, f),
        'psnr': M.calc_psnr(M.calc_mse(a, f)), 'psnr_root': M.calc_psnr(M.calc_mse(a, f), L=1.0, root=True),
        'cc': M.calc_cc(a, f), 'scd': M.calc_scd(a, b, f), 'en': M.calc_entropy(f), 'en_a': M.calc_entropy(a),
        'ce': M.calc_cross_ent(a, f), 'mi': M.calc_mul_info(a, f), 'mi_norm': M.calc_mul_info(a, f, normalized=True),
        'qabf': M.calc_Qabf(a, b, f), 'qabf_L1': M.calc_Qabf(a, b, f, L=1.0),
        'nabf': M.calc_Nabf(a, b, f), 'nabf_orig': M.calc_Nabf(a, b, f, modified=False), 'labf': M.calc_Labf(a, b, f),
        'ssim': M.calc_ssim(a, f), 'msssim': M.calc_msssim(a, f), 'msssim_pad': M.calc_msssim(a, f, use_padding=True),
    }
    v['qabf_full_q'], v['qabf_full_n'], v['qabf_full_l'] = M.calc_Qabf(a, b, f, full=True)
    if min(a.shape[-2:]) >= 41:
        v['viff'] = M.calc_viff(a, b, f)
        v['viff_full'] = M.calc_viff(a, b, f, simple=False)
    return v


@pytest.mark.parametrize("case", list(MC.CASES))
def test_mirror_functions_match_reference(case, f19):
    """every reference function and option, pooled over the batch for B > 1 (pooled2x256)"""
    import core.metric as M
    a, b, f = _dev(*MC.build(case, f19))
    with torch.no_grad():
        vals = mirror_values(M, a, b, f)
    for k, v in vals.items():
        assert_close(v, f19[f"{case}|{k}|64"], TOL.get(k, 1e-5), f"{case} {k}")


@pytest.mark.parametrize("case", ["cf256_int", "cf97x130_frac", "nat256x320", "histedge64x80", "pooled2x256"])
def test_histograms_exact_and_entropies(case, f19):
    import core.metric as M
    a, b, f = MC.build(case, f19)
    hx, hy, hxy = M._hist(*_dev(a, f))
    for s in range(a.shape[0]):
        x, y = a[s].ravel().astype(np.float64), f[s].ravel().astype(np.float64)
        assert np.array_equal(hx[s].cpu().numpy(), np.histogram(x, 256, (0, 256))[0])
        assert np.array_equal(hy[s].cpu().numpy(), np.histogram(y, 256, (0, 256))[0])
        assert np.array_equal(hxy[s].cpu().numpy().reshape(256, 256), np.histogram2d(x, y, 256, ((0, 256), (0, 256)))[0])
    # entropies of the pooled numpy counts in fp64
    x, y = a.ravel().astype(np.float64), f.ravel().astype(np.float64)
    p1, p2 = np.histogram(x, 256, (0, 256))[0] / x.size, np.histogram(y, 256, (0, 256))[0] / y.size
    p12 = np.histogram2d(x, y, 256, ((0, 256), (0, 256)))[0] / x.size
    ent = lambda p: -np.sum(p[p != 0] * np.log2(p[p != 0]))
    m = (p1 * p2) != 0
    en1, en2, je, ce = ent(p1), ent(p2), ent(p12), np.sum(p1[m] * np.log2(p1[m] / p2[m]))
    da, df = _dev(a, f)
    got = {'en': M.calc_entropy(df), 'ce': M.calc_cross_ent(da, df), 'mi': M.calc_mul_info(da, df), 'mi_norm': M.calc_mul_info(da, df, True)}
    want = {'en': en2, 'ce': ce, 'mi': en1 + en2 - je, 'mi_norm': 2 * (en1 + en2 - je) / (en1 + en2)}
    for k in got:
        assert abs(float(got[k]) - want[k]) <= 1e-9 * abs(want[k]), (case, k, float(got[k]), want[k])
        assert abs(float(got[k]) - f19[f"{case}|{k}|64"]) <= 1e-6 * abs(f19[f"{case}|{k}|64"]), (case, k)


EVAL_CASES = [c for c in MC.CASES if min(MC.CASES[c][1]) >= 41]


@pytest.mark.parametrize("case", EVAL_CASES)
def test_fusion_metrics_match_eval_table(case, f19):
    import core.metric as M
    a, b, f = _dev(*MC.build(case, f19))
    with torch.no_grad():
        r = M.fusion_metrics(a, b, f)
    assert list(r) == list(M.FUSION_METRICS)
    for k, v in r.items():
        assert v.shape == (a.shape[0],) and v.dtype == torch.float64, k
        for s in range(a.shape[0]):
            assert_close(v[s], f19[f"{case}|eval_{k}|{s}|64"], TOL.get(k, 1e-5), f"{case} {k} sample {s}")


def test_fusion_metrics_batch_invariant_and_deterministic(f19):
    """column i of a B = 4 call is bitwise the B = 1 call on sample i; two runs are bitwise equal"""
    import core.metric as M
    parts = [MC.build("cf256_int", f19), MC.build("pooled2x256", f19), MC.build("histedge64x80", f19)]
    a = np.concatenate([parts[0][0], parts[1][0], np.pad(parts[2][0], ((0, 0), (0, 0), (0, 192), (0, 176)), mode='reflect')])
    b = np.concatenate([parts[0][1], parts[1][1], np.pad(parts[2][1], ((0, 0), (0, 0), (0, 192), (0, 176)), mode='reflect')])
    f = np.concatenate([parts[0][2], parts[1][2], np.pad(parts[2][2], ((0, 0), (0, 0), (0, 192), (0, 176)), mode='reflect')])
    assert a.shape == (4, 1, 256, 256)
    a, b, f = _dev(a, b, f)
    with torch.no_grad():
        r4 = M.fusion_metrics(a, b, f)
        r4b = M.fusion_metrics(a, b, f)
        for k in r4:
            assert torch.equal(r4[k], r4b[k]) or (torch.isnan(r4[k]).any() and torch.equal(r4[k].nan_to_num(), r4b[k].nan_to_num())), k
        for i in range(4):
            r1 = M.fusion_metrics(a[i:i + 1], b[i:i + 1], f[i:i + 1])
            for k in r4:
                x, y = r4[k][i].item(), r1[k][0].item()
                assert x == y or (math.isnan(x) and math.isnan(y)), (k, i, x, y)


def test_validation():
    import core.metric as M
    x = torch.rand(1, 1, 64, 64) * 255
    with pytest.raises(RuntimeError):
        M.calc_std(x)   # CPU tensor
    with pytest.raises(RuntimeError):
        M.calc_std(x.cuda()[0])   # rank 3
    with pytest.raises(RuntimeError):
        M.calc_cc(torch.rand(1, 2, 64, 64, device='cuda'), torch.rand(1, 2, 64, 64, device='cuda'))
    with pytest.raises(RuntimeError):
        M.fusion_metrics(x, x, x)
    y = torch.rand(1, 1, 40, 64, device='cuda') * 255
    with pytest.raises(ValueError, match="41"):
        M.calc_viff(y, y, y)
    with pytest.raises(ValueError, match="41"):
        M.fusion_metrics(y, y, y)
