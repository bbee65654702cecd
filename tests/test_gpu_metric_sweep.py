"""Metric kernels (core/metric.py on csrc/metric.hip and mmif_metric_msssim) against the fp64 oracle (oracle/metric_oracle.py, pinned to
golden F19 by tests/test_metric_oracle_cpu.py) at the shapes, values and batch sizes F19 does not hold: tile and grid-stride edges,
the smallest legal images, the size thresholds, the eval / bench size 1024x1224, every input distribution of
metric_cases.SWEEP_DISTS, non-finite histogram input, batches up to 16 and the accepted input forms."""
import math

import numpy as np
import pytest
import torch

import metric_cases as MC
from oracle import metric_oracle as O

pytestmark = pytest.mark.gpu

# Relative tolerances.  Everything but SSIM / MS-SSIM is fp64 in the kernels and the finishing code: RTOL = 1e-9, taken relative to
# max(|ref|, 1e-3) as in test_gpu_metric.  VIF's per-pixel variances E[x^2] - mu^2 cancel by up to mu^2 / sigma^2 (1e5 on the
# 'onebin' images), so its sums keep fewer digits: RTOL_VIF = 1e-8.  SSIM and MS-SSIM run in fp32: test_gpu_metric.TOL's 1e-4,
# relative to max(|ref|, 0.1): they are means of per-pixel values in [-1, 1] whose fp32 rounding error is absolute.
# Largest errors measured on an MI355X (printed as SWEEP_MARGINS): scd 9.0e-12, psnr 3.3e-13, mi 3.8e-14, mse 2.0e-14, every other
# fp64 metric <= 4.1e-15; viff 1.1e-9 (onebin 64x80), viff_full 5.0e-10; ssim 3.0e-6 absolute (mean -0.008, ramp 48x49), msssim 2.5e-6.
RTOL = 1e-9
RTOL_VIF = 1e-8
RTOL_FP32 = 1e-4
FP32_KEYS = ('ssim', 'msssim')

CALC_SHAPES = [(2, 2), (2, 17), (17, 2), (3, 3), (15, 16), (16, 17), (33, 31), (32, 64), (3, 683), (512, 513), (1024, 1224)]
BIG_DISTS = {(512, 513): ('int', 'ramp', 'edge'), (1024, 1224): ('int', 'flat')}
VIF_SHAPES = [(41, 41), (41, 42), (42, 41), (48, 49)]
MSSSIM_SHAPES = [(161, 161), (161, 176), (176, 177), (322, 161), (1024, 1224), (160, 200)]
BIG = (1024, 1224)

_WORST = {}   # metric -> (largest relative error seen, where) -- printed at the end of the module: run with -s


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    print("\nSWEEP_MARGINS (largest relative error per metric): "
          + "; ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in sorted(_WORST.items())))


def _dev(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def assert_close(got, ref, key, what):
    got, ref = float(got), float(ref)
    if math.isnan(ref) or math.isinf(ref):
        assert (math.isnan(got) and math.isnan(ref)) or got == ref, (what, got, ref)
        return
    fp32 = key in FP32_KEYS
    err = abs(got - ref) / max(abs(ref), 0.1 if fp32 else 1e-3)
    _WORST[key] = max(_WORST.get(key, (0.0, '')), (err, what))
    assert err <= (RTOL_FP32 if fp32 else RTOL_VIF if key.startswith('viff') else RTOL), (what, got, ref, err)


def _calc_values(M, a, b, f, parts):
    v = {}
    if 'moments' in parts:
        m = M.calc_mse(a, f)
        v.update(mean=M.calc_mean(f), std=M.calc_std(f), ag=M.calc_ag(f), sf=M.calc_sf(f), mse=m, psnr=M.calc_psnr(m),
                 psnr_root=M.calc_psnr(m, L=1.0, root=True), cc=M.calc_cc(a, f), scd=M.calc_scd(a, b, f))
    if 'entropy' in parts:
        v.update(en=M.calc_entropy(f), en_a=M.calc_entropy(a), ce=M.calc_cross_ent(a, f), mi=M.calc_mul_info(a, f),
                 mi_norm=M.calc_mul_info(a, f, normalized=True))
    if 'qabf' in parts:
        v.update(qabf=M.calc_Qabf(a, b, f), qabf_L1=M.calc_Qabf(a, b, f, L=1.0), nabf=M.calc_Nabf(a, b, f),
                 nabf_orig=M.calc_Nabf(a, b, f, modified=False), labf=M.calc_Labf(a, b, f))
        v['qabf_full_q'], v['qabf_full_n'], v['qabf_full_l'] = M.calc_Qabf(a, b, f, full=True)
    if 'vif' in parts:
        v.update(viff=M.calc_viff(a, b, f), viff_full=M.calc_viff(a, b, f, simple=False))
    if 'ssim' in parts:
        v.update(ssim=M.calc_ssim(a, f), msssim=M.calc_msssim(a, f))
    return v


def _check_pooled(dist, shape, n, parts, seed=0):
    import core.metric as M
    trip = MC.sweep_triple(dist, *shape, n=n, seed=seed)
    want = O.mirror(*trip, parts=parts)
    with torch.no_grad():
        got = _calc_values(M, *_dev(*trip), parts)
    for k, v in got.items():
        assert_close(v, want[k], k, f"{dist} {shape} n={n} {k}")


def _calc_cases():
    for shape in CALC_SHAPES:
        for dist in BIG_DISTS.get(shape, MC.SWEEP_DISTS):
            yield pytest.param(shape, dist, id=f"{shape[0]}x{shape[1]}-{dist}")


@pytest.mark.parametrize("shape,dist", list(_calc_cases()))
def test_moments_entropy_qabf_vs_oracle(shape, dist):
    """calc_mean .. calc_Labf at the QT = 16 tile edges, either side of sample_blocks' first step (2048 px) and cap (262,144 px),
    the 2x2 minimum (reflect halo at h or w = 2, 3) and 1024x1224"""
    _check_pooled(dist, shape, 1, ('moments', 'entropy', 'qabf'))


@pytest.mark.parametrize("dist", ['int', 'frac', 'anti'])
def test_pooled_mirror_functions_b3(dist):
    """B = 3: the reference's pooled values (means over the batch, summed histograms, sums over all samples), HIP MS-SSIM included"""
    _check_pooled(dist, (165, 170), 3, ('moments', 'entropy', 'qabf', 'vif', 'ssim'), seed=1)


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (2, 2)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dist", ['int', 'onebin', 'edge'])
def test_entropies_tiny_images(shape, n, dist):
    """the entropy functions accept 1-px images"""
    import core.metric as M
    a, _, f = MC.sweep_triple(dist, *shape, n=n)
    da, df = _dev(a, f)
    with torch.no_grad():
        got = {'en': M.calc_entropy(df), 'ce': M.calc_cross_ent(da, df), 'mi': M.calc_mul_info(da, df),
               'mi_norm': M.calc_mul_info(da, df, normalized=True)}
    want = {'en': O.entropy(f), 'ce': O.cross_ent(a, f), 'mi': O.mul_info(a, f), 'mi_norm': O.mul_info(a, f, True)}
    for k in got:
        assert_close(got[k], want[k], k, f"{dist} {shape} n={n} {k}")


@pytest.mark.parametrize("shape,n", [((1, 1), 1), ((1, 5), 2), ((3, 683), 3), ((64, 80), 1), ((512, 513), 2), (BIG, 2)])
def test_histograms_exact_with_nonfinite(shape, n):
    """exact u32 counts against np.histogram / np.histogram2d with an explicit range: NaN, +-inf, < 0 and > 256 dropped, 256.0 in
    bin 255, one ulp below an integer and the 64-row slab edges in their own bins; entropies of the pooled counts"""
    import core.metric as M
    x, y = MC.nonfinite_pair(*shape, n=n)
    dx, dy = _dev(x, y)
    with torch.no_grad():
        hx, hy, hxy = (t.cpu().numpy() for t in M._hist(dx, dy))
    for s in range(n):
        assert np.array_equal(hx[s], O.hist(x[s])), s
        assert np.array_equal(hy[s], O.hist(y[s])), s
        assert np.array_equal(hxy[s].reshape(256, 256), O.hist2(x[s], y[s])), s
    with torch.no_grad():
        got = {'en': M.calc_entropy(dy), 'ce': M.calc_cross_ent(dx, dy), 'mi': M.calc_mul_info(dx, dy),
               'mi_norm': M.calc_mul_info(dx, dy, normalized=True)}
    want = {'en': O.entropy(y), 'ce': O.cross_ent(x, y), 'mi': O.mul_info(x, y), 'mi_norm': O.mul_info(x, y, True)}
    for k in got:
        assert_close(got[k], want[k], k, f"nonfinite {shape} n={n} {k}")


def _check_fusion(a, b, f, what, want):
    import core.metric as M
    with torch.no_grad():
        got = M.fusion_metrics(*_dev(a, b, f))
    assert tuple(got) == O.FUSION_METRICS
    for k, v in got.items():
        assert v.shape == (a.shape[0],) and v.dtype == torch.float64, k
        for s in range(a.shape[0]):
            assert_close(v[s], want[k][s], k, f"{what} {k} sample {s}")


def _vif_cases():
    for shape in VIF_SHAPES:
        for dist in MC.SWEEP_DISTS:
            yield pytest.param(shape, dist, id=f"{shape[0]}x{shape[1]}-{dist}")
    yield pytest.param(BIG, 'int', id="1024x1224-int")


@pytest.mark.parametrize("shape,dist", list(_vif_cases()))
def test_fusion_metrics_and_viff_vs_oracle(shape, dist):
    """every eval.py column per sample and the pooled calc_viff (both forms) at the 41 px minimum, the VT = 16 edges of the scale-0
    output (48x49 -> 32x33) and at 1024x1224, where the scale-1 level (508x608) needs vif_down's second grid-stride pass"""
    import core.metric as M
    trip = MC.sweep_triple(dist, *shape)
    vs = O.vif_sums(*trip)
    _check_fusion(*trip, f"{dist} {shape}", O.eval_table(*trip, vif=vs))
    a, b, f = _dev(*trip)
    with torch.no_grad():
        assert_close(M.calc_viff(a, b, f), O.viff_value(vs.sum(1), True), 'viff', f"{dist} {shape} viff")
        assert_close(M.calc_viff(a, b, f, simple=False), O.viff_value(vs.sum(1), False), 'viff_full', f"{dist} {shape} viff_full")


def test_fusion_metrics_mixed_batch_b8():
    """B = 8, every sample a different distribution: each column per sample against the oracle"""
    a, b, f = MC.mixed_batch(64, 80, 8)
    _check_fusion(a, b, f, "mixed B=8", O.eval_table(a, b, f))


def test_fusion_metrics_b16_bitwise_b1():
    """B = 16 at 1024x1224 (the bench shape, histograms of 2B = 32 rows): each column bitwise the B = 1 call on that sample"""
    import core.metric as M
    a, b, f = _dev(*MC.mixed_batch(*BIG, 16, seed=5))
    with torch.no_grad():
        r16 = M.fusion_metrics(a, b, f)
        for i in range(16):
            r1 = M.fusion_metrics(a[i:i + 1], b[i:i + 1], f[i:i + 1])
            for k in r16:
                x, y = r16[k][i].item(), r1[k][0].item()
                assert x == y or (math.isnan(x) and math.isnan(y)), (k, i, x, y)


@pytest.mark.parametrize("shape", MSSSIM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_msssim_vs_oracle(shape):
    """HIP MS-SSIM from the 161 px threshold (every pyramid level odd: 161 -> 81 -> 41 -> 21 -> 11) up to 1024x1224, pooled over
    B = 2; 160x200 takes the stock path"""
    import core.metric as M
    n = 2 if shape != BIG else 1
    a, _, f = MC.sweep_triple('frac', *shape, n=n)
    want = O.msssim(a, f)
    with torch.no_grad():
        assert_close(M.calc_msssim(*_dev(a, f)), want, 'msssim', f"{shape}")


@pytest.mark.parametrize("shape,data_range", [((11, 11), 255.0), ((11, 300), 255.0), ((12, 13), 255.0), ((11, 300), 1.0)])
def test_calc_ssim_small_vs_oracle(shape, data_range):
    """calc_ssim at min(h, w) = 11 (a one-row SSIM map) and 12x13, B = 2; data_range 1.0 on 0..1 inputs as test.py calls it"""
    import core.metric as M
    a, _, f = MC.sweep_triple('frac', *shape, n=2)
    if data_range == 1.0:
        a, f = a / np.float32(255.0), f / np.float32(255.0)
    with torch.no_grad():
        assert_close(M.calc_ssim(*_dev(a, f), data_range=data_range), O.ssim(a, f, data_range), 'ssim', f"{shape} {data_range}")


def test_input_forms_bitwise():
    """fp64, uint8 and a non-contiguous column window give bitwise the values of their contiguous fp32 copy"""
    import core.metric as M
    a, b, f = (torch.from_numpy(x) for x in MC.sweep_triple('int', 170, 180, n=2))
    wide = [torch.cat([torch.zeros(2, 1, 170, 7), x, torch.ones(2, 1, 170, 5)], 3).cuda() for x in (a, b, f)]
    forms = {
        'fp64': [x.double().cuda() / 3.0 for x in (a, b, f)],
        'uint8': [x.to(torch.uint8).cuda() for x in (a, b, f)],
        'window': [x[..., 7:187] for x in wide],
    }

    def run(a, b, f):
        r = dict(M.fusion_metrics(a, b, f))
        r.update(mean=M.calc_mean(f), en=M.calc_entropy(f), mi=M.calc_mul_info(a, f), qabf=M.calc_Qabf(a, b, f),
                 viff=M.calc_viff(a, b, f), ssim=M.calc_ssim(a, f), msssim=M.calc_msssim(a, f))
        return {k: v.cpu() for k, v in r.items()}

    with torch.no_grad():
        for name, xs in forms.items():
            assert xs[0].dtype != torch.float32 or not xs[0].is_contiguous(), name
            got = run(*xs)
            want = run(*[x.float().contiguous() for x in xs])
            for k in want:
                assert torch.equal(got[k].nan_to_num(), want[k].nan_to_num()), (name, k, got[k], want[k])


def test_identical_images_exact_zero_mse():
    """calc_mse(x, x) is exactly 0 (PSNR inf) and CC(x, x) is 1, as the reference's direct sums give"""
    import core.metric as M
    (a,) = _dev(MC.sweep_triple('frac', 97, 130, n=2)[0])
    with torch.no_grad():
        assert float(M.calc_mse(a, a)) == 0.0 and math.isinf(float(M.calc_psnr(M.calc_mse(a, a))))
        r = M.fusion_metrics(a, a, a)
    assert torch.equal(r['mse'], torch.zeros(2, dtype=torch.float64, device=a.device))
    assert_close(M.calc_cc(a, a), 1.0, 'cc', "cc(x, x)")
