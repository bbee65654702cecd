"""channel_pooling(x, 'nl') and attention_fusion(a, b, mode, 'nl', 'nl') through the public functions, on the kernels of
csrc/nonlocal_channel.hip, against golden F26 (the reference in float64) and the numpy float64 restatement of tests/channel_nl_cases.py.

Tolerance: the bar of tests/test_gpu_nonlocal.py.  Errors are max |got - ref| / max |ref|.  TORCH_ERR below is the error of the fp32
tensor-level composition ($MMIF_NONLOCAL=torch: rocBLAS matmuls, torch softmax and element-wise ops, the only path before these kernels) against
the same float64 values, measured on an MI355X; the HIP path's bar is  max(1e-4, 4 * that error)  -- 1e-4 is the project's fp32 bar, the factor
4 allows for a different but equally legitimate summation order.  The measured composition errors are 0 ... 1.9e-7 (four times that is far
below 1e-4), so the bar is 1e-4 for every case and tensor; the HIP path measured 0 ... 1.9e-7 on the same cases.  Each test prints the live figures of both paths before it asserts
(DESIGN.md section 4.5.1 records them).
"""
import numpy as np
import pytest
import torch

import channel_nl_cases as CC

pytestmark = pytest.mark.gpu

FP32_BAR = 1e-4
# case -> errors of the fp32 composition against float64, measured (MI355X, ROCm torch): (y, dx) for the channel map, (out, d1, d2) for the layer
TORCH_ERR = {
    "b2c7": (9.581e-08, 5.008e-08),
    "c20_signed": (6.110e-08, 6.909e-08),
    "b3c1": (0.0, 0.0),
    "c112": (1.838e-07, 5.133e-08),
    "scale2": (1.036e-07, 7.812e-08),
    "fusion_sa": (1.028e-07, 1.322e-07, 1.112e-07),
    "fusion_ca": (9.152e-08, 1.193e-07, 1.355e-07),
    "fusion_sca": (1.007e-07, 1.362e-07, 1.032e-07),
    "fusion_wavg": (1.030e-07, 9.660e-08, 1.090e-07),
}


def bar(case, k):
    return max(FP32_BAR, 4.0 * TORCH_ERR[case][k])


def err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def run_channel(x, g, impl, monkeypatch):
    """(y, dx, grad_fn name) of channel_pooling(x, 'nl') under $MMIF_NONLOCAL = impl"""
    from core.fusion import channel_pooling
    monkeypatch.setenv("MMIF_NONLOCAL", impl)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = channel_pooling(xt, 'nl')
    y.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    return y.detach().cpu().numpy(), xt.grad.cpu().numpy(), type(y.grad_fn).__name__


def run_fusion(mode, impl, monkeypatch, arrs=None):
    """(out, d1, d2, grad_fn name) of attention_fusion(t1, t2, mode, 'nl', 'nl') under $MMIF_NONLOCAL = impl"""
    from core.fusion import attention_fusion
    monkeypatch.setenv("MMIF_NONLOCAL", impl)
    t1, t2, g = arrs if arrs is not None else CC.fusion_inputs()
    a, b = torch.from_numpy(t1).cuda().requires_grad_(True), torch.from_numpy(t2).cuda().requires_grad_(True)
    o = attention_fusion(a, b, mode, 'nl', 'nl')
    o.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    return o.detach().cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy(), type(o.grad_fn).__name__


def test_library_exports_the_new_entry_points():
    from mmif._lib import lib
    for name in ("mmif_nonlocal_channel_workspace", "mmif_nonlocal_channel_fwd", "mmif_nonlocal_channel_bwd", "mmif_fuse_join_fwd", "mmif_fuse_join_bwd"):
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("name", list(CC.CASES))
def test_channel_map_vs_golden_and_restatement(name, monkeypatch):
    gold = np.load(CC.F26)
    x, g = CC.inputs(name), CC.upstream(name)
    idx = CC.sample_index(x.size)
    full = CC.channel_f64(x, g)
    figs = {}
    for impl in ("hip", "torch"):
        y, dx, fn = run_channel(x, g, impl, monkeypatch)
        figs[impl] = (err(y.reshape(-1)[idx], gold[f"{name}|y"]), err(dx.reshape(-1)[idx], gold[f"{name}|dx"]), err(y, full["y"]), err(dx, full["dx"]))
        print(f"F26 {name} {impl} ({fn}): y {figs[impl][0]:.3e} dx {figs[impl][1]:.3e} (fixture sample)  y {figs[impl][2]:.3e} dx {figs[impl][3]:.3e} (all elements)")
        assert fn.startswith("_NonlocalChannelFn") == (impl == "hip"), (impl, fn)
    e = figs["hip"]
    assert e[0] <= bar(name, 0) and e[2] <= bar(name, 0), (name, "y", e)
    assert e[1] <= bar(name, 1) and e[3] <= bar(name, 1), (name, "dx", e)


@pytest.mark.parametrize("mode", CC.FUSION_MODES)
def test_fusion_layer_vs_golden(mode, monkeypatch):
    gold = np.load(CC.F26)
    idx = CC.sample_index(int(np.prod(CC.FUSION_SHAPE)))
    figs = {}
    for impl in ("hip", "torch"):
        *res, fn = run_fusion(mode, impl, monkeypatch)
        figs[impl] = tuple(err(v.reshape(-1)[idx], gold[f"fusion_{mode}|{k}"]) for v, k in zip(res, ("out", "d1", "d2")))
        print(f"F26 fusion {mode} {impl} ({fn}): out {figs[impl][0]:.3e} d1 {figs[impl][1]:.3e} d2 {figs[impl][2]:.3e}")
        assert fn.startswith("_FusionJoinFn") == (impl == "hip"), (impl, fn)
    for k in range(3):
        assert figs["hip"][k] <= bar(f"fusion_{mode}", k), (mode, k, figs)


@pytest.mark.parametrize("name", ["b2c7", "c112", "scale2"])
def test_switch_settings_agree_channel(name, monkeypatch):
    x, g = CC.inputs(name), CC.upstream(name)
    (yh, dh, _), (yt, dt, _) = run_channel(x, g, "hip", monkeypatch), run_channel(x, g, "torch", monkeypatch)
    ey, ed = err(yh, yt.astype(np.float64)), err(dh, dt.astype(np.float64))
    print(f"F26 {name} hip vs torch: y {ey:.3e} dx {ed:.3e}")
    assert ey <= bar(name, 0) and ed <= bar(name, 1)


@pytest.mark.parametrize("mode", CC.FUSION_MODES)
def test_switch_settings_agree_fusion(mode, monkeypatch):
    h, t = run_fusion(mode, "hip", monkeypatch), run_fusion(mode, "torch", monkeypatch)
    es = [err(a, b.astype(np.float64)) for a, b in zip(h[:3], t[:3])]
    print(f"F26 fusion {mode} hip vs torch: out {es[0]:.3e} d1 {es[1]:.3e} d2 {es[2]:.3e}")
    assert all(e <= bar(f"fusion_{mode}", k) for k, e in enumerate(es))


def test_the_default_is_the_hip_path_and_it_is_bit_identical_run_to_run(monkeypatch):
    from core import fusion
    monkeypatch.delenv("MMIF_NONLOCAL", raising=False)
    assert fusion._nonlocal_impl() == "hip"
    x = torch.from_numpy(CC.inputs("c112")).cuda().requires_grad_(True)
    assert type(fusion.channel_pooling(x, 'nl').grad_fn).__name__.startswith("_NonlocalChannelFn")
    t1, t2, _ = (torch.from_numpy(a).cuda() for a in CC.fusion_inputs())
    for mode in CC.FUSION_MODES:
        o = fusion.attention_fusion(t1.requires_grad_(True), t2, mode, 'nl', 'nl')
        assert type(o.grad_fn).__name__.startswith("_FusionJoinFn"), mode
    a, b = run_fusion("sca", "hip", monkeypatch), run_fusion("sca", "hip", monkeypatch)
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))


def test_unsupported_inputs_fall_to_the_composition(monkeypatch):
    from core import fusion
    from mmif import tensor as T
    monkeypatch.setenv("MMIF_NONLOCAL", "hip")
    for shape in ((1, 257, 4, 4), (1, 1, 4, 4)):
        x = torch.rand(shape, device="cuda").requires_grad_(True)
        assert not T.nonlocal_channel_supported(x)
        assert not type(fusion.channel_pooling(x, 'nl').grad_fn).__name__.startswith("_NonlocalChannelFn")
    assert not T.nonlocal_channel_supported(torch.rand(2, 4, 4, 4))                       # CPU
    assert T.nonlocal_channel_supported(torch.rand(1, 256, 1, 1, device="cuda")) and T.nonlocal_channel_supported(torch.rand(2, 1, 1, 1, device="cuda"))
    x, y = torch.rand(2, 4, 8, 8, device="cuda").requires_grad_(True), torch.rand(1, 4, 8, 8, device="cuda")
    assert not type(fusion.attention_fusion(x, y, 'sca', 'nl', 'nl').grad_fn).__name__.startswith("_FusionJoinFn")   # shapes differ: broadcast by the composition


def test_peak_memory_of_the_fusion_layer_is_below_the_compositions(monkeypatch):
    """forward + backward of attention_fusion(.., 'sca', 'nl', 'nl') at 1 x 112 x 128 x 128: the peak extra memory of the HIP path against that of
    the composition, both measured here"""
    from core.fusion import attention_fusion
    shape = (1, 112, 128, 128)
    rng = np.random.default_rng(2660)
    arrs = [(rng.random(shape) ** 2).astype(np.float32) for _ in range(2)] + [rng.standard_normal(shape).astype(np.float32)]
    peaks = {}
    for impl in ("torch", "hip"):
        monkeypatch.setenv("MMIF_NONLOCAL", impl)
        t1, t2, g = (torch.from_numpy(a).cuda() for a in arrs)
        t1.requires_grad_(True), t2.requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        o = attention_fusion(t1, t2, 'sca', 'nl', 'nl')
        o.backward(g)
        torch.cuda.synchronize()
        peaks[impl] = torch.cuda.max_memory_allocated() - before
        assert torch.isfinite(o).all() and torch.isfinite(t1.grad).all() and torch.isfinite(t2.grad).all()
        del o, t1, t2, g
    one = int(np.prod(shape)) * 4
    print(f"F26 peak extra memory, fusion layer fwd + bwd {shape}: composition {peaks['torch'] / 2**20:.1f} MiB, HIP {peaks['hip'] / 2**20:.1f} MiB "
          f"(one map: {one / 2**20:.1f} MiB)")
    assert peaks["hip"] < peaks["torch"], peaks
