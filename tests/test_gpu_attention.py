"""The spatial-reduction attention core (csrc/attention.hip), Attention, TransformerBlock / MetaFormerBlock and the small kernels under
them (depth-wise patch conv, channel LayerNorm, residual join) against golden F24 (the reference in float64) and the numpy float64
restatements of tests/attention_cases.py.

Tolerance.  Errors are max |got - ref| / max |ref| per tensor.  TORCH_ERR below is the error E of the stock fp32 torch composition
against the same float64 values, measured on an MI355X: $MMIF_SRA=torch for the core, Attention and the blocks, the stock torch modules
for the small kernels.  The HIP path's bar per case and tensor is  max(1e-4, 4 * E)  -- 1e-4 is the project's fp32 bar, the factor 4
allows for a different but equally legitimate summation order through exp.  The measured E are 8e-9 ... 5.3e-6, so the bar is 1e-4 for
every case and tensor; the HIP path measured at most 8.3e-6 on the same cases.  A case without an entry would be held to the 1e-4 floor
itself.  Every test prints the live figures of both paths before it asserts (DESIGN.md section 4.6 records them).  dq and dk of the
one-key case, 0 in the reference, are held to max |got| <= 1e-4 * max |dv_ref|; a tensor that is identically zero in the reference
elsewhere (LayerNorm over one channel) is held to max |got| <= the bar."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import attention_cases as AC

pytestmark = pytest.mark.gpu

FP32_BAR = 1e-4
# '<group>|<case>' -> {tensor: error of the stock fp32 composition against float64}, measured (MI355X, ROCm torch)
TORCH_ERR = {
    "attn|a128": {"dx": 7.013e-07, "k.layers.0.weight": 2.777e-07, "pool.layers.0.weight": 4.590e-07, "proj.layers.0.weight": 2.881e-07, "q.layers.0.weight": 4.797e-07, "v.layers.0.weight": 4.007e-07, "y": 5.435e-07},
    "attn|a16": {"dx": 8.814e-07, "k.layers.0.weight": 4.663e-07, "pool.layers.0.weight": 9.120e-07, "proj.layers.0.weight": 4.891e-07, "q.layers.0.weight": 2.507e-07, "v.layers.0.weight": 1.035e-06, "y": 2.637e-07},
    "attn|a256": {"dx": 5.747e-07, "k.layers.0.weight": 7.007e-07, "proj.layers.0.weight": 3.879e-07, "q.layers.0.weight": 6.259e-07, "v.layers.0.weight": 5.608e-07, "y": 7.232e-07},
    "attn|a32": {"dx": 2.862e-07, "k.layers.0.weight": 2.847e-07, "pool.layers.0.weight": 3.557e-07, "proj.layers.0.weight": 3.616e-07, "q.layers.0.weight": 5.771e-07, "v.layers.0.weight": 4.037e-07, "y": 2.380e-07},
    "attn|a32_avg": {"dx": 4.159e-07, "k.layers.0.weight": 2.967e-07, "proj.layers.0.weight": 3.683e-07, "q.layers.0.weight": 3.857e-07, "v.layers.0.weight": 2.009e-07, "y": 4.420e-07},
    "attn|a32_h4": {"dx": 2.578e-07, "k.layers.0.weight": 2.684e-07, "pool.layers.0.weight": 2.346e-07, "proj.layers.0.weight": 3.264e-07, "q.layers.0.weight": 2.947e-07, "v.layers.0.weight": 2.134e-07, "y": 3.606e-07},
    "attn|a40": {"dx": 4.109e-07, "k.layers.0.weight": 4.607e-07, "pool.layers.0.weight": 4.045e-07, "proj.layers.0.weight": 4.092e-07, "q.layers.0.weight": 6.229e-07, "v.layers.0.weight": 4.400e-07, "y": 3.147e-07},
    "attn|a48_sr5": {"dx": 2.617e-07, "k.layers.0.weight": 2.424e-07, "pool.layers.0.weight": 2.278e-07, "proj.layers.0.weight": 3.809e-07, "q.layers.0.weight": 2.677e-07, "v.layers.0.weight": 2.118e-07, "y": 2.816e-07},
    "attn|a64_48": {"dx": 3.418e-07, "k.layers.0.weight": 3.973e-07, "pool.layers.0.weight": 3.930e-07, "proj.layers.0.weight": 3.331e-07, "q.layers.0.weight": 5.158e-07, "v.layers.0.weight": 2.348e-07, "y": 4.098e-07},
    "block|metaformer16": {"dx": 1.117e-07, "ffn.layers.0.layers.0.weight": 2.354e-07, "ffn.layers.1.layers.0.weight": 1.538e-07, "ffn.layers.2.layers.0.weight": 2.249e-07, "layer_scale1.scale": 3.312e-07, "layer_scale2.scale": 3.077e-07, "norm1.weight": 4.255e-07, "norm2.weight": 1.416e-07, "res_scale1.scale": 9.457e-08, "res_scale2.scale": 7.100e-08, "token_mixer.k.layers.0.weight": 5.557e-07, "token_mixer.pool.layers.0.weight": 6.812e-07, "token_mixer.proj.layers.0.weight": 3.647e-07, "token_mixer.q.layers.0.weight": 3.218e-07, "token_mixer.v.layers.0.weight": 8.328e-07, "y": 9.841e-08},
    "block|transformer32": {"dx": 2.698e-07, "ffn.layers.0.layers.0.weight": 2.733e-07, "ffn.layers.1.layers.0.weight": 2.406e-07, "ffn.layers.2.layers.0.weight": 3.196e-07, "norm1.bias": 3.213e-07, "norm1.weight": 2.321e-07, "norm2.bias": 3.657e-07, "norm2.weight": 3.691e-07, "token_mixer.k.layers.0.weight": 3.117e-07, "token_mixer.pool.layers.0.weight": 3.754e-07, "token_mixer.proj.layers.0.weight": 2.960e-07, "token_mixer.q.layers.0.weight": 4.043e-07, "token_mixer.v.layers.0.weight": 4.159e-07, "y": 1.624e-07},
    "core|d32": {"dk": 3.741e-07, "dq": 2.425e-07, "dv": 3.006e-07, "o": 1.927e-07},
    "core|d8": {"dk": 2.205e-07, "dq": 1.872e-07, "dv": 2.393e-07, "o": 1.660e-07},
    "core|h2_m6": {"dk": 2.547e-07, "dq": 1.517e-07, "dv": 3.221e-07, "o": 1.482e-07},
    "core|h3_m17": {"dk": 1.601e-07, "dq": 2.380e-07, "dv": 1.454e-07, "o": 2.481e-07},
    "core|hot": {"dk": 4.073e-06, "dq": 5.110e-06, "dv": 1.592e-06, "o": 5.314e-06},
    "core|level3": {"dk": 8.022e-07, "dq": 5.384e-07, "dv": 6.248e-07, "o": 6.369e-07},
    "core|m1": {"dv": 4.343e-07, "o": 0.000e+00},
    "core|m5000": {"dk": 6.278e-07, "dq": 9.064e-07, "dv": 4.426e-07, "o": 6.991e-07},
    "core|n740_m2": {"dk": 4.316e-07, "dq": 1.738e-07, "dv": 4.557e-07, "o": 1.474e-07},
    "core|sr1_h16": {"dk": 2.193e-07, "dq": 2.638e-07, "dv": 2.839e-07, "o": 2.657e-07},
    "join|l0_r0_a0": {"da": 0.000e+00, "db": 0.000e+00, "y": 5.368e-08},
    "join|l0_r0_a1": {"da": 0.000e+00, "db": 0.000e+00, "y": 3.974e-08},
    "join|l0_r1_a0": {"da": 0.000e+00, "db": 2.830e-08, "drs": 1.544e-07, "y": 5.019e-08},
    "join|l0_r1_a1": {"da": 0.000e+00, "db": 3.224e-08, "drs": 7.479e-08, "y": 6.679e-08},
    "join|l1_r0_a0": {"da": 2.726e-08, "db": 0.000e+00, "dls": 7.791e-08, "y": 4.656e-08},
    "join|l1_r0_a1": {"da": 3.112e-08, "db": 0.000e+00, "dls": 6.273e-08, "y": 9.073e-08},
    "join|l1_r1_a0": {"da": 2.726e-08, "db": 2.830e-08, "dls": 7.791e-08, "drs": 1.544e-07, "y": 4.781e-08},
    "join|l1_r1_a1": {"da": 3.112e-08, "db": 3.224e-08, "dls": 3.867e-08, "drs": 1.435e-07, "y": 8.333e-08},
    "ln|c16_w0_b0": {"dx": 1.051e-07, "y": 9.370e-08},
    "ln|c16_w0_b1": {"db": 6.855e-08, "dx": 1.051e-07, "y": 9.865e-08},
    "ln|c16_w1_b0": {"dw": 1.295e-07, "dx": 1.344e-07, "y": 7.354e-08},
    "ln|c16_w1_b1": {"db": 6.855e-08, "dw": 1.295e-07, "dx": 1.344e-07, "y": 9.738e-08},
    "ln|c1_w0_b0": {"dx": 0.000e+00, "y": 0.000e+00},
    "ln|c1_w0_b1": {"db": 2.939e-07, "dx": 0.000e+00, "y": 0.000e+00},
    "ln|c1_w1_b0": {"dw": 0.000e+00, "dx": 0.000e+00, "y": 0.000e+00},
    "ln|c1_w1_b1": {"db": 2.939e-07, "dw": 0.000e+00, "dx": 0.000e+00, "y": 0.000e+00},
    "ln|c256_w0_b0": {"dx": 1.308e-07, "y": 1.096e-07},
    "ln|c256_w0_b1": {"db": 6.984e-08, "dx": 1.308e-07, "y": 1.069e-07},
    "ln|c256_w1_b0": {"dw": 9.290e-08, "dx": 1.168e-07, "y": 9.738e-08},
    "ln|c256_w1_b1": {"db": 6.984e-08, "dw": 9.290e-08, "dx": 1.168e-07, "y": 9.694e-08},
    "ln|c7_w0_b0": {"dx": 1.478e-07, "y": 1.121e-07},
    "ln|c7_w0_b1": {"db": 6.857e-08, "dx": 1.478e-07, "y": 9.968e-08},
    "ln|c7_w1_b0": {"dw": 6.055e-08, "dx": 8.032e-08, "y": 1.372e-07},
    "ln|c7_w1_b1": {"db": 6.857e-08, "dw": 6.055e-08, "dx": 8.032e-08, "y": 1.208e-07},
    "patch|s16_b0_r0": {"dw": 4.275e-08, "dx": 2.812e-08, "y": 3.586e-08},
    "patch|s16_b0_r1": {"dw": 3.086e-08, "dx": 2.767e-08, "y": 3.586e-08},
    "patch|s16_b1_r0": {"db": 4.600e-08, "dw": 3.764e-08, "dx": 2.938e-08, "y": 3.686e-08},
    "patch|s16_b1_r1": {"db": 2.852e-08, "dw": 5.238e-08, "dx": 3.939e-08, "y": 4.747e-08},
    "patch|s2_b0_r0": {"dw": 3.213e-08, "dx": 2.816e-08, "y": 2.386e-08},
    "patch|s2_b0_r1": {"dw": 1.845e-08, "dx": 2.901e-08, "y": 2.091e-08},
    "patch|s2_b1_r0": {"db": 1.903e-08, "dw": 3.836e-08, "dx": 3.304e-08, "y": 2.690e-08},
    "patch|s2_b1_r1": {"db": 5.018e-08, "dw": 1.418e-08, "dx": 4.276e-08, "y": 2.690e-08},
    "patch|s5_b0_r0": {"dw": 3.793e-08, "dx": 4.292e-08, "y": 1.751e-08},
    "patch|s5_b0_r1": {"dw": 2.736e-08, "dx": 4.292e-08, "y": 8.362e-09},
    "patch|s5_b1_r0": {"db": 3.775e-08, "dw": 4.788e-08, "dx": 3.327e-08, "y": 3.925e-08},
    "patch|s5_b1_r1": {"db": 9.651e-08, "dw": 4.788e-08, "dx": 3.595e-08, "y": 3.925e-08},
    "patch|s8_b0_r0": {"dw": 4.698e-08, "dx": 3.008e-08, "y": 3.558e-08},
    "patch|s8_b0_r1": {"dw": 4.758e-08, "dx": 3.008e-08, "y": 3.748e-08},
    "patch|s8_b1_r0": {"db": 5.771e-08, "dw": 3.477e-08, "dx": 2.892e-08, "y": 5.788e-08},
    "patch|s8_b1_r1": {"db": 4.386e-08, "dw": 3.068e-08, "dx": 3.560e-08, "y": 6.083e-08},
}


def bar(group, case, key):
    """max(1e-4, 4 E); a tensor without a measured E gets the floor itself, the strictest value the rule can give"""
    return max(FP32_BAR, 4.0 * TORCH_ERR.get(f"{group}|{case}", {}).get(key, 0.0))


def err(got, ref):
    """max |got - ref| / max |ref|; where the reference is identically zero (LayerNorm over one channel), max |got|"""
    ref = np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (scale if scale > 0.0 else 1.0))


def cuda(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(AC.F24)


def check(group, case, figs, ref, extra=None):
    """print both paths' figures, then hold the HIP path to the bar: against the full restatement and against the fixture sample"""
    g = gold()
    for key in ref:
        line = []
        for impl, res in figs.items():
            full = err(res[key], ref[key])
            gk = f"{group}|{case}|{key}"
            samp = err(np.asarray(res[key]).reshape(-1)[AC.sample_index(np.asarray(res[key]).size)], g[gk]) if gk in g.files else float("nan")
            line.append(f"{impl} {full:.3e} (fixture sample {samp:.3e})")
            if impl == "hip":
                hip = (full, samp)
        print(f"F24 {group} {case} {key}: " + "  ".join(line) + f"  bar {bar(group, case, key):.1e}")
        assert hip[0] <= bar(group, case, key), (group, case, key, hip)
        assert not hip[1] > bar(group, case, key), (group, case, key, hip)


# ------------------------------------------------------------------ the core operator
@functools.lru_cache(maxsize=None)
def core_ref(name):
    q, k, v, go, heads, scale = AC.core_inputs(name)
    return AC.sra_f64(q, k, v, heads, scale, go)


def run_core(name, impl, monkeypatch):
    from core import block as B
    monkeypatch.setenv("MMIF_SRA", impl)
    q, k, v, go, heads, scale = AC.core_inputs(name)
    ts = [cuda(t, True) for t in (q, k, v)]
    o = B.sra_core(*ts, heads, scale)
    if impl == "hip":
        assert type(o.grad_fn).__name__.startswith("_SraFn"), "the HIP kernels must run this shape"
    o.backward(cuda(go))
    torch.cuda.synchronize()
    return {"o": host(o), "dq": host(ts[0].grad), "dk": host(ts[1].grad), "dv": host(ts[2].grad)}


@pytest.mark.parametrize("name", list(AC.CORE_CASES))
def test_core_vs_float64(name, monkeypatch):
    full = core_ref(name)
    figs = {impl: run_core(name, impl, monkeypatch) for impl in ("hip", "torch")}
    assert all(np.isfinite(a).all() for a in figs["hip"].values())
    keys = ("o", "dq", "dk", "dv")
    if name == "m1":   # softmax of one key: dq = dk = 0 in the reference
        lim = 1e-4 * np.abs(full["dv"]).max()
        for key in ("dq", "dk"):
            print(f"F24 core m1 {key}: hip max |got| {np.abs(figs['hip'][key]).max():.3e}  torch {np.abs(figs['torch'][key]).max():.3e}  limit {lim:.3e}")
            assert np.abs(figs["hip"][key]).max() <= lim
        keys = ("o", "dv")
    check("core", name, figs, {k: full[k] for k in keys})


def test_core_is_bit_identical_run_to_run(monkeypatch):
    a, b = run_core("level3", "hip", monkeypatch), run_core("level3", "hip", monkeypatch)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_core_peak_memory_stays_below_half_an_energy_tensor(monkeypatch):
    """the capability itself: forward + backward at (1, 1, 16, 65536, 256) allocate less than 32 MiB above the operands -- half of ONE
    64 MiB energy tensor; the composition holds several"""
    from core import block as B
    monkeypatch.delenv("MMIF_SRA", raising=False)
    n, m = 65536, 256
    gen = torch.Generator(device="cuda").manual_seed(24)
    q, k, v, go = (torch.randn(1, 16, s, device="cuda", generator=gen) for s in (n, m, m, n))
    for t in (q, k, v):
        t.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    o = B.sra_core(q, k, v, 1, 0.25)
    o.backward(go)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"F24 peak extra memory fwd + bwd (1, 1, 16, 65536, 256): {peak / 2**20:.1f} MiB (one energy tensor: {n * m * 4 / 2**20:.0f} MiB)")
    assert all(torch.isfinite(t).all() for t in (o, q.grad, k.grad, v.grad))
    assert peak < 32 * 2**20


def test_the_default_is_the_hip_path_and_other_head_sizes_fall_back(monkeypatch):
    from core import block as B
    monkeypatch.delenv("MMIF_SRA", raising=False)
    assert B._sra_impl() == "hip"
    q, k = torch.randn(1, 40, 50, device="cuda", requires_grad=True), torch.randn(1, 40, 3, device="cuda")
    assert not type(B.sra_core(q, k, k, 2, 20 ** -0.5).grad_fn).__name__.startswith("_SraFn")   # d = 20
    q, k = torch.randn(1, 272, 50, device="cuda", requires_grad=True), torch.randn(1, 272, 3, device="cuda")
    assert not type(B.sra_core(q, k, k, 17, 0.25).grad_fn).__name__.startswith("_SraFn")        # A = 272 > 256
    q, k = torch.randn(1, 32, 50, device="cuda", requires_grad=True), torch.randn(1, 32, 3, device="cuda")
    assert type(B.sra_core(q, k, k, 2, 0.25).grad_fn).__name__.startswith("_SraFn")
    monkeypatch.setenv("MMIF_SRA", "torch")
    assert not type(B.sra_core(q, k, k, 2, 0.25).grad_fn).__name__.startswith("_SraFn")


# ------------------------------------------------------------------ modules
def run_module(mod, params, x, g, impl, monkeypatch):
    monkeypatch.setenv("MMIF_SRA", impl)
    sd = mod.state_dict()
    assert all(k in sd for k in params)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    mod = mod.cuda().train()
    xt = cuda(x, True)
    y = mod(xt)
    y.backward(cuda(g))
    torch.cuda.synchronize()
    out = {"y": host(y), "dx": host(xt.grad)}
    out.update({k: host(p.grad) for k, p in mod.named_parameters() if p.grad is not None})
    return out


@functools.lru_cache(maxsize=None)
def attn_ref(name):
    x, g, params, (in_ch, out_ch, kw) = AC.attn_case(name)
    return AC.attention_f64(x, params, in_ch, out_ch, kw, g)


@pytest.mark.parametrize("name", list(AC.ATTN_CASES))
def test_attention_module_vs_float64(name, monkeypatch):
    """output, dx and every weight gradient; under $MMIF_SRA=torch the same cases meet the same bars"""
    from core import block as B
    x, g, params, (in_ch, out_ch, kw) = AC.attn_case(name)
    ref = attn_ref(name)
    figs = {impl: run_module(B.Attention(in_ch, out_ch, **kw), params, x, g, impl, monkeypatch) for impl in ("hip", "torch")}
    assert sorted(figs["hip"]) == sorted(ref)
    check("attn", name, figs, ref)
    for key in ref:
        assert err(figs["torch"][key], ref[key]) <= bar("attn", name, key), (name, key, "MMIF_SRA=torch")


@functools.lru_cache(maxsize=None)
def block_ref(name):
    x, g, params = AC.block_case(name)
    return AC.block_f64(name, x, params, g)


def make_block(name):
    from core import block as B
    in_ch, out_ch, _, norm, _, ls, rs, _ = AC.BLOCK_CASES[name]
    if norm == "bn":
        return B.TransformerBlock(in_ch, out_ch)
    return B.MetaFormerBlock(in_ch, out_ch, token_mixer=B.Attention, layer_scale=ls, res_scale=rs)


@pytest.mark.parametrize("name", list(AC.BLOCK_CASES))
def test_block_vs_float64(name, monkeypatch):
    """TransformerBlock(32, 32) in train mode and MetaFormerBlock(16, 16, Attention, layer_scale, res_scale): output, dx, every parameter gradient"""
    x, g, params = AC.block_case(name)
    ref = block_ref(name)
    figs = {impl: run_module(make_block(name), params, x, g, impl, monkeypatch) for impl in ("hip", "torch")}
    assert sorted(figs["hip"]) == sorted(ref)
    check("block", name, figs, ref)
    for key in ref:
        assert err(figs["torch"][key], ref[key]) <= bar("block", name, key), (name, key, "MMIF_SRA=torch")


def test_transformer_block_updates_running_statistics_and_runs_in_eval(monkeypatch):
    monkeypatch.delenv("MMIF_SRA", raising=False)
    x, g, params = AC.block_case("transformer32")
    mod = make_block("transformer32")
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    mod = mod.cuda().train()
    mod(cuda(x))
    x64 = x.astype(np.float64)
    mean, var = x64.mean(axis=(0, 2, 3)), x64.var(axis=(0, 2, 3), ddof=1)
    assert int(mod.norm1.num_batches_tracked) == 1
    assert err(host(mod.norm1.running_mean), 0.1 * mean) <= FP32_BAR and err(host(mod.norm1.running_var), 0.9 + 0.1 * var) <= FP32_BAR
    y = mod.eval()(cuda(x))
    assert y.shape == x.shape and torch.isfinite(y).all() and int(mod.norm1.num_batches_tracked) == 1


def test_attention_raises_on_inputs_smaller_than_sr_ratio():
    from core import block as B
    a = B.Attention(16, 16).cuda()   # sr_ratio 16
    with pytest.raises(RuntimeError):
        a(torch.randn(1, 16, 8, 20, device="cuda"))
    with pytest.raises(RuntimeError):
        B.Attention(16, 16, down_mode='avgpool').cuda()(torch.randn(1, 16, 20, 8, device="cuda"))


def test_transition_and_former_blocks_run(monkeypatch):
    """TransitionBlock(down_mode='stride') against float64 (patch conv s = 2 + ReLU6, then 1x1 + ReLU6); the other new blocks: shapes, finite
    gradients for every parameter the forward uses"""
    from core import block as B
    monkeypatch.delenv("MMIF_SRA", raising=False)
    rng = np.random.default_rng(2499)
    x, g = AC._f32(rng.standard_normal((2, 16, 9, 14))), AC._f32(rng.standard_normal((2, 32, 4, 7)))
    params = AC.make_params({"layers.0.layers.0.weight": (16, 1, 2, 2), "layers.1.layers.0.weight": (32, 16, 1, 1)}, 2498)
    got = run_module(B.TransitionBlock(16, 32), params, x, g, "hip", monkeypatch)
    w0, w1 = (params[k].astype(np.float64) for k in sorted(params))
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    y0 = AC.relu6_fwd(AC.patchconv_fwd(x64, w0))
    y1 = AC.relu6_fwd(AC.conv1x1_fwd(y0, w1))
    g0, dw1, _ = AC.conv1x1_bwd(y0, w1, AC.relu6_bwd(y1, g64))
    dx, dw0, _ = AC.patchconv_bwd(x64, w0, AC.relu6_bwd(y0, g0))
    for key, ref in (("y", y1), ("dx", dx), ("layers.0.layers.0.weight", dw0), ("layers.1.layers.0.weight", dw1)):
        e = err(got[key], ref)
        print(f"F24 TransitionBlock {key}: hip {e:.3e}")
        assert e <= FP32_BAR, (key, e)
    assert B.TransitionBlock(16, 32, down_mode='maxpool').cuda()(cuda(x)).shape == (2, 32, 4, 7)
    for cls in (B.ConvFormerBlock, B.Res2FormerBlock, B.TransformerBlock):
        mod = cls(16, 16).cuda().train()
        xt = torch.randn(2, 16, 20, 24, device="cuda", requires_grad=True)
        y = mod(xt)
        y.sum().backward()
        assert y.shape == xt.shape and torch.isfinite(y).all() and torch.isfinite(xt.grad).all()
        used = [p.grad for p in mod.parameters() if p.grad is not None]
        assert len(used) >= 8 and all(torch.isfinite(t).all() for t in used), cls.__name__


# ------------------------------------------------------------------ the small kernels (yardstick: the stock torch modules on the GPU)
@pytest.mark.parametrize("s", AC.PATCH_S)
def test_patch_conv_vs_float64(s):
    from core import block as B
    for bias in (False, True):
        for relu6 in (False, True):
            x, w, b, g = AC.patch_case(s, bias)
            ref = AC.patch_f64(x, w, b, g, relu6)
            if not bias:
                ref.pop("db")
            case = f"s{s}_b{int(bias)}_r{int(relu6)}"
            layer = B.ConvLayer(6, 6, ksize=s, stride=s, padding=0, groups=6, bias=bias, act=nn.ReLU6 if relu6 else None)
            assert layer._patch
            figs = {}
            for impl in ("hip", "torch"):
                xt, wt = cuda(x, True), cuda(w, True)
                bt = cuda(b, True) if bias else None
                if impl == "hip":
                    with torch.no_grad():
                        layer.layers[0].weight.copy_(torch.from_numpy(w))
                        if bias:
                            layer.layers[0].bias.copy_(torch.from_numpy(b))
                    layer = layer.cuda()
                    layer.zero_grad()
                    y = layer(xt)
                    assert "PatchConv" in type(y.grad_fn).__name__ or relu6
                    y.backward(cuda(g))
                    figs[impl] = {"y": host(y), "dx": host(xt.grad), "dw": host(layer.layers[0].weight.grad)}
                    if bias:
                        figs[impl]["db"] = host(layer.layers[0].bias.grad)
                else:
                    y = F.conv2d(xt, wt, bt, stride=s, groups=6)
                    y = F.relu6(y) if relu6 else y
                    y.backward(cuda(g))
                    figs[impl] = {"y": host(y), "dx": host(xt.grad), "dw": host(wt.grad)}
                    if bias:
                        figs[impl]["db"] = host(bt.grad)
            h, wd = x.shape[2:]
            dx = figs["hip"]["dx"]
            assert np.all(dx[:, :, (h // s) * s:] == 0.0) and np.all(dx[:, :, :, (wd // s) * s:] == 0.0)   # exactly 0 beyond the covered area
            names = {"y": "y", "dx": "dx", "dw": "layers.0.weight", "db": "layers.0.bias"}
            check_small("patch", case, figs, ref, names)


def check_small(group, case, figs, ref, names):
    g = gold()
    for key, refv in ref.items():
        if refv is None:
            continue
        e = {impl: err(res[key], refv) for impl, res in figs.items()}
        gk = f"{group}|{case}|{names[key]}"   # (a tensor that is identically zero in the reference is not in the fixture)
        samp = err(np.asarray(figs["hip"][key]).reshape(-1)[AC.sample_index(np.asarray(refv).size)], g[gk]) if gk in g.files else 0.0
        print(f"F24 {group} {case} {key}: hip {e['hip']:.3e} (fixture sample {samp:.3e})  torch {e['torch']:.3e}  bar {bar(group, case, key):.1e}")
        assert e["hip"] <= bar(group, case, key) and samp <= bar(group, case, key), (group, case, key, e, samp)


def ln_stock(x, weight, bias, eps=1e-6):
    c = x - x.mean((1, ), keepdim=True)
    y = c / torch.sqrt(c.pow(2).mean((1, ), keepdim=True) + eps)
    y = y * weight if weight is not None else y
    return y + bias if bias is not None else y


@pytest.mark.parametrize("c", AC.LN_C)
def test_layernorm_vs_float64(c):
    from core import block as B
    for scale in (False, True):
        for bias in (False, True):
            x, w, b, g = AC.ln_case(c)
            ref = AC.ln_f64(x, w if scale else None, b if bias else None, g)
            if not scale:
                ref.pop("dw")
            if not bias:
                ref.pop("db")
            case = f"c{c}_w{int(scale)}_b{int(bias)}"
            figs = {}
            for impl in ("hip", "torch"):
                xt = cuda(x, True)
                wt, bt = (cuda(w, True) if scale else None), (cuda(b, True) if bias else None)
                if impl == "hip":
                    mod = B.LayerNorm(c, scale=scale, bias=bias).cuda()
                    with torch.no_grad():
                        if scale:
                            mod.weight.copy_(wt)
                        if bias:
                            mod.bias.copy_(bt)
                    y = mod(xt)
                    assert type(y.grad_fn).__name__.startswith("_LayerNormFn")
                    wt, bt = mod.weight, mod.bias
                else:
                    y = ln_stock(xt, wt, bt)
                y.backward(cuda(g))
                figs[impl] = {"y": host(y), "dx": host(xt.grad)}
                if scale:
                    figs[impl]["dw"] = host(wt.grad)
                if bias:
                    figs[impl]["db"] = host(bt.grad)
            check_small("ln", case, figs, ref, {"y": "y", "dx": "dx", "dw": "weight", "db": "bias"})
    # another normalized_dim: the stock composition
    y = B.LayerNorm(4, normalized_dim=(1, 2, 3), scale=False).cuda()(torch.randn(2, 4, 5, 6, device="cuda", requires_grad=True))
    assert not type(y.grad_fn).__name__.startswith("_LayerNormFn")


def test_join_vs_float64():
    from core import block as B
    a, b, ls, rs, g = AC.join_case()
    for use_ls in (False, True):
        for use_rs in (False, True):
            for relu6 in (False, True):
                ref = AC.join_f64(a, b, ls if use_ls else None, rs if use_rs else None, g, relu6)
                case = f"l{int(use_ls)}_r{int(use_rs)}_a{int(relu6)}"
                figs = {}
                for impl in ("hip", "torch"):
                    at, bt = cuda(a, True), cuda(b, True)
                    lt, rt = (cuda(ls, True) if use_ls else None), (cuda(rs, True) if use_rs else None)
                    if impl == "hip":
                        y = B._JoinFn.apply(at, bt, lt, rt, B.T.ACT_RELU6 if relu6 else B.T.ACT_NONE)
                    else:
                        y = (at * lt[None, :, None, None] if use_ls else at) + (bt * rt[None, :, None, None] if use_rs else bt)
                        y = F.relu6(y) if relu6 else y
                    y.backward(cuda(g))
                    figs[impl] = {"y": host(y), "da": host(at.grad), "db": host(bt.grad)}
                    if use_ls:
                        figs[impl]["dls"] = host(lt.grad)
                    if use_rs:
                        figs[impl]["drs"] = host(rt.grad)
                check_small("join", case, figs, ref, {k: k for k in ("y", "da", "db", "dls", "drs")})
