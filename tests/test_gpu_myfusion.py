"""MixConvBlock, MixFormerBlock, DCBlock, Decoder, LSDecoder and MyFusion on the device (fp32) against golden F25 -- the reference's own
modules in float64 (tests/golden/make_golden_myfusion.py; cases in tests/myfusion_cases.py).

Tolerances are the project's for the same kind of comparison: blocks as test_res2_conv_block_vs_golden (y 2e-5, dx 5e-5, parameters 1e-4;
2e-3 where a BatchNorm's batch statistics are inside, as test_gpu_general_conv.py's norm layers), models as test_n4_nested_models_vs_golden
(image 2e-4, gradients 2e-3 through close_digest).  A parameter gets no gradient exactly where the manifest says the reference's does not."""
import json

import numpy as np
import pytest
import torch

import attention_cases as AC
import myfusion_cases as FC
from gpu_util import close, close_digest, dtype_ctx
from oracle import fusion_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def f25():
    return np.load(FC.F25), json.load(open(FC.F25_MANIFEST))


def _load(mod, seed):
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in FC.closed_form_state(mod, seed).items()})
    return mod.to(DEV)


def _sampled(a):
    a = np.asarray(a).reshape(-1)
    return a[AC.sample_index(a.size)]


def _check_params(mod, g, man, name, sep, tol, digest):
    no_grad = set(man["no_gradient"][name])
    for k, p in mod.named_parameters():
        if k in no_grad:
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        if digest:
            close_digest(p.grad.cpu().numpy(), g[f"{name}{sep}dp_{k}"], tol, k)
        else:
            close(_sampled(p.grad.cpu().numpy()), g[f"{name}{sep}dp_{k}"], tol, k)
    assert no_grad <= {k for k, _ in mod.named_parameters()} | {f"x{i}" for i in range(4)}


@pytest.mark.parametrize("name", list(FC.BLOCK_CASES))
def test_block_vs_golden(name, f25):
    import core.block as B
    g, man = f25
    seed, bn = FC.BLOCK_CASES[name][5], FC.BLOCK_CASES[name][6]
    ty, tx, tp = (2e-3, 2e-3, 2e-3) if bn else (2e-5, 5e-5, 1e-4)
    with dtype_ctx("fp32"):
        blk = _load(FC.build_block(B, name), seed)
        x = torch.from_numpy(FC.block_input(name)).to(DEV).requires_grad_(True)
        y = blk(x)
        y.backward(torch.from_numpy(FC.upstream(y.shape)).to(DEV))
    close(_sampled(y.detach().cpu().numpy()), g[f"{name}|y"], ty, "y")
    close(_sampled(x.grad.cpu().numpy()), g[f"{name}|dx"], tx, "dx")
    _check_params(blk, g, man, name, "|", tp, False)


@pytest.mark.parametrize("name", list(FC.DECODER_CASES))
def test_decoder_vs_golden(name, f25):
    import core.block as B
    g, man = f25
    with dtype_ctx("fp32"):
        dec = _load(FC.build_decoder(B, name), FC.DECODER_CASES[name][1])
        feats = [torch.from_numpy(f).to(DEV).requires_grad_(True) for f in FC.pyramid_inputs()]
        y = dec(feats)
        y.backward(torch.from_numpy(FC.upstream(y.shape)).to(DEV))
    close(_sampled(y.detach().cpu().numpy()), g[f"{name}|y"], 2e-5, "y")
    for i, f in enumerate(feats):
        if f"x{i}" in man["no_gradient"][name]:
            assert f.grad is None, i
        else:
            close(_sampled(f.grad.cpu().numpy()), g[f"{name}|dx{i}"], 5e-5, f"dx{i}")
    _check_params(dec, g, man, name, "|", 1e-4, False)


@pytest.mark.parametrize("shape", FC.SHAPES, ids=lambda s: f"{s[0]}x{s[2]}x{s[3]}")
@pytest.mark.parametrize("cfg", list(FC.CONFIGS))
def test_myfusion_vs_golden(cfg, shape, f25):
    import core.block as B
    import core.model as M
    g, man = f25
    tag = FC.tag(cfg, shape)
    with dtype_ctx("fp32"):
        model = _load(FC.build_model(M, B, cfg), FC.CONFIGS[cfg][1])
        i1, i2 = (torch.from_numpy(a).to(DEV) for a in FC.model_inputs(shape))
        y = model(i1, i2)
        y.backward(torch.from_numpy(FC.model_upstream(y.shape)).to(DEV))
    yn = y.detach().cpu().numpy()
    O.assert_alive(yn, tag, lo=FC.ALIVE[0], hi=FC.ALIVE[1])
    print(f"{tag}: positive {float((yn > 0).mean()):.4f} (reference {man['positive_fraction'][tag]})")
    close(_sampled(yn), g[tag + "__y"], 2e-4, "fused image")
    _check_params(model, g, man, tag, "__", 2e-3, True)
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert float(p.grad.abs().max()) > 0.0, f"{k}: all-zero gradient"
