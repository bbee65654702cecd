"""Golden F24 on the CPU: the numpy float64 restatements of tests/attention_cases.py (explicit backward formulas, the ones csrc/attention.hip,
csrc/glue.hip and the patch conv of csrc/conv_general.hip implement) against the reference's own float64 results, the reference's
state_dict key lists against our modules, and the argument validation of the new entry points (which runs before any launch, so it
needs no GPU)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import attention_cases as AC

TOL = 1e-11   # float64 against float64: different summation orders only


@pytest.fixture(scope="module")
def gold():
    return np.load(AC.F24)


@pytest.fixture(scope="module")
def manifest():
    with open(AC.F24_MANIFEST) as f:
        return json.load(f)


ZERO_BY_DESIGN = sorted(["core|m1|dq", "core|m1|dk"] + [f"ln|c1_w{w}_b{b}|{t}" for w in (0, 1) for b in (0, 1) for t in ("dx", ) + (("y", ) if not b else ()) + (("weight", ) if w else ())])


def pin(gold, key, full):
    full = np.asarray(full, np.float64).reshape(-1)
    if key in ZERO_BY_DESIGN:   # identically zero in the reference (listed in the manifest, not stored): rounding residue at most
        assert key not in gold.files and np.abs(full).max() <= 1e-12, key
        return
    ref = gold[key]
    got = full[AC.sample_index(full.size)]
    assert got.shape == ref.shape, key
    scale = max(np.abs(ref).max(), 1e-300)
    assert np.abs(got - ref).max() <= TOL * max(scale, 1.0), (key, np.abs(got - ref).max(), scale)


def test_fixture_is_small_and_complete(gold, manifest):
    assert os.path.getsize(AC.F24) <= 802015, "f24_attention.npz must not outgrow the largest older fixture (f3_conv.npz)"
    assert sorted(gold.files) == sorted(manifest["sizes"])
    for key, size in manifest["sizes"].items():
        assert gold[key].size == AC.sample_index(size).size, key
    assert sorted(manifest["zero_in_the_reference"]) == ZERO_BY_DESIGN


@pytest.mark.parametrize("name", list(AC.CORE_CASES))
def test_core_restatement_matches_the_reference(name, gold):
    q, k, v, go, heads, scale = AC.core_inputs(name)
    ref = AC.sra_f64(q, k, v, heads, scale, go)
    for key in ("o", "dq", "dk", "dv"):
        pin(gold, f"core|{name}|{key}", ref[key])


def test_core_edge_properties():
    q, k, v, go, heads, scale = AC.core_inputs("m1")
    ref = AC.sra_f64(q, k, v, heads, scale, go)
    assert np.array_equal(ref["o"], np.broadcast_to(v.astype(np.float64), ref["o"].shape))   # softmax of one key: o = v
    tiny = 1e-12 * np.abs(ref["dv"]).max()   # dq = dk = 0 up to the rounding of go . v - go . o
    assert np.abs(ref["dq"]).max() <= tiny and np.abs(ref["dk"]).max() <= tiny
    q, k, v, go, heads, scale = AC.core_inputs("hot")
    assert AC.sra_f64(q, k, v, heads, scale)["zmax"] >= 100.0   # exp overflows in fp32 without a maximum


@pytest.mark.parametrize("name", list(AC.ATTN_CASES))
def test_attention_restatement_matches_the_reference(name, gold):
    x, g, params, (in_ch, out_ch, kw) = AC.attn_case(name)
    ref = AC.attention_f64(x, params, in_ch, out_ch, kw, g)
    keys = [k.split("|")[2] for k in gold.files if k.startswith(f"attn|{name}|")]
    assert sorted(keys) == sorted(ref), (keys, sorted(ref))
    for key in keys:
        pin(gold, f"attn|{name}|{key}", ref[key])


@pytest.mark.parametrize("name", list(AC.BLOCK_CASES))
def test_block_restatement_matches_the_reference(name, gold):
    x, g, params = AC.block_case(name)
    ref = AC.block_f64(name, x, params, g)
    keys = [k.split("|")[2] for k in gold.files if k.startswith(f"block|{name}|")]
    assert sorted(keys) == sorted(ref), (keys, sorted(ref))
    for key in keys:
        pin(gold, f"block|{name}|{key}", ref[key])


@pytest.mark.parametrize("s", AC.PATCH_S)
def test_patch_conv_restatement_matches_the_reference(s, gold):
    for bias in (False, True):
        for relu6 in (False, True):
            x, w, b, g = AC.patch_case(s, bias)
            ref = AC.patch_f64(x, w, b, g, relu6)
            name = f"s{s}_b{int(bias)}_r{int(relu6)}"
            pin(gold, f"patch|{name}|y", ref["y"])
            pin(gold, f"patch|{name}|dx", ref["dx"])
            pin(gold, f"patch|{name}|layers.0.weight", ref["dw"])
            if bias:
                pin(gold, f"patch|{name}|layers.0.bias", ref["db"])
            h, wd = x.shape[2:]
            assert np.all(ref["dx"][:, :, (h // s) * s:] == 0.0) and np.all(ref["dx"][:, :, :, (wd // s) * s:] == 0.0)


@pytest.mark.parametrize("c", AC.LN_C)
def test_layernorm_restatement_matches_the_reference(c, gold):
    for scale in (False, True):
        for bias in (False, True):
            x, w, b, g = AC.ln_case(c)
            ref = AC.ln_f64(x, w if scale else None, b if bias else None, g)
            name = f"c{c}_w{int(scale)}_b{int(bias)}"
            pin(gold, f"ln|{name}|y", ref["y"])
            pin(gold, f"ln|{name}|dx", ref["dx"])
            if scale:
                pin(gold, f"ln|{name}|weight", ref["dw"])
            if bias:
                pin(gold, f"ln|{name}|bias", ref["db"])


def test_join_restatement_matches_the_reference(gold):
    a, b, ls, rs, g = AC.join_case()
    for use_ls in (False, True):
        for use_rs in (False, True):
            for relu6 in (False, True):
                ref = AC.join_f64(a, b, ls if use_ls else None, rs if use_rs else None, g, relu6)
                name = f"l{int(use_ls)}_r{int(use_rs)}_a{int(relu6)}"
                for key in ("y", "da", "db") + (("dls", ) if use_ls else ()) + (("drs", ) if use_rs else ()):
                    pin(gold, f"join|{name}|{key}", ref[key])
    y = AC.join_f64(a, b, ls, rs, g, True)["y"]
    assert (y == 0.0).any() and (y == 6.0).any()   # ReLU6 clips at both ends in this case


def test_state_dict_keys_match_the_reference(manifest):
    import torch
    from core import block as B
    ours = {"transformer32": B.TransformerBlock(32, 32),
            "metaformer16": B.MetaFormerBlock(16, 16, token_mixer=B.Attention, layer_scale=1e-2, res_scale=1.0)}
    for name, mod in ours.items():
        assert list(mod.state_dict().keys()) == manifest["state_dict_keys"][name], name
        shapes = AC.block_param_shapes(name)
        sd = mod.state_dict()
        for key, shape in shapes.items():
            assert tuple(sd[key].shape) == tuple(shape), (name, key)
        rest = [k for k in sd if k not in shapes]
        assert all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in rest), rest
    # initialisation as in the reference: Scale at its init value, LayerNorm weight 1, BatchNorm the torch default
    m = ours["metaformer16"]
    assert torch.equal(m.layer_scale1.scale, torch.full((16, ), 1e-2)) and torch.equal(m.res_scale2.scale, torch.ones(16))
    assert torch.equal(m.norm1.weight, torch.ones(16, 1, 1)) and m.norm1.bias is None
    assert isinstance(ours["transformer32"].norm1, torch.nn.BatchNorm2d)
    for name in ("Attention", "FFN", "Scale", "LayerNorm", "MetaFormerBlock", "ConvFormerBlock", "Res2FormerBlock", "TransformerBlock", "TransitionBlock"):
        assert name in B.__all__ and hasattr(B, name), name


def test_constructor_defaults_follow_the_reference():
    from core import block as B
    for in_ch, heads, d, sr in ((16, 1, 16, 16), (32, 2, 16, 8), (64, 4, 16, 4), (128, 8, 16, 2), (256, 16, 16, 1), (40, 2, 20, 8)):
        a = B.Attention(in_ch, in_ch)
        assert (a.num_heads, a.head_dim, a.sr_ratio, a.att_dim) == (heads, d, sr, heads * d)
        assert a.scale == d ** -0.5
    assert isinstance(B.Attention(32, 32, down_mode='avgpool').pool, torch_nn().AvgPool2d)
    # the new ConvLayer route: depth-wise kernel == stride conv; everything else keeps its route
    assert B.Attention(32, 32).pool._patch and B.Attention(32, 32).pool._epilogue
    t = B.TransitionBlock(16, 32)
    assert t.layers[0]._patch and not t.layers[1]._patch
    assert not B.ConvLayer(16, 16, ksize=3, groups=16)._patch and B.ConvLayer(16, 16, ksize=3, groups=16)._depthwise
    assert not B.ConvLayer(16, 16, ksize=3, stride=2)._patch and B.ConvLayer(16, 16, ksize=3, stride=2)._gen
    assert not B.ConvLayer(16, 16, ksize=17, stride=17, padding=0, groups=16)._patch   # beyond the kernel's range: the stock module


def torch_nn():
    import torch.nn as nn
    return nn


def test_stock_composition_of_the_core_matches_float64_on_the_cpu():
    """$MMIF_SRA=torch and every unsupported shape run this composition: same layout, same results"""
    import torch
    from core import block as B
    for name in ("h2_m6", "d8", "hot"):
        q, k, v, go, heads, scale = AC.core_inputs(name)
        ref = AC.sra_f64(q, k, v, heads, scale, go)
        ts = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (q, k, v)]
        o = B.sra_core(*ts, heads, scale)   # CPU tensors: the composition
        o.backward(torch.from_numpy(go.astype(np.float64)))
        for got, key in zip([o.detach()] + [t.grad for t in ts], ("o", "dq", "dk", "dv")):
            assert np.abs(got.numpy() - ref[key]).max() <= 1e-9 * np.abs(ref[key]).max(), (name, key)


def test_switch_validates(monkeypatch):
    from core import block as B
    monkeypatch.setenv("MMIF_SRA", "cuda")
    with pytest.raises(ValueError):
        B._sra_impl()
    monkeypatch.setenv("MMIF_SRA", "torch")
    assert B._sra_impl() == "torch"
    monkeypatch.delenv("MMIF_SRA")
    assert B._sra_impl() == "hip"


def test_new_c_abi_exists_and_validates_before_any_launch():
    from mmif._lib import lib
    for name in ("mmif_sra_workspace", "mmif_sra_fwd", "mmif_sra_bwd", "mmif_patchconv_fwd", "mmif_patchconv_dgrad", "mmif_patchconv_wgrad_workspace",
                 "mmif_patchconv_wgrad", "mmif_layernorm_fwd", "mmif_layernorm_bwd", "mmif_glue_workspace", "mmif_join_fwd", "mmif_join_bwd"):
        assert hasattr(lib, name), name
    one = C.c_void_p(8)   # never dereferenced: validation fails first
    assert lib.mmif_sra_workspace(1, 1, 16, 256, 4) > 0
    for b, heads, d, n, m, word in ((1, 1, 20, 64, 4, b"8, 16 or 32"), (1, 17, 16, 64, 4, b"heads * d <= 256"), (1, 1, 16, 0, 4, b"1 <= n, m"),
                                    (1, 1, 16, 64, 0, b"1 <= n, m"), (70000, 1, 16, 64, 4, b"b * heads <= 65535")):
        assert lib.mmif_sra_workspace(b, heads, d, n, m) == 0
        assert word in lib.mmif_last_error() and b"mmif_sra_workspace" in lib.mmif_last_error()
        assert lib.mmif_sra_fwd(one, one, one, one, one, b, heads, d, n, m, 0.25, None) != 0
        assert b"mmif_sra_fwd" in lib.mmif_last_error()
        assert lib.mmif_sra_bwd(one, one, one, one, one, one, one, one, one, b, heads, d, n, m, 0.25, one, 1 << 30, None) != 0
        assert b"mmif_sra_bwd" in lib.mmif_last_error()
    assert lib.mmif_sra_bwd(one, one, one, one, one, one, one, one, one, 1, 1, 16, 256, 4, 0.25, one, 16, None) != 0   # too small a workspace
    assert b"workspace" in lib.mmif_last_error()
    assert lib.mmif_patchconv_fwd(one, one, None, one, 1, 4, 32, 32, 17, None) != 0 and b"[2, 16]" in lib.mmif_last_error()
    assert lib.mmif_patchconv_fwd(one, one, None, one, 1, 4, 7, 32, 8, None) != 0 and b"smaller than the kernel" in lib.mmif_last_error()
    assert lib.mmif_patchconv_wgrad_workspace(4, 1) == 0 and lib.mmif_patchconv_wgrad_workspace(4, 16) == 64 * 4 * 257 * 4
    assert lib.mmif_layernorm_fwd(one, None, None, one, one, 1, 257, 16, 1e-6, None) != 0 and b"256 channels" in lib.mmif_last_error()
    assert lib.mmif_join_fwd(one, one, None, None, one, 1, 4, 16, 1, None) != 0 and b"ReLU6" in lib.mmif_last_error()
    assert lib.mmif_join_bwd(one, one, None, None, one, one, one, one, one, None, 1, 4, 16, 0, None, 0, None) != 0   # dls without ls
    assert lib.mmif_glue_workspace(4) == 64 * 4 * 2 * 4 and lib.mmif_glue_workspace(0) == 0
    assert lib.mmif_join_bwd(one, one, one, None, one, one, one, one, one, None, 1, 4, 16, 0, one, 16, None) != 0 and b"workspace" in lib.mmif_last_error()
    assert lib.mmif_layernorm_bwd(one, one, None, one, one, one, None, 1, 4, 16, None, 0, None) != 0 and b"workspace" in lib.mmif_last_error()
