"""Golden F24: the reference's own modules (core/block.py: Attention :355-434, LayerNorm :472-500, Scale :460-469, MetaFormerBlock
:503-540, TransformerBlock :603-617, and ConvLayer as the depth-wise kernel = stride conv) evaluated in float64 -- outputs and the autograd
gradients of sum(y * upstream) w.r.t. the input and every parameter -- on the case tables of tests/attention_cases.py (inputs and
parameters are rebuilt by the tests from seeds: the fixture holds results only).  Needs a checkout of the reference, named by
$MMIF_REFERENCE; never imported by a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_attention.py   ->   tests/golden/f24_attention.npz, f24_manifest.json

Keys: '<group>|<case>|<tensor>' (flat, at attention_cases.sample_index(size)); groups: core, attn, block, patch, ln, join.  The manifest
lists every key with its full size, the tensors that are identically zero in the reference (not stored) and the reference's state_dict key
lists of the two block cases.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attention_cases as AC  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")


def load_ref():
    assert os.path.isfile(os.path.join(REF, "core", "block.py")), "set MMIF_REFERENCE to a checkout of the reference"
    sys.path.insert(0, os.path.join(REF, "core"))   # block.py falls back to `from fusion import concat_fusion`
    spec = importlib.util.spec_from_file_location("ref_block", os.path.join(REF, "core", "block.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


OUT, SIZES, ZERO = {}, {}, []


def store(key, a):
    a = np.asarray(a, np.float64).reshape(-1)
    assert np.isfinite(a).all(), key
    if np.abs(a).max() == 0.0:   # zero by the definition of the case (dq and dk of the one-key case, LayerNorm over one channel): an
        ZERO.append(key)         # all-zero array pins nothing, so it is listed in the manifest instead of stored
        return
    SIZES[key] = int(a.size)
    OUT[key] = a[AC.sample_index(a.size)]


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def load_params(mod, params):
    sd = mod.state_dict()
    missing = [k for k in sd if k not in params and not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert not missing and all(k in sd for k in params), (missing, [k for k in params if k not in sd])
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    return mod.double()


def run_module(group, name, mod, x, g):
    xt = t64(x, True)
    y = mod(xt)
    (y * t64(g)).sum().backward()
    store(f"{group}|{name}|y", y.detach().numpy())
    store(f"{group}|{name}|dx", xt.grad.numpy())
    for k, p in mod.named_parameters():
        if p.grad is None:   # sr_ratio == 1: the pool layer exists and is never called
            assert k == "pool.layers.0.weight" and mod.sr_ratio == 1, (name, k)
            continue
        store(f"{group}|{name}|{k}", p.grad.numpy())


def main():
    R = load_ref()
    torch.set_num_threads(8)
    # the core, as the reference composes it (core/block.py:419-431)
    for name in AC.CORE_CASES:
        q, k, v, go, heads, scale = AC.core_inputs(name)
        b, a, n = q.shape
        d = a // heads
        qt, kt, vt = t64(q, True), t64(k, True), t64(v, True)
        attn = ((qt.reshape(b, heads, d, n).permute(0, 1, 3, 2) @ kt.reshape(b, heads, d, -1)) * scale).softmax(dim=-1)
        o = (attn @ vt.reshape(b, heads, d, -1).permute(0, 1, 3, 2)).transpose(2, 3).reshape(b, a, n)
        (o * t64(go)).sum().backward()
        for key, val in (("o", o.detach()), ("dq", qt.grad), ("dk", kt.grad), ("dv", vt.grad)):
            store(f"core|{name}|{key}", val.numpy())
    for name in AC.ATTN_CASES:
        x, g, params, (in_ch, out_ch, kw) = AC.attn_case(name)
        run_module("attn", name, load_params(R.Attention(in_ch, out_ch, **kw), params), x, g)
    keylists = {}
    for name, (in_ch, out_ch, _, norm, relu6, ls, rs, _) in AC.BLOCK_CASES.items():
        x, g, params = AC.block_case(name)
        mod = R.TransformerBlock(in_ch, out_ch) if norm == "bn" else R.MetaFormerBlock(in_ch, out_ch, token_mixer=R.Attention, layer_scale=ls, res_scale=rs)
        keylists[name] = list(mod.state_dict().keys())
        run_module("block", name, load_params(mod, params).train(), x, g)
    for s in AC.PATCH_S:
        for bias in (False, True):
            for relu6 in (False, True):
                x, w, b, g = AC.patch_case(s, bias)
                mod = R.ConvLayer(6, 6, ksize=s, stride=s, padding=0, groups=6, bias=bias, act=nn.ReLU6 if relu6 else None)
                p = {"layers.0.weight": w}
                if bias:
                    p["layers.0.bias"] = b
                run_module("patch", f"s{s}_b{int(bias)}_r{int(relu6)}", load_params(mod, p), x, g)
    for c in AC.LN_C:
        for scale in (False, True):
            for bias in (False, True):
                x, w, b, g = AC.ln_case(c)
                mod = R.LayerNorm(c, scale=scale, bias=bias)
                p = {}
                if scale:
                    p["weight"] = w
                if bias:
                    p["bias"] = b
                name = f"c{c}_w{int(scale)}_b{int(bias)}"
                if p:
                    run_module("ln", name, load_params(mod, p), x, g)
                else:
                    xt = t64(x, True)
                    y = mod.double()(xt)
                    (y * t64(g)).sum().backward()
                    store(f"ln|{name}|y", y.detach().numpy())
                    store(f"ln|{name}|dx", xt.grad.numpy())
    # the residual join of MetaFormerBlock.forward (core/block.py:533-538): act(layer_scale(a) + res_scale(b))
    a, b, ls, rs, g = AC.join_case()
    for use_ls in (False, True):
        for use_rs in (False, True):
            for relu6 in (False, True):
                at, bt = t64(a, True), t64(b, True)
                sl, sr = R.Scale(5).double() if use_ls else nn.Identity(), R.Scale(5).double() if use_rs else nn.Identity()
                if use_ls:
                    sl.scale.data.copy_(t64(ls))
                if use_rs:
                    sr.scale.data.copy_(t64(rs))
                y = (nn.ReLU6() if relu6 else nn.Identity())(sl(at) + sr(bt))
                (y * t64(g)).sum().backward()
                name = f"l{int(use_ls)}_r{int(use_rs)}_a{int(relu6)}"
                store(f"join|{name}|y", y.detach().numpy())
                store(f"join|{name}|da", at.grad.numpy())
                store(f"join|{name}|db", bt.grad.numpy())
                if use_ls:
                    store(f"join|{name}|dls", sl.scale.grad.numpy())
                if use_rs:
                    store(f"join|{name}|drs", sr.scale.grad.numpy())
    np.savez_compressed(AC.F24, **OUT)
    with open(AC.F24_MANIFEST, "w") as f:
        json.dump({"fixture": "f24_attention.npz", "sample_above": AC.SAMPLE_ABOVE, "sizes": SIZES, "zero_in_the_reference": ZERO, "state_dict_keys": keylists}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", AC.F24, os.path.getsize(AC.F24), "bytes;", len(OUT), "arrays")


if __name__ == "__main__":
    main()
