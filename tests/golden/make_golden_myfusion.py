"""Golden F25: the reference's own MixConvBlock, MixFormerBlock, DCBlock, Decoder, LSDecoder (core/block.py) and MyFusion (core/model.py:630-842)
evaluated in float64 on the cases of tests/myfusion_cases.py -- outputs and the autograd gradients of sum(y * upstream) w.r.t. the inputs and
every parameter.  Needs a checkout of the reference, named by $MMIF_REFERENCE; never imported by a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_myfusion.py   ->   tests/golden/f25_myfusion.npz, f25_manifest.json

Keys: '<block case>|y', '|dx' (decoders: '|dx<level>'), '|dp_<parameter>' -- flat, at attention_cases.sample_index(size);
'MyFusion_<config>_<n>x<h>x<w>__y' (sampled the same way) and '__dp_<parameter>' (gpu_util.digest of the gradient).  The manifest lists every
key with its full size, the parameters and inputs that get no gradient (never stored: the inherited, never-called `dwconv` of the Mix / Res2
blocks; under decoder=Decoder, which reads the deepest level only, fuse1..3 and the first three pyramid inputs), the positive fraction of
every fused image, and the reference's constructor defaults, block.__all__ and state_dict key lists.

The generator refuses a model case whose fused image has less than 0.1 or more than 0.95 positive pixels, and any stored array that is
all-zero."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import attention_cases as AC  # noqa: E402
import myfusion_cases as FC  # noqa: E402
from gpu_util import digest  # noqa: E402
from oracle import fusion_oracle as O  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")
OUT, SIZES, NO_GRAD, POSITIVE = {}, {}, {}, {}


def load_ref():
    assert os.path.isfile(os.path.join(REF, "core", "model.py")), "set MMIF_REFERENCE to a checkout of the reference"
    sys.path.insert(0, os.path.join(REF, "core"))   # block.py / model.py fall back to `from block import *`, `from fusion import *`
    import block as RB
    import model as RM
    return RB, RM


def store(key, a, as_digest=False):
    a = np.asarray(a, np.float64)
    assert np.isfinite(a).all(), key
    O.assert_alive(a, key)                       # an all-zero array pins nothing: refused
    SIZES[key] = int(a.size)
    OUT[key] = digest(a) if as_digest else a.reshape(-1)[AC.sample_index(a.size)]


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def load(mod, seed):
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in FC.closed_form_state(mod, seed).items()})
    return mod.double()


def param_grads(name, mod, sep, as_digest, allowed):
    missing = []
    for k, p in mod.named_parameters():
        if p.grad is None:
            assert allowed(k), (name, k)
            missing.append(k)
            continue
        store(f"{name}{sep}dp_{k}", p.grad.numpy(), as_digest)
    return missing


def main():
    RB, RM = load_ref()
    torch.set_num_threads(8)
    state = {}
    for name, (_, _, _, _, _, seed, _) in FC.BLOCK_CASES.items():
        mod = FC.build_block(RB, name)
        state[name] = FC.key_shapes(mod)
        mod = load(mod, seed)
        x = t64(FC.block_input(name), True)
        y = mod(x)
        (y * t64(FC.upstream(y.shape))).sum().backward()
        O.assert_alive(y.detach().numpy(), name, lo=0.05, hi=0.95)       # every block ends in a ReLU6
        store(f"{name}|y", y.detach().numpy())
        store(f"{name}|dx", x.grad.numpy())
        NO_GRAD[name] = param_grads(name, mod, "|", False, lambda k: k.endswith("dwconv.layers.0.weight") and "Mix" in FC.BLOCK_CASES[name][0])
    for name, (_, seed) in FC.DECODER_CASES.items():
        mod = FC.build_decoder(RB, name)
        state[name] = FC.key_shapes(mod)
        mod = load(mod, seed)
        feats = [t64(f, True) for f in FC.pyramid_inputs()]
        y = mod(feats)
        (y * t64(FC.upstream(y.shape))).sum().backward()
        O.assert_alive(y.detach().numpy(), name, lo=0.05, hi=0.95)
        store(f"{name}|y", y.detach().numpy())
        NO_GRAD[name] = []
        for i, f in enumerate(feats):
            if f.grad is None:
                assert name == "decoder" and i < 3
                NO_GRAD[name].append(f"x{i}")
            else:
                store(f"{name}|dx{i}", f.grad.numpy())
        NO_GRAD[name] += param_grads(name, mod, "|", False, lambda k: False)
    for cfg, (_, seed, _) in FC.CONFIGS.items():
        state["MyFusion_" + cfg] = FC.key_shapes(FC.build_model(RM, RB, cfg))
        for shape in FC.SHAPES:
            tag = FC.tag(cfg, shape)
            mod = load(FC.build_model(RM, RB, cfg), seed)
            i1, i2 = (t64(a) for a in FC.model_inputs(shape))
            y = mod(i1, i2)
            (y * t64(FC.model_upstream(y.shape))).sum().backward()
            yn = y.detach().numpy()
            O.assert_alive(yn, tag, lo=FC.ALIVE[0], hi=FC.ALIVE[1])
            POSITIVE[tag] = round(float((yn > 0).mean()), 4)
            store(tag + "__y", yn)
            NO_GRAD[tag] = param_grads(tag, mod, "__", True,
                                       lambda k: k.endswith("dwconv.layers.0.weight") or (cfg == "C" and k.startswith(("fuse1.", "fuse2.", "fuse3."))))
            print(tag, "positive", POSITIVE[tag], "params without gradient", len(NO_GRAD[tag]))
    names = ("MixConvBlock", "MixFormerBlock", "DCBlock", "Decoder", "LSDecoder")
    defaults = {n: FC.ctor_defaults(getattr(RB, n)) for n in names}
    defaults["MyFusion"] = FC.ctor_defaults(RM.MyFusion)
    np.savez_compressed(FC.F25, **OUT)
    with open(FC.F25_MANIFEST, "w") as f:
        json.dump({"fixture": "f25_myfusion.npz", "sample_above": AC.SAMPLE_ABOVE, "sizes": SIZES, "no_gradient": NO_GRAD, "positive_fraction": POSITIVE,
                   "defaults": defaults, "block_all": list(RB.__all__), "model_all": list(RM.__all__), "state_dict": state}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FC.F25, os.path.getsize(FC.F25), "bytes;", len(OUT), "arrays")


if __name__ == "__main__":
    main()
