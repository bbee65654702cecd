"""Cases of golden F25 (tests/golden/make_golden_myfusion.py -> f25_myfusion.npz + f25_manifest.json): the reference's MixConvBlock,
MixFormerBlock, DCBlock, Decoder, LSDecoder and MyFusion in float64.  Inputs and parameters are rebuilt from closed forms
(oracle.fusion_oracle), so the fixture holds results only.  The builders take the module namespaces (the port's core.block / core.model, or
the reference's) so that the generator, the CPU layout test and the GPU test construct the same things.

Block cases: 2 x C x 10 x 12 signed inputs; the two decoders read a four-level pyramid of 16 / 32 / 64 / 128 channels at 16 x 20, 8 x 10,
4 x 5 and 2 x 2 (what stride-2 kernel-2 convs make of 16 x 20).  Model cases: the four (configuration, seed) pairs below at 1 x 1 x 32 x 32
and 2 x 1 x 32 x 40 -- MyFusion ends in a ReLU6 and many parameter seeds give a fused image that is zero everywhere; these are alive: the
fraction of positive pixels lies in [0.1, 0.95] (the generator and the GPU test both assert it) and every stored gradient is non-zero."""
import inspect
import os

from oracle import fusion_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F25, F25_MANIFEST = os.path.join(G, "f25_myfusion.npz"), os.path.join(G, "f25_manifest.json")
ALIVE = (0.1, 0.95)

# name -> (class, args, kwargs, train mode, input channels, parameter seed, BatchNorm inside)
BLOCK_CASES = {
    "mix_16_16": ("MixConvBlock", (16, 16), {}, False, 16, 25, False),
    "mix_16_32_attn": ("MixConvBlock", (16, 32), {"attention": True}, False, 16, 26, False),
    "mix_8_8_s2": ("MixConvBlock", (8, 8), {"scale": 2}, False, 8, 27, False),
    "mixformer_16_16": ("MixFormerBlock", (16, 16), {}, True, 16, 28, True),
    "dc_32_16": ("DCBlock", (32, 16), {}, False, 32, 29, False),
    "dc_16_16_res": ("DCBlock", (16, 16), {"residual": True}, False, 16, 30, False),
}
BLOCK_HW = (10, 12)
DECODER_CASES = {"decoder": ("Decoder", 31), "lsdecoder": ("LSDecoder", 32)}
PYRAMID = ((16, 16, 20), (32, 8, 10), (64, 4, 5), (128, 2, 2))
NUM_CH = [16, 32, 64, 128]

# configuration -> (MyFusion arguments with class NAMES, seed, train mode)
CONFIGS = {
    "A": ({}, 7, False),
    "B": (dict(encoder="MixConvBlock", decoder="LSDecoder", fusion_method="elem", fusion_mode="max", down_mode="maxpool", up_mode="nearest",
               share_weight_levels=2), 2, False),
    "C": (dict(encoder=["SepConvBlock", "MixConvBlock", "Res2ConvBlock", "MixFormerBlock"], decoder="Decoder", fusion_method="concat",
               share_weight_levels=0), 3, True),
    "D": (dict(encoder="MixConvBlock", decoder="FSDecoder", fusion_method="rfn", share_weight_levels=3), 3, False),
}
SHAPES = ((1, 1, 32, 32), (2, 1, 32, 40))


def tag(cfg, shape):
    return f"MyFusion_{cfg}_{shape[0]}x{shape[2]}x{shape[3]}"


def build_block(B, name):
    cls, args, kw, train, _, _, _ = BLOCK_CASES[name]
    m = getattr(B, cls)(*args, **kw)
    return m.train() if train else m.eval()


def build_decoder(B, name):
    return getattr(B, DECODER_CASES[name][0])(B.DCBlock, NUM_CH).eval()


def build_model(M, B, cfg):
    kw, _, train = CONFIGS[cfg]
    kw = dict(kw)
    for k in ("encoder", "decoder"):
        if k in kw:
            kw[k] = [getattr(B, n) for n in kw[k]] if isinstance(kw[k], list) else getattr(B, kw[k])
    m = M.MyFusion(**kw)
    return m.train() if train else m.eval()


def closed_form_state(module, seed):
    """what gpu_util.load_closed_form loads: closed_form_param(i, key, shape, seed) for the i-th state_dict entry"""
    return {k: O.closed_form_param(i, k, tuple(v.shape), seed) for i, (k, v) in enumerate(module.state_dict().items())}


def block_input(name):
    c = BLOCK_CASES[name][4]
    return O.closed_form_signed((2, c) + BLOCK_HW, 0.5, 1.0)


def pyramid_inputs():
    return [O.closed_form_signed((2, c, h, w), 0.5 + 0.1 * i, 1.0) for i, (c, h, w) in enumerate(PYRAMID)]


def upstream(shape):
    return O.closed_form_signed(tuple(shape), 1.5, 1.0)


def model_inputs(shape):
    return O.closed_form_image(shape, 0.3), O.closed_form_image(shape, 1.7)


def model_upstream(shape):
    return O.closed_form_signed(tuple(shape), 0.9, 1.0)


def ctor_defaults(cls):
    """constructor signature as JSON: name -> default (classes by name, '<required>' where there is none)"""
    out = {}
    for k, p in inspect.signature(cls.__init__).parameters.items():
        if k == "self":
            continue
        d = p.default
        out[k] = "<required>" if d is inspect.Parameter.empty else (d.__name__ if inspect.isclass(d) else d)
    return out


def key_shapes(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]
