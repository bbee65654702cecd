"""No GPU: the fp64 definitions of tests/mixdw_cases.py equal torch's float64 autograd of the composition the kernels replace (chunk -> F.pad
-> F.conv2d(groups) -> cat); the case table covers what it claims; every planted wrong definition exceeds the bound on some case; the library
exports the entry points and refuses every illegal argument combination before any launch; ConvLayer routes depth-wise 5 x 5 / 7 x 7 layers;
the constructor defaults, __all__ and state_dict keys of the new blocks and of MyFusion equal the lists recorded from the reference (F25
manifest); the training / test scripts accept --model MyFusion with its flags."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mixdw_cases as MC
from mixdw_cases import CASES, LEGAL, TH, TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SMALL = [c for c in CASES if c.n * c.c * c.nseg * c.h * c.w <= 400000]


def _torch_composition(c, o):
    x = torch.from_numpy(o["x"]).double().requires_grad_()
    ws = [torch.from_numpy(np.ascontiguousarray(w)).double().reshape(c.c, 1, k, k).requires_grad_() for w, k in zip(MC.unpack(c, o["w"]), c.ks)]
    b = torch.from_numpy(o["bias"]).double().requires_grad_() if c.bias else None
    ys = []
    for i, (xs, w, k) in enumerate(zip(torch.chunk(x, c.nseg, dim=1), ws, c.ks)):
        p = k // 2
        xp = F.pad(xs, (p, p, p, p), mode="reflect" if c.reflect else "constant") if p else xs
        ys.append(F.conv2d(xp, w, b[i * c.c:(i + 1) * c.c] if c.bias else None, groups=c.c))
    y = torch.cat(ys, dim=1)
    y.backward(torch.from_numpy(o["gy"]).double())
    return dict(y=y.detach().numpy(), dx=x.grad.numpy(), dw=torch.cat([w.grad.reshape(-1) for w in ws]).numpy(), db=b.grad.numpy() if c.bias else None)


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_definitions_equal_torch_float64_autograd(c):
    o = MC.operands(c)
    want, got = _torch_composition(c, o), MC.define(c, o)
    for name in ("y", "dx", "dw", "db"):
        if want[name] is None:
            continue
        g, w = np.asarray(got[name]).reshape(-1), want[name].reshape(-1)
        scale = max(np.abs(w).max(), 1e-30)
        assert np.abs(g - w).max() <= 1e-12 * scale * max(1, c.n * c.h * c.w) ** 0.5, name


def test_bounds_are_small_against_the_outputs():
    """no bound exceeds 1e-3 of its output's scale, and none is zero where the output is not"""
    for c in SMALL:
        o = MC.operands(c)
        want, bound = MC.define(c, o), MC.bounds(c, o)
        for name in ("y", "dx", "dw", "db"):
            w, b = np.asarray(want[name]), np.asarray(bound[name])
            assert b.shape == w.shape
            assert b.max() <= 1e-3 * np.abs(w).max(), (c.id, name, b.max(), np.abs(w).max())
            assert (b[w != 0] > 0).all(), (c.id, name)


def test_the_table_covers_what_it_claims():
    assert {(c.k0, c.nseg) for c in CASES} == set(LEGAL) and len(LEGAL) == 10
    assert {c.c for c in CASES} >= {1, 3, 8} and {c.n for c in CASES} >= {1, 3}
    for k0, nseg in LEGAL:
        mine = [c for c in CASES if (c.k0, c.nseg) == (k0, nseg)]
        assert {c.reflect for c in mine} == {True, False} and {c.bias for c in mine} == {True, False}, (k0, nseg)
        assert {c.h for c in mine} >= {TH - 1, TH, TH + 1, 2 * TH + 1} and {c.w for c in mine} >= {TW - 1, TW, TW + 1, 2 * TW + 1}, (k0, nseg)
        assert all(c.h != c.w for c in mine if c.h >= TH - 1)
        assert {c.guard for c in mine} == {3, 4}
    for k in (1, 3, 5, 7):      # the smallest reflect plane of each kernel size, as a lone kernel and as the largest of a mix
        p = k // 2
        assert any(c.reflect and c.nseg == 1 and c.k0 == k and (c.h, c.w) == (p + 1, p + 1) for c in CASES)
        assert any(c.reflect and c.k0 == 1 and c.ks[-1] == k and (c.h, c.w) == (p + 1, p + 1) for c in CASES)
    assert any(c.n * c.c * c.nseg * c.tiles > MC.MAX_BLOCKS for c in CASES)
    assert all(c.guard > 0 and MC.SENT != 0.0 for c in CASES)
    for c in CASES:
        assert c.workspace_bytes == c.n * c.c * c.nseg * c.tiles * MC.SLOTS * 4
        assert not c.reflect or min(c.h, c.w) >= c.ks[-1] // 2 + 1


def test_the_kernel_constants_are_the_tables():
    src = open(os.path.join(ROOT, "multi-modal-image-fusion_amd", "csrc", "mixdw.hip")).read()
    assert f"MD_TH = {TH}, MD_TW = {TW}" in src and f"MD_MAX_BLOCKS = {MC.MAX_BLOCKS};" in src
    assert "MD_SLOTS = MD_KMAX * MD_KMAX + 1" in src and MC.SLOTS == 50
    assert "atomic" not in src.split("#include")[1] and "getenv" not in src


@pytest.mark.parametrize("mut", sorted(MC.MUTATIONS))
def test_every_planted_wrong_definition_exceeds_the_bound_somewhere(mut):
    hit = []
    for c in SMALL:
        o = MC.operands(c)
        true, bound = MC.define(c, o), MC.bounds(c, o)
        wrong = MC.define(c, o, mut)
        for name in MC.MUTATIONS[mut]:
            t, w = np.asarray(true[name]), np.asarray(wrong[name])
            if t.shape == w.shape and (np.abs(t - w) > np.asarray(bound[name])).any():
                hit.append((c.id, name))
    assert hit, mut
    assert {n for _, n in hit} == set(MC.MUTATIONS[mut]), (mut, hit[:4])


def test_library_exports_the_entry_points_and_validates_without_gpu():
    from mmif._lib import SIGNATURES, lib
    for name in ("mmif_mixdw_fwd", "mmif_mixdw_dgrad", "mmif_mixdw_wgrad_workspace", "mmif_mixdw_wgrad"):
        assert hasattr(lib, name) and name in SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mmif.h")).read()
    assert all(f"{n}(" in hdr for n in ("mmif_mixdw_fwd", "mmif_mixdw_dgrad", "mmif_mixdw_wgrad_workspace", "mmif_mixdw_wgrad"))
    f = (ctypes.c_float * 64)()
    big = (ctypes.c_char * (1 << 16))()
    ws, nws = ctypes.addressof(big), 1 << 16

    def calls(n, c, nseg, k0, h, wd, reflect):
        a = (n, c, nseg, k0, h, wd)
        return ((lambda: lib.mmif_mixdw_fwd(f, f, None, f, *a, reflect, None), b"mixdw_fwd"),
                (lambda: lib.mmif_mixdw_dgrad(f, f, f, *a, reflect, None), b"mixdw_dgrad"),
                (lambda: lib.mmif_mixdw_wgrad(f, f, f, None, *a, reflect, ws, nws, None), b"mixdw_wgrad"))

    bad = [((1, 1, 1, 2, 8, 8, 0), b"k0 must be odd"), ((1, 1, 1, 0, 8, 8, 0), b"k0 must be odd"), ((1, 1, 1, -1, 8, 8, 0), b"k0 must be odd"),
           ((1, 1, 0, 1, 8, 8, 0), b"nseg must be 1..4"), ((1, 1, 5, 1, 8, 8, 0), b"nseg must be 1..4"),
           ((1, 1, 2, 7, 8, 8, 0), b"must be <= 7"), ((1, 1, 4, 3, 8, 8, 0), b"must be <= 7"), ((1, 1, 1, 9, 8, 8, 0), b"must be <= 7"),
           ((1, 1, 1, 7, 3, 8, 1), b"reflect padding needs h,w >= 4"), ((1, 1, 4, 1, 8, 3, 1), b"reflect padding needs h,w >= 4"),
           ((1, 1, 1, 3, 1, 1, 1), b"reflect padding needs h,w >= 2"), ((1, 1, 2, 3, 2, 2, 1), b"reflect padding needs h,w >= 3"),
           ((0, 1, 1, 1, 8, 8, 0), b"bad arguments"), ((1, 0, 1, 1, 8, 8, 0), b"bad arguments"), ((1, 1, 1, 1, 0, 8, 0), b"bad arguments"),
           ((1, 1, 1, 1, 8, 0, 0), b"bad arguments")]
    for args, msg in bad:
        for call, who in calls(*args):
            assert call() == -1, (args, who)
            err = lib.mmif_last_error()
            assert who + b":" in err and msg in err, (args, err)
        assert args[6] or lib.mmif_mixdw_wgrad_workspace(*args[:6]) == 0      # (the query has no padding mode)
    # null pointers and a short workspace (legal geometry)
    a = (1, 1, 2, 1, 4, 4)
    assert lib.mmif_mixdw_fwd(None, f, None, f, *a, 1, None) == -1 and b"mixdw_fwd: null pointer" in lib.mmif_last_error()
    assert lib.mmif_mixdw_dgrad(f, None, f, *a, 1, None) == -1 and b"mixdw_dgrad: null pointer" in lib.mmif_last_error()
    assert lib.mmif_mixdw_wgrad(f, f, None, None, *a, 1, ws, nws, None) == -1 and b"mixdw_wgrad: null pointer" in lib.mmif_last_error()
    need = lib.mmif_mixdw_wgrad_workspace(*a)
    assert need == 1 * 2 * 1 * MC.SLOTS * 4
    assert lib.mmif_mixdw_wgrad(f, f, f, None, *a, 1, ws, need - 4, None) == -3 and b"mixdw_wgrad: workspace" in lib.mmif_last_error()
    # the k = 1, 3 entry points keep their own contract
    assert lib.mmif_dwconv_dgrad(f, f, f, 1, 1, 4, 4, 5, 1, None) == -1 and b"dwconv_dgrad: ksize must be 1 or 3" in lib.mmif_last_error()


def test_convlayer_routes_wide_depthwise_layers():
    import core.block as B
    for k in (5, 7):
        l = B.ConvLayer(16, 16, ksize=k, groups=16)
        assert l._depthwise and l._dw_wide and l._epilogue
        assert B.ConvLayer(16, 16, ksize=k, groups=16, bias=False, act=None, padding_mode='zeros')._dw_wide
        assert not B.ConvLayer(16, 16, ksize=k, groups=16, padding=1)._depthwise and not B.ConvLayer(16, 16, ksize=k, groups=16, stride=2)._depthwise
        assert not B.ConvLayer(16, 16, ksize=k, groups=4)._depthwise
    assert not B.ConvLayer(16, 16, ksize=9, groups=16)._depthwise
    for k in (1, 3):
        l = B.ConvLayer(16, 16, ksize=k, groups=16)
        assert l._depthwise and not l._dw_wide
    # a wide depth-wise layer has no CPU path, like every other kernel-backed layer
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        B.ConvLayer(4, 4, ksize=5, groups=4)(torch.zeros(1, 4, 8, 8))
    blk = B.MixConvBlock(8, 8)
    assert blk._fused and [d.layers[0].kernel_size for d in blk.dwconvs] == [(1, 1), (3, 3), (5, 5), (7, 7)]
    assert not B.MixConvBlock(8, 8, norm=nn.BatchNorm2d)._fused and not B.MixConvBlock(4, 4, scale=5)._fused


def _manifest():
    return json.load(open(os.path.join(G, "f25_manifest.json")))


def test_new_blocks_and_myfusion_mirror_the_reference_layout():
    import core.block as B
    import core.model as M
    import myfusion_cases as FC
    man, _defaults = _manifest(), FC.ctor_defaults
    for name in ("MixConvBlock", "MixFormerBlock", "DCBlock", "Decoder", "LSDecoder"):
        assert name in B.__all__
        assert _defaults(getattr(B, name)) == man["defaults"][name], name
    assert "MyFusion" in M.__all__ and _defaults(M.MyFusion) == man["defaults"]["MyFusion"]
    assert [n for n in man["block_all"] if n in ("MixConvBlock", "MixFormerBlock", "DCBlock", "Decoder", "LSDecoder")] == \
        [n for n in B.__all__ if n in ("MixConvBlock", "MixFormerBlock", "DCBlock", "Decoder", "LSDecoder")]
    for case in FC.BLOCK_CASES:
        assert FC.key_shapes(FC.build_block(B, case)) == man["state_dict"][case], case
    for case in FC.DECODER_CASES:
        assert FC.key_shapes(FC.build_decoder(B, case)) == man["state_dict"][case], case
    for cfg in FC.CONFIGS:
        assert FC.key_shapes(FC.build_model(M, B, cfg)) == man["state_dict"]["MyFusion_" + cfg], cfg
    with pytest.raises(AssertionError):
        M.MyFusion(fusion_method='elem', fusion_mode='sca')
    with pytest.raises(AssertionError):
        M.MyFusion(fusion_method='attn', fusion_mode='sum')
    m = M.MyFusion(fusion_method='other')
    with pytest.raises(ValueError, match=r"only supported \['elem', 'attn', 'concat', 'rfn'\] method"):
        m.fusion((None, ) * 4, (None, ) * 4)
    sd = B.MixConvBlock(16, 16).state_dict()
    assert "dwconv.layers.0.weight" in sd and [k for k in sd if k.startswith("dwconvs.")] == [f"dwconvs.{i}.layers.0.weight" for i in range(4)]


def test_scripts_accept_myfusion_and_its_flags():
    import common
    import core.block as B
    flags = ["--encoder", "SepConvBlock,MixConvBlock,Res2ConvBlock,MixFormerBlock", "--decoder", "LSDecoder", "--fusion_method", "elem",
             "--fusion_mode", "max", "--down_mode", "maxpool", "--up_mode", "nearest", "--share_weight_levels", "2"]
    pkg = os.path.join(ROOT, "multi-modal-image-fusion_amd")
    for script, parse in (("train.py", common.get_train_args), ("test.py", common.get_test_args)):
        assert "build_model(args)" in open(os.path.join(pkg, script)).read()
        m = common.build_model(parse(["--model", "MyFusion"] + flags))
        assert type(m).__name__ == "MyFusion" and m.share_weight_levels == 2 and m.fusion_mode == "max"
        assert isinstance(m.EB2_2, B.MixConvBlock) and isinstance(m.EB4_1, B.MixFormerBlock) and not hasattr(m, 'EB3_2') and isinstance(m.decode, B.LSDecoder)
        d = common.build_model(parse(["--model", "MyFusion"]))
        assert isinstance(d.EB1_1, B.SepConvBlock) and isinstance(d.decode, B.NestDecoder) and d.share_weight_levels == 4
        assert d.fusion_method == "attn" and d.fusion_mode == "sca" and d.down_mode == "stride" and d.up_mode == "bilinear"
        one = common.build_model(parse(["--model", "MyFusion", "--encoder", "MixConvBlock"]))
        assert all(isinstance(getattr(one, f"EB{i}_1"), B.MixConvBlock) for i in (1, 2, 3, 4))
        with pytest.raises(ValueError, match="--encoder takes one name or four"):
            common.build_model(parse(["--model", "MyFusion", "--encoder", "SepConvBlock,MixConvBlock"]))
        assert type(common.build_model(parse(["--model", "DenseFuse"]))).__name__ == "DenseFuse"
        assert parse([]).model == "PFNetv1"
