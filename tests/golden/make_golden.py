#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by IMPORTING THE REFERENCE.

Run once in the build container (where /root/reference exists):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

The reference (chenzpstar/Multi-Modal-Image-Fusion, torch-CPU, fp32) is executed on
closed-form inputs / parameters (oracle.fusion_oracle.closed_form_*), so the committed
fixtures hold only the reference's OUTPUTS; tests rebuild the inputs from the same
formulas.  Nothing here is imported at test time and the reference never travels to the
GPU box.  Fixture map:

  f1_loss_known_answer.json  core/loss.py:388-423 recipe (seed 0, rand(2,1,256,256) x3)
  f2_loss_grads.npz          loss values + d/dimgf on closed-form images (incl. clamp / tie cases)
  f3_conv.npz, f3_conv_2.npz ConvLayer fwd + (dx, dW, db) per (Cin, Cout, k) (the cases split in two halves)
  f4_blocks.npz              DenseBlock / ConvBlock / RFN / NestDecoder / fusion fns fwd + bwd
  f5_models.npz              PFNetv1, PFNetv2, DenseFuse, NestFuse, RFNNest forward + grad digests
  f5_manifest.json           state_dict key/shape manifests
  f6_traj.npz                3-step train trajectories (train.py:61-75 semantics)
  f8_feed.npz                data/transform.py norm (3 modes) + transform (8 modes) on an integer-valued 6x6 / 5x5 patch
  f9_ssim_modes.npz          SSIMLoss 'w-ssim' | 'ms-ssim' | 'msw-ssim' (core/loss.py:259-277) and TVLoss (:347-358): value + d/dimgf
  f10_vifnet.npz / f10_manifest.json   VIFNet (core/model.py:189-206) forward + gradient digests + state_dict manifest
  f11_general_conv.npz       ConvLayer with k = 5/7, stride 2, zero padding, ConvTranspose2d (core/block.py:56-76): fwd + (dx, dW, db)
  f12_n4_models.npz / f12_manifest.json   bilinear Upsample (core/block.py:965-991) fwd + dx; DeepFuse, DBNet forward + gradient digests
  f13_n4_norm.npz / f13_manifest.json   ConvLayer with BatchNorm2d / GroupNorm + ReLU / LeakyReLU / Tanh (core/block.py:78-92): y, dx, parameter
                             gradients, running buffers; SEDRFuse, IFCNN, DIFNet, PMGI forward + gradient / buffer digests
  f14_n4_nested.npz / f14_manifest.json   UNFusion, MAFusion forward + gradient digests
  f15_n4_res2.npz / f15_manifest.json   depth-wise ConvLayer, ReLU6, Res2ConvBlock (core/block.py:286-350), Res2Fusion
  f7_metric_ssim.json        core/metric.py:316-364 calc_ssim (the SSIM that test.py:49-52 reports) on closed-form images
  f16_stock_fallbacks.npz    the argument combinations that run as stock torch ops (core/_stock.py): SSIMLoss(use_padding=True) in its four
                             modes, SSIM(size_average=False) / other windows, metric calc_ssim(win 7, padding, full), channel_pooling('nuclear')
  f17_reference_init.json    PFNetv1's state_dict after torch.manual_seed(0): key, shape, dtype, sha256 of the bytes
  f18_sample_folders.json    data/samples layout: relative path, width, height, PIL mode, format of every image
"""
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MMIF_REFERENCE", "/root/reference")
sys.path.insert(0, REF)       # reference's `core` package
sys.path.insert(1, ROOT)      # oracle.* (closed-form helpers only)

import numpy as np
import torch
import torch.nn as nn

import core.block as rblock      # noqa: E402  (reference)
import core.fusion as rfusion    # noqa: E402
import core.loss as rloss        # noqa: E402
import core.model as rmodel      # noqa: E402
from oracle.fusion_oracle import assert_alive, closed_form_image, closed_form_param, closed_form_signed, live_param  # noqa: E402

assert os.path.realpath(rblock.__file__).startswith(os.path.realpath(REF)), rblock.__file__
torch.set_num_threads(8)
T = torch.from_numpy


def load_closed_form(module, seed=0):
    sd = module.state_dict()
    new = {}
    for i, (k, v) in enumerate(sd.items()):
        new[k] = T(closed_form_param(i, k, tuple(v.shape), seed))
    module.load_state_dict(new)
    return module


def load_live(module, name):
    """the live closed-form set of NestFuse / RFN-Nest (oracle.LIVE_PARAMS): the final ReLU passes 30-60 % of the pixels"""
    sd = module.state_dict()
    module.load_state_dict({k: T(live_param(name, i, k, tuple(v.shape))) for i, (k, v) in enumerate(sd.items())})
    return module


# tensors that are zero BY DEFINITION of the case they pin (everything else must be alive, see save())
ZERO_BY_DESIGN = {"attn_zero__y", "attn_zero__da",            # all-zero features: the clamp(min=1e-7) branch, core/fusion.py:33
                  "c_g_grad",                                 # constant fused image: the Sobel gradient of a constant is 0
                  "bn_eval_buf_layers.1.num_batches_tracked", # eval mode / a BatchNorm PMGI never calls: the counter stays 0
                  "PMGI_2x32x32__buf_transfer1.1.layers.1.num_batches_tracked", "PMGI_1x19x26__buf_transfer1.1.layers.1.num_batches_tracked"}


def save(fname, out):
    """np.savez_compressed with a liveness gate: a fixture that is all-zero pins nothing (the round-3 NestFuse / RFN-Nest F5 cases
    compared 0 with 0 for three rounds), so the generator refuses to write one unless the case is zero by design."""
    for k, v in out.items():
        if k not in ZERO_BY_DESIGN:
            assert_alive(v, f"{fname}:{k}")
    np.savez_compressed(os.path.join(HERE, fname), **out)


def digest(a):
    """Compact pin of a tensor: sum, abs-sum, first 16 and 16 strided samples."""
    f = np.asarray(a, dtype=np.float32).reshape(-1)
    n = f.size
    idx = (np.arange(16) * max(1, n // 16)) % n
    return np.concatenate(([f.astype(np.float64).sum(), np.abs(f.astype(np.float64)).sum()],
                           f[:16] if n >= 16 else np.pad(f, (0, 16 - n)), f[idx])).astype(np.float64)


# ---------------------------------------------------------------- F1
def make_f1():
    torch.manual_seed(0)
    x1 = torch.rand(2, 1, 256, 256)
    x2 = torch.rand(2, 1, 256, 256)
    y = torch.rand(2, 1, 256, 256)
    out = {}
    out["ssim"] = rloss.SSIMLoss("ssim", weight=1.0)(x1, x2, y).item()
    out["pixel_avg"] = rloss.PixelLoss("l1", weight=0.01)(x1, x2, y).item()
    out["grad_avg"] = rloss.GradLoss("l1", weight=0.1)(x1, x2, y).item()
    out["tv"] = rloss.TVLoss("l1", weight=1.0)(y - x1).item()
    out["pixel_max"] = rloss.PixelLoss("l1", weight=0.01)(x1, x2, y, mode="max").item()
    out["grad_max"] = rloss.GradLoss("l1", weight=0.1)(x1, x2, y, mode="max").item()
    out["total_max"] = out["ssim"] + out["pixel_max"] + out["grad_max"]
    out["ssim_per_sample_x1_y"] = rloss.SSIM(11, 1.0, False)(x1, y)["ssim"].tolist()
    out["window_1d"] = rloss._gaussian_kernel(11, 1.5).tolist()
    out["window_2d_sum"] = float(rloss.create_window(11).double().sum())
    # first 8 values of each random image so the test can confirm it regenerated the same inputs
    out["x1_head"] = x1.reshape(-1)[:8].tolist()
    out["y_head"] = y.reshape(-1)[:8].tolist()
    json.dump(out, open(os.path.join(HERE, "f1_loss_known_answer.json"), "w"), indent=1)


# ---------------------------------------------------------------- F2
def loss_case(img1, img2, imgf):
    res = {}
    i1, i2 = T(img1), T(img2)
    f = T(imgf).clone().requires_grad_(True)
    l1 = rloss.SSIMLoss("ssim", weight=1.0)(i1, i2, f)
    l2 = rloss.PixelLoss("l1", weight=0.01)(i1, i2, f, mode="max")
    l3 = rloss.GradLoss("l1", weight=0.1)(i1, i2, f, mode="max")
    for name, l in (("ssim", l1), ("pixel", l2), ("grad", l3)):
        g, = torch.autograd.grad(l, f, retain_graph=True)
        res["l_" + name] = np.float64(l.item())
        res["g_" + name] = g.numpy()
    g, = torch.autograd.grad(l1 + l2 + l3, f)
    res["g_total"] = g.numpy()
    res["l_pixel_avg"] = np.float64(rloss.PixelLoss("l1", weight=0.01)(i1, i2, f.detach(), mode="avg").item())
    res["l_grad_avg"] = np.float64(rloss.GradLoss("l1", weight=0.1)(i1, i2, f.detach(), mode="avg").item())
    return res


def f2_inputs(case):
    if case == "a":
        s = (2, 1, 32, 32)
        return closed_form_image(s, 0.1), closed_form_image(s, 1.3), closed_form_image(s, 2.2)
    if case == "b":
        s = (1, 1, 64, 48)
        return closed_form_image(s, 0.7), closed_form_image(s, 0.2), closed_form_image(s, 1.9)
    if case == "c":  # constant fused image: sigma_f^2 = 0 -> clamp branch of calc_ssim
        s = (1, 1, 24, 24)
        return closed_form_image(s, 0.4), closed_form_image(s, 1.1), np.full(s, 0.375, np.float32)
    if case == "d":  # img1 == img2: ties in torch.max
        s = (2, 1, 20, 28)
        a = closed_form_image(s, 0.9)
        return a, a.copy(), closed_form_image(s, 2.9)
    raise KeyError(case)


def make_f2():
    out = {}
    for case in "abcd":
        for k, v in loss_case(*f2_inputs(case)).items():
            out[f"{case}_{k}"] = v
    save("f2_loss_grads.npz", out)


# ---------------------------------------------------------------- F3
F3_CASES = [  # (name, Cin, Cout, k, relu, N, H, W)
    ("c1_16", 1, 16, 3, True, 2, 12, 20),
    ("c16_16", 16, 16, 3, True, 2, 12, 20),
    ("c48_16", 48, 16, 3, True, 2, 12, 20),
    ("c128_64", 128, 64, 3, True, 2, 12, 20),
    ("c16_1_lin", 16, 1, 3, False, 2, 12, 20),
    ("c8_64_k1", 8, 64, 1, True, 2, 12, 20),
    ("c88_64_k1", 88, 64, 1, True, 2, 12, 20),
    ("c16_16_thin_h", 16, 16, 3, True, 1, 2, 9),     # 2-row image: every row reflects
    ("c16_16_thin_w", 16, 16, 3, True, 1, 9, 2),
    ("c32_16_odd", 32, 16, 3, True, 1, 37, 53),      # ragged vs. any power-of-two tile
]


def make_f3():
    out = {}
    for name, cin, cout, k, relu, N, H, W in F3_CASES:
        layer = rblock.ConvLayer(cin, cout, ksize=k, act=nn.ReLU if relu else None)
        load_closed_form(layer, seed=3)
        x = T(closed_form_signed((N, cin, H, W), 0.5, 1.0)).requires_grad_(True)
        gy = T(closed_form_signed((N, cout, H, W), 1.5, 1.0))
        y = layer(x)
        y.backward(gy)
        out[name + "_y"] = y.detach().numpy()
        out[name + "_dx"] = x.grad.numpy()
        out[name + "_dw"] = layer.layers[0].weight.grad.numpy()
        out[name + "_db"] = layer.layers[0].bias.grad.numpy()
    # two files, the first half of the cases and the rest, to keep each fixture under 1 MiB
    first = {c[0] for c in F3_CASES[:(len(F3_CASES) + 1) // 2]}
    save("f3_conv.npz", {k: v for k, v in out.items() if k.rsplit("_", 1)[0] in first})
    save("f3_conv_2.npz", {k: v for k, v in out.items() if k.rsplit("_", 1)[0] not in first})


# ---------------------------------------------------------------- F11 (row n4: the general ConvLayer forms)
#            name            cin cout k  stride transposed padding_mode relu  N  H   W
F11_CASES = [("k5_1_16",       1, 16, 5, 1, False, "reflect", True, 2, 13, 17),
             ("k7_16_32",     16, 32, 7, 1, False, "reflect", True, 1, 12, 20),
             ("k7_tiny",       8,  8, 7, 1, False, "reflect", True, 1, 4, 5),
             ("k5_16_1_lin",  16,  1, 5, 1, False, "reflect", False, 2, 9, 11),
             ("s2_32_64",     32, 64, 3, 2, False, "reflect", True, 2, 13, 18),
             ("s2_even",      24, 16, 3, 2, False, "reflect", True, 1, 16, 32),
             ("zeros_k3",     16, 24, 3, 1, False, "zeros", True, 1, 10, 9),
             ("convT_24_16",  24, 16, 3, 2, True, "zeros", True, 2, 7, 9),
             ("convT_lin",     8, 12, 3, 2, True, "zeros", False, 1, 5, 4)]


def make_f11():
    out = {}
    for name, cin, cout, k, stride, transposed, pmode, relu, N, H, W in F11_CASES:
        layer = rblock.ConvLayer(cin, cout, ksize=k, stride=stride, act=nn.ReLU if relu else None,
                                 layer=nn.ConvTranspose2d if transposed else nn.Conv2d, padding_mode=pmode)
        load_closed_form(layer, seed=11)
        x = T(closed_form_signed((N, cin, H, W), 0.5, 1.0)).requires_grad_(True)
        y = layer(x)
        gy = T(closed_form_signed(tuple(y.shape), 1.5, 1.0))
        y.backward(gy)
        out[name + "_y"] = y.detach().numpy()
        out[name + "_dx"] = x.grad.numpy()
        out[name + "_dw"] = layer.layers[0].weight.grad.numpy()
        out[name + "_db"] = layer.layers[0].bias.grad.numpy()
    save("f11_general_conv.npz", out)


# ---------------------------------------------------------------- F12 (row n4: bilinear up-sampling, DeepFuse, DBNet)
def make_f12():
    out, manifest = {}, {}
    for tag, scale, shape in (("bl_x2", 2, (2, 3, 5, 7)), ("bl_x8", 8, (1, 4, 4, 3)), ("bl_x2_row", 2, (1, 2, 1, 6))):
        up = rblock.Upsample('bilinear', scale)
        x = T(closed_form_signed(shape, 0.4, 1.0)).requires_grad_(True)
        tgt = (shape[0], shape[1], shape[2] * scale, shape[3] * scale)
        y = up(x, torch.Size(tgt))
        y.backward(T(closed_form_signed(tgt, 1.3, 1.0)))
        out[tag + "_y"], out[tag + "_dx"] = y.detach().numpy(), x.grad.numpy()
    for name, shapes in (("DeepFuse", ((2, 1, 32, 32), (1, 1, 21, 30))), ("DBNet", ((2, 1, 32, 32), (1, 1, 40, 24), (1, 1, 37, 53)))):
        for shape in shapes:
            tag = f"{name}_{shape[0]}x{shape[2]}x{shape[3]}"
            model = load_closed_form(getattr(rmodel, name)(), seed=2)
            manifest[name] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
            i1, i2 = T(closed_form_image(shape, 0.3)), T(closed_form_image(shape, 1.7))
            y = model(i1, i2)
            y.backward(T(closed_form_signed(shape, 0.9, 1.0)))
            out[tag + "__y"] = y.detach().numpy()
            for k, p in model.named_parameters():
                out[f"{tag}__dp_{k}"] = digest(p.grad.numpy())
    # (seed 2: with seed 1 one pre-activation of DBNet's decode.1 at 2x32x32 lies within fp32 rounding of zero, so its ReLU mask --
    # and 1 % of the gradients behind it -- depends on the summation order of the conv that produced it)
    save("f12_n4_models.npz", out)
    json.dump(manifest, open(os.path.join(HERE, "f12_manifest.json"), "w"), indent=0)


# ---------------------------------------------------------------- F13 (row n4: norm / activation epilogues, SEDRFuse, IFCNN, DIFNet, PMGI)
#             name        cin cout k stride transposed norm act  train  N  H   W
F13_CASES = [("bn_relu",   16, 24, 3, 1, False, "bn", "relu", True, 3, 10, 12), ("bn_eval", 16, 24, 3, 1, False, "bn", "relu", False, 2, 9, 8),
             ("bn_lin",     8, 16, 3, 1, False, "bn", None, True, 2, 7, 9), ("bn_leaky_k5", 3, 16, 5, 1, False, "bn", "leaky", True, 2, 12, 11),
             ("bn_leaky_k1", 32, 16, 1, 1, False, "bn", "leaky", True, 2, 6, 7), ("gn_relu", 1, 64, 3, 1, False, "gn", "relu", True, 2, 10, 10),
             ("gn_s2",     24, 32, 3, 2, False, "gn", "relu", True, 2, 11, 14), ("gn_convT", 32, 16, 3, 2, True, "gn", "relu", True, 2, 5, 6),
             ("tanh_k1",   40, 1, 1, 1, False, None, "tanh", True, 2, 8, 9), ("leaky_k3", 16, 16, 3, 1, False, None, "leaky", True, 1, 9, 9)]
_NORMS = {"bn": nn.BatchNorm2d, "gn": nn.GroupNorm, None: None}
_ACTS = {"relu": nn.ReLU, "leaky": nn.LeakyReLU, "tanh": nn.Tanh, None: None}


def make_f13():
    out, manifest = {}, {}
    for name, cin, cout, k, stride, transposed, norm, act, train, N, H, W in F13_CASES:
        layer = rblock.ConvLayer(cin, cout, ksize=k, stride=stride, norm=_NORMS[norm], act=_ACTS[act],
                                 layer=nn.ConvTranspose2d if transposed else nn.Conv2d)
        load_closed_form(layer, seed=13)
        if norm == "bn":   # non-trivial running statistics (closed-form loading makes running_var signed: use its magnitude)
            layer.layers[1].running_var.abs_().add_(0.5)
            layer.layers[1].num_batches_tracked.zero_()
        layer.train(train)
        x = T(closed_form_signed((N, cin, H, W), 0.5, 1.0)).requires_grad_(True)
        y = layer(x)
        y.backward(T(closed_form_signed(tuple(y.shape), 1.5, 1.0)))
        out[name + "_y"], out[name + "_dx"] = y.detach().numpy(), x.grad.numpy()
        for kname, p in layer.named_parameters():
            out[f"{name}_dp_{kname}"] = p.grad.numpy()
        for kname, b in layer.named_buffers():
            out[f"{name}_buf_{kname}"] = b.detach().numpy().astype(np.float32)
    for name, shapes in (("SEDRFuse", ((2, 1, 32, 32),)), ("IFCNN", ((2, 1, 32, 32), (1, 1, 21, 30))), ("DIFNet", ((2, 1, 32, 32),)),
                         ("PMGI", ((2, 1, 32, 32), (1, 1, 19, 26)))):
        for shape in shapes:
            tag = f"{name}_{shape[0]}x{shape[2]}x{shape[3]}"
            model = load_closed_form(getattr(rmodel, name)(), seed=2)
            for mod in model.modules():
                if isinstance(mod, nn.BatchNorm2d):
                    mod.running_var.abs_().add_(0.5)
                    mod.num_batches_tracked.zero_()
            model.train()
            manifest[name] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
            i1, i2 = T(closed_form_image(shape, 0.3)), T(closed_form_image(shape, 1.7))
            y = model(i1, i2)
            y.backward(T(closed_form_signed(tuple(y.shape), 0.9, 1.0)))
            out[tag + "__y"] = y.detach().numpy()
            for k, p in model.named_parameters():
                if p.grad is not None:   # (PMGI never calls transfer1[1], core/model.py:589: no gradient)
                    out[f"{tag}__dp_{k}"] = digest(p.grad.numpy())
            for k, b in model.named_buffers():
                out[f"{tag}__buf_{k}"] = digest(b.detach().numpy().astype(np.float32))
    save("f13_n4_norm.npz", out)
    json.dump(manifest, open(os.path.join(HERE, "f13_manifest.json"), "w"), indent=0)


# ---------------------------------------------------------------- F14 (row n4: UNFusion, MAFusion -- compositions of the primitives above)
def make_f14():
    out, manifest = {}, {}
    for name, shapes in (("UNFusion", ((1, 1, 32, 32), (1, 1, 37, 53))), ("MAFusion", ((1, 1, 32, 32), (1, 1, 40, 24)))):
        for shape in shapes:
            tag = f"{name}_{shape[0]}x{shape[2]}x{shape[3]}"
            model = load_closed_form(getattr(rmodel, name)(), seed=2)
            manifest[name] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
            i1, i2 = T(closed_form_image(shape, 0.3)), T(closed_form_image(shape, 1.7))
            y = model(i1, i2)
            y.backward(T(closed_form_signed(tuple(y.shape), 0.9, 1.0)))
            out[tag + "__y"] = y.detach().numpy()
            for k, p in model.named_parameters():
                out[f"{tag}__dp_{k}"] = digest(p.grad.numpy())
    save("f14_n4_nested.npz", out)
    json.dump(manifest, open(os.path.join(HERE, "f14_manifest.json"), "w"), indent=0)


# ---------------------------------------------------------------- F15 (row n4: depth-wise ConvLayer, ReLU6, Res2ConvBlock, Res2Fusion)
def make_f15():
    out, manifest = {}, {}
    for name, kw, shape in (("dw_k3", dict(in_ch=16, out_ch=16, ksize=3, groups=16, bias=False, act=None), (2, 16, 9, 11)),
                            ("dw_k1", dict(in_ch=24, out_ch=24, ksize=1, groups=24, bias=False, act=None), (1, 24, 5, 6)),
                            ("dw_k3_bias", dict(in_ch=8, out_ch=8, ksize=3, groups=8, act=None), (2, 8, 2, 7)),
                            ("relu6_k1", dict(in_ch=16, out_ch=64, ksize=1, bias=False, act=nn.ReLU6), (2, 16, 6, 7))):
        layer = rblock.ConvLayer(**kw)
        load_closed_form(layer, seed=15)
        x = T(closed_form_signed(shape, 0.5, 8.0 if name == "relu6_k1" else 1.0)).requires_grad_(True)
        y = layer(x)
        y.backward(T(closed_form_signed(tuple(y.shape), 1.5, 1.0)))
        out[name + "_y"], out[name + "_dx"] = y.detach().numpy(), x.grad.numpy()
        for kname, p in layer.named_parameters():
            out[f"{name}_dp_{kname}"] = p.grad.numpy()
    blk = load_closed_form(rblock.Res2ConvBlock(16, 32, 4), seed=15)
    x = T(closed_form_signed((2, 16, 10, 12), 0.5, 1.0)).requires_grad_(True)
    y = blk(x)
    y.backward(T(closed_form_signed(tuple(y.shape), 1.5, 1.0)))
    out["res2block_y"], out["res2block_dx"] = y.detach().numpy(), x.grad.numpy()
    for kname, p in blk.named_parameters():
        if p.grad is not None:
            out[f"res2block_dp_{kname}"] = p.grad.numpy()
    for shape in ((1, 1, 32, 32), (2, 1, 24, 40)):
        tag = f"Res2Fusion_{shape[0]}x{shape[2]}x{shape[3]}"
        model = load_closed_form(rmodel.Res2Fusion(), seed=2)
        manifest["Res2Fusion"] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        i1, i2 = T(closed_form_image(shape, 0.3)), T(closed_form_image(shape, 1.7))
        y = model(i1, i2)
        y.backward(T(closed_form_signed(tuple(y.shape), 0.9, 1.0)))
        out[tag + "__y"] = y.detach().numpy()
        for k, p in model.named_parameters():
            if p.grad is not None:   # (Res2ConvBlock never calls the dwconv it inherits from SepConvBlock)
                out[f"{tag}__dp_{k}"] = digest(p.grad.numpy())
    save("f15_n4_res2.npz", out)
    json.dump(manifest, open(os.path.join(HERE, "f15_manifest.json"), "w"), indent=0)


# ---------------------------------------------------------------- F4
def run_module(mod, inputs, gout_phase):
    xs = [T(a).requires_grad_(True) for a in inputs]
    y = mod(*xs)
    gy = T(closed_form_signed(tuple(y.shape), gout_phase, 1.0))
    y.backward(gy)
    res = {"y": y.detach().numpy()}
    for i, x in enumerate(xs):
        res[f"dx{i}"] = x.grad.numpy()
    for k, p in mod.named_parameters():
        res["dp_" + k] = digest(p.grad.numpy())
    return res


def make_f4():
    out = {}

    def put(prefix, res):
        for k, v in res.items():
            out[f"{prefix}__{k}"] = v

    m = load_closed_form(rblock.DenseBlock(16, 16), 4)
    put("dense", run_module(m, [closed_form_signed((2, 16, 10, 14), 0.3)], 0.8))
    m = load_closed_form(rblock.ConvBlock(16, 64), 5)
    put("convblock", run_module(m, [closed_form_signed((1, 16, 9, 11), 0.4)], 0.9))
    m = load_closed_form(rblock.RFN(16), 6)
    put("rfn", run_module(m, [closed_form_signed((1, 16, 8, 10), 0.6), closed_form_signed((1, 16, 8, 10), 1.6)], 1.0))

    # NestDecoder with odd sizes so Upsample._pad (core/block.py:981-991) is exercised
    ch = [8, 16, 24, 32]
    dec = load_closed_form(rblock.NestDecoder(rblock.ConvBlock, ch, "nearest"), 7)
    sizes = [(37, 53), (18, 26), (9, 13), (4, 6)]
    feats = [T(closed_form_signed((1, c, h, w), 0.2 * i + 0.1)).requires_grad_(True) for i, (c, (h, w)) in enumerate(zip(ch, sizes))]
    y = dec(feats)
    y.backward(T(closed_form_signed(tuple(y.shape), 1.1)))
    out["nestdec__y"] = y.detach().numpy()
    for i, f in enumerate(feats):
        out[f"nestdec__dx{i}"] = f.grad.numpy()
    for k, p in dec.named_parameters():
        out["nestdec__dp_" + k] = digest(p.grad.numpy())

    # maxpool + nearest upsample on their own
    x = T(closed_form_signed((1, 8, 10, 14), 0.77)).requires_grad_(True)
    y = nn.MaxPool2d(2, 2)(x)
    y.backward(T(closed_form_signed(tuple(y.shape), 0.31)))
    out["maxpool__y"], out["maxpool__dx"] = y.detach().numpy(), x.grad.numpy()
    x = T(closed_form_signed((1, 8, 4, 6), 0.57)).requires_grad_(True)
    y = rblock.Upsample("nearest", 2)(x, (1, 8, 9, 13))
    y.backward(T(closed_form_signed(tuple(y.shape), 0.41)))
    out["upsample__y"], out["upsample__dx"] = y.detach().numpy(), x.grad.numpy()

    # fusion functions
    s = (2, 16, 6, 10)
    a, b = closed_form_signed(s, 0.15), closed_form_signed(s, 1.25)
    gy = closed_form_signed(s, 2.35)
    for mode in ("sum", "mean", "max"):
        ta, tb = T(a).requires_grad_(True), T(b).requires_grad_(True)
        y = rfusion.element_fusion(ta, tb, mode)
        y.backward(T(gy))
        out[f"elem_{mode}__y"], out[f"elem_{mode}__da"], out[f"elem_{mode}__db"] = y.detach().numpy(), ta.grad.numpy(), tb.grad.numpy()
    for mode in ("sa", "ca", "sca"):
        ta, tb = T(a).requires_grad_(True), T(b).requires_grad_(True)
        y = rfusion.attention_fusion(ta, tb, mode)
        y.backward(T(gy))
        out[f"attn_{mode}__y"], out[f"attn_{mode}__da"], out[f"attn_{mode}__db"] = y.detach().numpy(), ta.grad.numpy(), tb.grad.numpy()
    # all-zero features: the clamp(min=1e-7) branch of weighted_fusion (core/fusion.py:33)
    z = np.zeros(s, np.float32)
    ta, tb = T(z).requires_grad_(True), T(z.copy()).requires_grad_(True)
    y = rfusion.attention_fusion(ta, tb, "sca")
    y.backward(T(gy))
    out["attn_zero__y"], out["attn_zero__da"], out["attn_zero__db"] = y.detach().numpy(), ta.grad.numpy(), tb.grad.numpy()
    # post-ReLU style features (non-negative, many exact zeros) as NestFuse produces
    ar, br = np.maximum(a, 0), np.maximum(b, 0)
    ta, tb = T(ar).requires_grad_(True), T(br).requires_grad_(True)
    y = rfusion.attention_fusion(ta, tb, "sca")
    y.backward(T(gy))
    out["attn_relu__y"], out["attn_relu__da"], out["attn_relu__db"] = y.detach().numpy(), ta.grad.numpy(), tb.grad.numpy()
    save("f4_blocks.npz", out)


# ---------------------------------------------------------------- F5
# (model, shape, parameter set): closed-form seed 1, or "live" = oracle.LIVE_PARAMS for the two nets that end in a ReLU
# (core/model.py:344) -- with seed 1 that ReLU is dead on every pixel (y = 0, all gradients 0).  2x36x44 walks the odd pyramid
# 36x44 -> 18x22 -> 9x11 -> 4x5 (Upsample._pad, core/block.py:981-991) with two samples.
F5_CASES = [("PFNetv1", (2, 1, 32, 32), 1), ("PFNetv2", (2, 1, 32, 32), 1), ("DenseFuse", (2, 1, 32, 32), 1),
            ("NestFuse", (1, 1, 32, 32), "live"), ("RFNNest", (1, 1, 32, 32), "live"),
            ("NestFuse", (2, 1, 36, 44), "live"), ("RFNNest", (2, 1, 36, 44), "live"), ("PFNetv1", (1, 1, 37, 53), 1)]


def make_f5():
    out, manifest = {}, {}
    for name, shape, pset in F5_CASES:
        tag = f"{name}_{shape[0]}x{shape[2]}x{shape[3]}"
        model = getattr(rmodel, name)()
        model = load_live(model, name) if pset == "live" else load_closed_form(model, seed=pset)
        manifest[name] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        i1, i2 = T(closed_form_image(shape, 0.3)), T(closed_form_image(shape, 1.7))
        y = model(i1, i2)
        # upstream gradient: a random-sign tensor for the seed-1 cases; the live cases take a smooth positive one (as a loss gives): with
        # random signs every parameter gradient is a sum of ~3000 cancelling terms, and ONE ReLU decision taken the other way on a
        # pre-activation within rounding of zero -- by either fp32 implementation -- moves it by 1 / sqrt(3000) = 2 % (measured on the HIP
        # kernels at 2x36x44: 9e-3 on decode.DB1_3 in BOTH kernel families, 1e-6 on every other case)
        gy = T(closed_form_image(shape, 0.9)) if pset == "live" else T(closed_form_signed(shape, 0.9, 1.0))
        y.backward(gy)
        out[tag + "__y"] = y.detach().numpy()
        if pset == "live":     # post-ReLU output: part of the mask open, part closed
            assert_alive(out[tag + "__y"], tag + "__y", 0.3, 0.7)
        for k, p in model.named_parameters():
            out[f"{tag}__dp_{k}"] = digest(p.grad.numpy())
        if name == "DenseFuse":  # auto-encoder mode, core/model.py:43-51
            out[tag + "__y_ae"] = model(i1).detach().numpy()
    save("f5_models.npz", out)
    json.dump(manifest, open(os.path.join(HERE, "f5_manifest.json"), "w"), indent=0)


# ---------------------------------------------------------------- F6
def make_f6():
    out = {}
    for name in ("PFNetv1", "DenseFuse"):
        model = load_closed_form(getattr(rmodel, name)(), seed=2)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, betas=(0.9, 0.999))
        l_ssim = rloss.SSIMLoss("ssim", weight=1.0)
        l_pix = rloss.PixelLoss("l1", weight=0.01)
        l_grad = rloss.GradLoss("l1", weight=0.1)
        shape = (4, 1, 64, 64)
        rows = []
        for step in range(3):
            i1 = T(closed_form_image(shape, 0.21 + step))
            i2 = T(closed_form_image(shape, 1.43 + step))
            opt.zero_grad(set_to_none=True)
            f = model(i1, i2)
            a, b, c = l_ssim(i1, i2, f), l_pix(i1, i2, f, mode="max"), l_grad(i1, i2, f, mode="max")
            tot = a + b + c
            tot.backward()
            norm = nn.utils.clip_grad_norm_(model.parameters(), max_norm=5)
            opt.step()
            rows.append([a.item(), b.item(), c.item(), tot.item(), float(norm)])
            if step == 0:
                out[name + "__imgf0"] = f.detach().numpy()
        out[name + "__rows"] = np.array(rows, dtype=np.float64)
        for k, p in model.state_dict().items():
            out[f"{name}__w_{k}"] = digest(p.numpy())
    save("f6_traj.npz", out)


def make_f10():
    """VIFNet: the PFNet/DenseFuse-style net with a shared encoder, concat fusion and PFNetv1's decoder."""
    out, manifest = {}, {}
    for shape in ((2, 1, 32, 32), (1, 1, 37, 53)):
        tag = f"VIFNet_{shape[0]}x{shape[2]}x{shape[3]}"
        model = load_closed_form(rmodel.VIFNet(), seed=1)
        manifest["VIFNet"] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        i1, i2 = T(closed_form_image(shape, 0.3)), T(closed_form_image(shape, 1.7))
        y = model(i1, i2)
        y.backward(T(closed_form_signed(shape, 0.9, 1.0)))
        out[tag + "__y"] = y.detach().numpy()
        for k, p in model.named_parameters():
            out[f"{tag}__dp_{k}"] = digest(p.grad.numpy())
    save("f10_vifnet.npz", out)
    json.dump(manifest, open(os.path.join(HERE, "f10_manifest.json"), "w"), indent=0)


def make_f7():
    """core/metric.py calc_ssim as test.py uses it (data_range=1.0) and with its default data_range=255."""
    import core.metric as rmetric
    out = {}
    for tag, shape, scale, kw in (("unit_2x40x52", (2, 1, 40, 52), 1.0, dict(data_range=1.0)),
                                  ("unit_1x64x64", (1, 1, 64, 64), 1.0, dict(data_range=1.0)),
                                  ("u8range_1x64x64", (1, 1, 64, 64), 255.0, dict())):
        a = T(closed_form_image(shape, 0.37) * scale)
        b = T(closed_form_image(shape, 1.91) * scale)
        with torch.no_grad():
            s_ab = rmetric.calc_ssim(a, b, **kw)
            s_aa = rmetric.calc_ssim(a, a, **kw)
            s_full, cs_full = rmetric.calc_ssim(a, b, full=True, **kw)
        out[tag] = {"shape": list(shape), "scale": scale, "kwargs": kw, "ssim": float(s_ab), "ssim_self": float(s_aa),
                    "ssim_full": float(s_full), "cs_full": float(cs_full)}
    json.dump(out, open(os.path.join(HERE, "f7_metric_ssim.json"), "w"), indent=1)


def feed_patch(P, seed):
    """Closed-form uint8 patch without symmetries."""
    y, x = np.mgrid[0:P, 0:P]
    return ((y * 37 + x * 11 + (y * x) * 5 + seed * 13) % 256).astype(np.uint8)


def make_f8():
    """data/transform.py as FusionPatches.__getitem__ applies it (data/patches.py:61-74): norm, then transform."""
    sys.path.insert(0, os.path.join(REF, "data"))
    import transform as rtf   # the reference's data/transform.py (data/ has no __init__-free import path of its own)
    out = {}
    for P in (5, 6):
        patch = feed_patch(P, P).astype(np.float32)
        for nm, tag in ((None, "none"), ("min-max", "minmax"), ("z-score", "zscore")):
            n = rtf.norm(patch.copy(), mode=nm)
            for mode in range(8):
                out[f"P{P}_{tag}_m{mode}"] = np.ascontiguousarray(rtf.transform(n, mode=mode)).astype(np.float32)
    save("f8_feed.npz", out)


def make_f9():
    """The SSIMLoss modes beyond 'ssim' and TVLoss, on closed-form images (value + gradient w.r.t. the fused image)."""
    out = {}
    def run(tag, fn, shape, phases=(0.3, 1.7, 2.9)):
        i1, i2 = T(closed_form_image(shape, phases[0])), T(closed_form_image(shape, phases[1]))
        f = T(closed_form_image(shape, phases[2])).requires_grad_(True)
        loss = fn(i1, i2, f)
        loss.backward()
        out[tag + "__loss"] = np.float64(loss.item())
        out[tag + "__grad"] = f.grad.numpy()
    for mode, shapes in (("w-ssim", [(2, 1, 40, 52), (3, 1, 33, 47)]), ("msw-ssim", [(2, 1, 40, 52), (1, 1, 33, 47)]),
                         ("ms-ssim", [(1, 1, 192, 208), (2, 1, 193, 211)])):
        for shape in shapes:
            fn = rloss.SSIMLoss(mode, weight=0.7)
            run(f"{mode}_{shape[0]}x{shape[2]}x{shape[3]}", fn, shape)
    # flat source image: sigma clamps (1e-4) and the gamma denominators
    for mode in ("w-ssim", "msw-ssim"):
        shape = (2, 1, 24, 24)
        i1 = T(np.full(shape, 0.4, np.float32)); i2 = T(closed_form_image(shape, 1.1))
        f = T(closed_form_image(shape, 2.2)).requires_grad_(True)
        loss = rloss.SSIMLoss(mode)(i1, i2, f)
        loss.backward()
        out[f"{mode}_flat__loss"] = np.float64(loss.item())
        out[f"{mode}_flat__grad"] = f.grad.numpy()
    for mode in ("l1", "l2"):
        shape = (2, 1, 21, 34)
        x = T(closed_form_image(shape, 0.77)).requires_grad_(True)
        loss = rloss.TVLoss(mode, weight=0.3)(x)
        loss.backward()
        out[f"tv_{mode}__loss"] = np.float64(loss.item())
        out[f"tv_{mode}__grad"] = x.grad.numpy()
    save("f9_ssim_modes.npz", out)


def make_f16():
    """Argument combinations outside the HIP kernels (stock torch fallbacks that must not change results)."""
    import core.metric as rmetric
    out = {}
    shape = (2, 1, 40, 52)
    i1, i2 = T(closed_form_image(shape, 0.3)), T(closed_form_image(shape, 1.7))
    for mode, shp in (("ssim", shape), ("w-ssim", shape), ("msw-ssim", shape), ("ms-ssim", (1, 1, 192, 208))):
        a, b = T(closed_form_image(shp, 0.3)), T(closed_form_image(shp, 1.7))
        f = T(closed_form_image(shp, 2.9)).requires_grad_(True)
        loss = rloss.SSIMLoss(mode, use_padding=True, weight=0.7)(a, b, f)
        loss.backward()
        out[f"pad_{mode}__loss"] = np.float64(loss.item())
        out[f"pad_{mode}__grad"] = f.grad.numpy()
    f = T(closed_form_image(shape, 2.9))
    for tag, mod in (("ssim_maps", rloss.SSIM(11, 1.0, False, False)), ("ssim_pad7", rloss.SSIM(7, 1.0, True, True))):
        res = mod(i1, f)
        for k, v in res.items():
            out[f"{tag}__{k}"] = v.numpy()
    out["msssim_pad"] = rloss.MS_SSIM(11, 1.0, True, True)(T(closed_form_image((1, 1, 192, 208), 0.3)), T(closed_form_image((1, 1, 192, 208), 2.9))).numpy()
    out["mswssim_avg"] = np.float64(rloss.MSW_SSIM((11, 7, 3), 1.0, False, True)(i1, i2, f).item())
    s, c = rmetric.calc_ssim(i1, f, win_size=7, data_range=1.0, use_padding=True, full=True)
    out["metric_w7_pad_full"] = np.array([s.item(), c.item()], np.float64)
    out["metric_small"] = np.float64(rmetric.calc_ssim(i1[:, :, :9, :20], f[:, :, :9, :20], data_range=1.0).item())
    out["metric_maps"] = rmetric.calc_ssim(i1, f, data_range=1.0, size_average=False).numpy()
    t = T(closed_form_signed((2, 6, 9, 13), 0.9)).requires_grad_(True)
    v = rfusion.channel_pooling(t, 'nuclear')
    (v * T(np.arange(1, 7, dtype=np.float32).reshape(1, 6, 1, 1))).sum().backward()
    out["nuclear__y"] = v.detach().numpy()
    out["nuclear__dx"] = t.grad.numpy()
    save("f16_stock_fallbacks.npz", out)


def make_f17():
    """The reference's PFNetv1 initialisation after torch.manual_seed(0) (core/block.py init): per state_dict entry its shape and the
    sha256 of its float32 bytes, so that a test can check the mirror's init bit for bit without the reference."""
    import hashlib
    torch.manual_seed(0)
    sd = rmodel.PFNetv1().state_dict()
    out = {"model": "PFNetv1", "seed": 0, "torch": torch.__version__,
           "tensors": [[k, list(v.shape), str(v.dtype), hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest()] for k, v in sd.items()]}
    json.dump(out, open(os.path.join(HERE, "f17_reference_init.json"), "w"), indent=0)


def make_f18():
    """The layout of the reference's demo sample folders (data/samples: relative path, width, height, PIL mode, format of every image), so
    that a test can rebuild a stand-in tree of the same names, sizes and colour modes."""
    from PIL import Image
    base = os.path.join(REF, "data", "samples")
    files = []
    for dirpath, _, names in sorted(os.walk(base)):
        for n in sorted(names):
            p = os.path.join(dirpath, n)
            with Image.open(p) as im:
                files.append([os.path.relpath(p, base).replace(os.sep, "/"), im.size[0], im.size[1], im.mode, im.format])
    json.dump({"files": files}, open(os.path.join(HERE, "f18_sample_folders.json"), "w"), indent=0)


if __name__ == "__main__":
    which = sys.argv[1:] or ["f1", "f2", "f3", "f4", "f5", "f6", "f7", "f8", "f9", "f10", "f11", "f12", "f13", "f14", "f15", "f16", "f17", "f18"]
    for w in which:
        globals()["make_" + w]()
        print("wrote", w)
