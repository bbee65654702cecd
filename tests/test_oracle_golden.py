"""Pin the CPU oracle (oracle/fusion_oracle.py) to the reference's own outputs.

The fixtures under tests/golden/ were produced by importing the reference
(tests/golden/make_golden.py); inputs/parameters are closed-form and rebuilt here.
Tolerances: fp32 oracle vs fp32 reference (different summation order) -> 2e-5 relative to the
tensor's max-abs; the fp64 oracle run tightens logic errors vs rounding.
"""
import json
import os

import numpy as np
import pytest

from oracle import fusion_oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")


def close(a, b, rtol=2e-5, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(np.abs(b).max(), 1e-12)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, f"{what}: max err {err:.3e} (scale {scale:.3e})"


def digest(a):
    f = np.asarray(a, dtype=np.float32).reshape(-1)
    n = f.size
    idx = (np.arange(16) * max(1, n // 16)) % n
    return np.concatenate(([f.astype(np.float64).sum(), np.abs(f.astype(np.float64)).sum()],
                           f[:16] if n >= 16 else np.pad(f, (0, 16 - n)), f[idx])).astype(np.float64)


def close_digest(arr, dg, rtol=5e-5, what=""):
    mine = digest(arr)
    scale = max(np.abs(np.asarray(arr)).max(), 1e-12)
    n = np.asarray(arr).size
    # sums accumulate rounding over n elements
    assert abs(mine[0] - dg[0]) <= rtol * scale * max(1.0, np.sqrt(n)) * 4, (what, "sum", mine[0], dg[0])
    assert abs(mine[1] - dg[1]) <= rtol * max(dg[1], scale), (what, "abs-sum", mine[1], dg[1])
    assert np.abs(mine[2:] - dg[2:]).max() <= rtol * scale, (what, "samples", np.abs(mine[2:] - dg[2:]).max(), scale)


# ------------------------------------------------------------------ F1
def test_f1_known_answer_losses():
    import torch
    ref = json.load(open(os.path.join(G, "f1_loss_known_answer.json")))
    torch.manual_seed(0)
    x1 = torch.rand(2, 1, 256, 256).numpy()
    x2 = torch.rand(2, 1, 256, 256).numpy()
    y = torch.rand(2, 1, 256, 256).numpy()
    np.testing.assert_allclose(x1.reshape(-1)[:8], ref["x1_head"], rtol=0, atol=0)
    np.testing.assert_allclose(y.reshape(-1)[:8], ref["y_head"], rtol=0, atol=0)
    np.testing.assert_allclose(O.gaussian_window_1d(), ref["window_1d"], rtol=0, atol=0)
    assert abs(float(O.create_window().astype(np.float64).sum()) - ref["window_2d_sum"]) < 1e-7
    l, _ = O.ssim_loss(x1, x2, y, 1.0, need_grad=False)
    assert abs(l - ref["ssim"]) < 2e-6
    # the values printed by core/loss.py:419-423 (4 decimals) and SURVEY section 4
    assert abs(l - 0.9944541454) < 2e-6
    l, _ = O.pixel_loss(x1, x2, y, 0.01, "avg", False)
    assert abs(l - ref["pixel_avg"]) < 1e-8
    l, _ = O.grad_loss(x1, x2, y, 0.1, "avg", False)
    assert abs(l - ref["grad_avg"]) < 5e-7
    lp, _ = O.pixel_loss(x1, x2, y, 0.01, "max", False)
    assert abs(lp - ref["pixel_max"]) < 1e-8
    lg, _ = O.grad_loss(x1, x2, y, 0.1, "max", False)
    assert abs(lg - ref["grad_max"]) < 5e-7
    (a, b, c, tot), _ = O.fusion_losses(x1, x2, y, need_grad=False)
    assert abs(tot - ref["total_max"]) < 3e-6
    s, _ = O.ssim_terms(x1, y, O.create_window())
    np.testing.assert_allclose(s, ref["ssim_per_sample_x1_y"], atol=2e-7)


# ------------------------------------------------------------------ F2
def f2_inputs(case):
    if case == "a":
        s = (2, 1, 32, 32)
        return O.closed_form_image(s, 0.1), O.closed_form_image(s, 1.3), O.closed_form_image(s, 2.2)
    if case == "b":
        s = (1, 1, 64, 48)
        return O.closed_form_image(s, 0.7), O.closed_form_image(s, 0.2), O.closed_form_image(s, 1.9)
    if case == "c":
        s = (1, 1, 24, 24)
        return O.closed_form_image(s, 0.4), O.closed_form_image(s, 1.1), np.full(s, 0.375, np.float32)
    if case == "d":
        s = (2, 1, 20, 28)
        a = O.closed_form_image(s, 0.9)
        return a, a.copy(), O.closed_form_image(s, 2.9)
    raise KeyError(case)


@pytest.mark.parametrize("case", list("abcd"))
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_f2_loss_values_and_grads(case, dt):
    ref = np.load(os.path.join(G, "f2_loss_grads.npz"))
    i1, i2, f = (a.astype(dt) for a in f2_inputs(case))
    l1, g1 = O.ssim_loss(i1, i2, f, 1.0)
    l2, g2 = O.pixel_loss(i1, i2, f, 0.01, "max")
    l3, g3 = O.grad_loss(i1, i2, f, 0.1, "max")
    assert abs(l1 - ref[f"{case}_l_ssim"]) < 3e-6
    assert abs(l2 - ref[f"{case}_l_pixel"]) < 1e-7
    assert abs(l3 - ref[f"{case}_l_grad"]) < 1e-6
    # case c: constant f makes the reference's own fp32 SSIM gradient ill-conditioned (sigma_f^2
    # is pure rounding noise around the clamp); compare it loosely there.
    rt = 5e-3 if case == "c" else (2e-4 if dt == np.float32 else 2e-4)
    close(g1, ref[f"{case}_g_ssim"], rt, "g_ssim")
    close(g2, ref[f"{case}_g_pixel"], 1e-6, "g_pixel")
    close(g3, ref[f"{case}_g_grad"], 1e-6, "g_grad")
    close(g1 + g2 + g3, ref[f"{case}_g_total"], rt, "g_total")
    la, _ = O.pixel_loss(i1, i2, f, 0.01, "avg", False)
    lb, _ = O.grad_loss(i1, i2, f, 0.1, "avg", False)
    assert abs(la - ref[f"{case}_l_pixel_avg"]) < 1e-7
    assert abs(lb - ref[f"{case}_l_grad_avg"]) < 1e-6


# ------------------------------------------------------------------ F3
F3_CASES = [
    ("c1_16", 1, 16, 3, True, 2, 12, 20), ("c16_16", 16, 16, 3, True, 2, 12, 20),
    ("c48_16", 48, 16, 3, True, 2, 12, 20), ("c128_64", 128, 64, 3, True, 2, 12, 20),
    ("c16_1_lin", 16, 1, 3, False, 2, 12, 20), ("c8_64_k1", 8, 64, 1, True, 2, 12, 20),
    ("c88_64_k1", 88, 64, 1, True, 2, 12, 20), ("c16_16_thin_h", 16, 16, 3, True, 1, 2, 9),
    ("c16_16_thin_w", 16, 16, 3, True, 1, 9, 2), ("c32_16_odd", 32, 16, 3, True, 1, 37, 53),
]


def f3_tensors(case):
    name, cin, cout, k, relu, N, H, W = case
    w = O.closed_form_param(0, "layers.0.weight", (cout, cin, k, k), 3)
    b = O.closed_form_param(1, "layers.0.bias", (cout,), 3)
    x = O.closed_form_signed((N, cin, H, W), 0.5, 1.0)
    gy = O.closed_form_signed((N, cout, H, W), 1.5, 1.0)
    return x, w, b, gy


@pytest.mark.parametrize("case", F3_CASES, ids=[c[0] for c in F3_CASES])
def test_f3_conv_layer(case):
    ref = {**np.load(os.path.join(G, "f3_conv.npz")), **np.load(os.path.join(G, "f3_conv_2.npz"))}
    name, relu = case[0], case[4]
    x, w, b, gy = f3_tensors(case)
    y = O.conv2d_reflect_fwd(x, w, b, relu)
    close(y, ref[name + "_y"], 2e-5, "y")
    gx, gw, gb = O.conv2d_reflect_bwd(x, w, y, gy, relu)
    close(gx, ref[name + "_dx"], 2e-5, "dx")
    close(gw, ref[name + "_dw"], 2e-5, "dw")
    close(gb, ref[name + "_db"], 2e-5, "db")


# ------------------------------------------------------------------ F4
def _params(mod, seed):
    return O.OrderedDict((k, O.closed_form_param(i, k, s, seed)) for i, (k, s) in enumerate(mod.param_shapes().items()))


def _check_dp(ref, prefix, Gd, strip=""):
    keys = [k for k in ref.files if k.startswith(prefix + "__dp_")]
    assert keys
    for k in keys:
        name = k[len(prefix) + 5:]
        close_digest(Gd[strip + name], ref[k], 5e-5, name)


def test_f4_dense_block():
    ref = np.load(os.path.join(G, "f4_blocks.npz"))
    m = O.DenseBlock("", 16, 16)
    # reference keys are 'layers.i.layers.0.weight'; oracle prefix '' gives '.layers.i...'
    P = O.OrderedDict((k, O.closed_form_param(i, k, s, 4)) for i, (k, s) in enumerate(m.param_shapes().items()))
    x = O.closed_form_signed((2, 16, 10, 14), 0.3)
    y = m.forward(P, x)
    close(y, ref["dense__y"], 2e-5, "y")
    Gd = {}
    gx = m.backward(P, Gd, O.closed_form_signed(y.shape, 0.8))
    close(gx, ref["dense__dx0"], 2e-5, "dx")
    _check_dp(ref, "dense", Gd, strip=".")


def test_f4_convblock_and_rfn():
    ref = np.load(os.path.join(G, "f4_blocks.npz"))
    m = O.ConvBlock("", 16, 64)
    P = _params(m, 5)
    x = O.closed_form_signed((1, 16, 9, 11), 0.4)
    y = m.forward(P, x)
    close(y, ref["convblock__y"], 2e-5)
    Gd = {}
    close(m.backward(P, Gd, O.closed_form_signed(y.shape, 0.9)), ref["convblock__dx0"], 2e-5)
    _check_dp(ref, "convblock", Gd, strip=".")

    m = O.RFN("", 16)
    P = _params(m, 6)
    x1, x2 = O.closed_form_signed((1, 16, 8, 10), 0.6), O.closed_form_signed((1, 16, 8, 10), 1.6)
    y = m.forward(P, x1, x2)
    close(y, ref["rfn__y"], 2e-5)
    Gd = {}
    g1, g2 = m.backward(P, Gd, O.closed_form_signed(y.shape, 1.0))
    close(g1, ref["rfn__dx0"], 2e-5)
    close(g2, ref["rfn__dx1"], 2e-5)
    _check_dp(ref, "rfn", Gd, strip=".")


def test_f4_pool_upsample():
    ref = np.load(os.path.join(G, "f4_blocks.npz"))
    x = O.closed_form_signed((1, 8, 10, 14), 0.77)
    y, idx = O.maxpool2x2_fwd(x)
    close(y, ref["maxpool__y"], 0)
    close(O.maxpool2x2_bwd(O.closed_form_signed(y.shape, 0.31), idx, x.shape), ref["maxpool__dx"], 0)
    x = O.closed_form_signed((1, 8, 4, 6), 0.57)
    y = O.upsample_nearest2x_fwd(x, (9, 13))
    close(y, ref["upsample__y"], 0)
    close(O.upsample_nearest2x_bwd(O.closed_form_signed(y.shape, 0.41), x.shape), ref["upsample__dx"], 1e-6)


def test_f4_fusion_functions():
    ref = np.load(os.path.join(G, "f4_blocks.npz"))
    s = (2, 16, 6, 10)
    a, b, gy = O.closed_form_signed(s, 0.15), O.closed_form_signed(s, 1.25), O.closed_form_signed(s, 2.35)
    for mode in ("sum", "mean", "max"):
        close(O.element_fusion(a, b, mode), ref[f"elem_{mode}__y"], 1e-6)
        da, db = O.element_fusion_bwd(a, b, gy, mode)
        close(da, ref[f"elem_{mode}__da"], 1e-6)
        close(db, ref[f"elem_{mode}__db"], 1e-6)
    for mode in ("sa", "ca", "sca"):
        close(O.attention_fusion(a, b, mode), ref[f"attn_{mode}__y"], 2e-5, mode)
        da, db = O.attention_fusion_bwd(a, b, gy, mode)
        close(da, ref[f"attn_{mode}__da"], 5e-5, mode)
        close(db, ref[f"attn_{mode}__db"], 5e-5, mode)
    z = np.zeros(s, np.float32)
    close(O.attention_fusion(z, z, "sca"), ref["attn_zero__y"], 0)
    da, db = O.attention_fusion_bwd(z, z, gy, "sca")
    close(da, ref["attn_zero__da"], 1e-6)
    close(db, ref["attn_zero__db"], 1e-6)
    ar, br = np.maximum(a, 0), np.maximum(b, 0)
    close(O.attention_fusion(ar, br, "sca"), ref["attn_relu__y"], 2e-5)
    da, db = O.attention_fusion_bwd(ar, br, gy, "sca")
    close(da, ref["attn_relu__da"], 5e-5)
    close(db, ref["attn_relu__db"], 5e-5)
    with pytest.raises(ValueError):
        O.element_fusion(a, b, "nope")
    with pytest.raises(ValueError):
        O.attention_fusion(a, b, "nope")


# ------------------------------------------------------------------ F5
# parameter set: closed-form seed 1, or "live" (oracle.LIVE_PARAMS) for the nets whose last layer is a ReLU -- seed 1 kills it everywhere
F5_CASES = [("PFNetv1", (2, 1, 32, 32), 1), ("PFNetv2", (2, 1, 32, 32), 1), ("DenseFuse", (2, 1, 32, 32), 1),
            ("NestFuse", (1, 1, 32, 32), "live"), ("RFNNest", (1, 1, 32, 32), "live"),
            ("NestFuse", (2, 1, 36, 44), "live"), ("RFNNest", (2, 1, 36, 44), "live"), ("PFNetv1", (1, 1, 37, 53), 1)]


@pytest.mark.parametrize("name,shape,pset", F5_CASES, ids=[f"{n}-{s[0]}x{s[2]}x{s[3]}" for n, s, _ in F5_CASES])
def test_f5_models(name, shape, pset):
    ref = np.load(os.path.join(G, "f5_models.npz"))
    man = json.load(open(os.path.join(G, "f5_manifest.json")))
    tag = f"{name}_{shape[0]}x{shape[2]}x{shape[3]}"
    m = O.MODELS[name]()
    assert [[k, list(s)] for k, s in m.param_shapes().items()] == man[name]
    P = m.init_params_live() if pset == "live" else m.init_params(seed=pset)
    i1, i2 = O.closed_form_image(shape, 0.3), O.closed_form_image(shape, 1.7)
    y = m.forward(P, i1, i2)
    if pset == "live":
        O.assert_alive(ref[tag + "__y"], tag, 0.3, 0.7)
    close(y, ref[tag + "__y"], 5e-5, "y")
    Gd = m.backward(P, O.closed_form_image(shape, 0.9) if pset == "live" else O.closed_form_signed(shape, 0.9, 1.0))
    for k in P:
        close_digest(Gd[k], ref[f"{tag}__dp_{k}"], 1e-4, k)
    if name == "DenseFuse":
        close(m.forward(P, i1), ref[tag + "__y_ae"], 5e-5, "auto-encoder")


def test_no_golden_fixture_is_all_zero():
    """a fixture that is all-zero pins nothing: every tensor of every committed fixture is alive except the ones that are zero by the
    definition of their case (the list the generator's save() gate uses)"""
    import glob
    zero_by_design = {"attn_zero__y", "attn_zero__da", "c_g_grad", "bn_eval_buf_layers.1.num_batches_tracked",
                      "PMGI_2x32x32__buf_transfer1.1.layers.1.num_batches_tracked", "PMGI_1x19x26__buf_transfer1.1.layers.1.num_batches_tracked"}
    files = sorted(glob.glob(os.path.join(G, "*.npz")))
    assert len(files) >= 13
    for f in files:
        d = np.load(f)
        for k in d.files:
            if k not in zero_by_design:
                O.assert_alive(d[k], f"{os.path.basename(f)}:{k}")


# ------------------------------------------------------------------ F6
@pytest.mark.parametrize("name", ["PFNetv1", "DenseFuse"])
def test_f6_train_trajectory(name):
    ref = np.load(os.path.join(G, "f6_traj.npz"))
    m = O.MODELS[name]()
    P = m.init_params(seed=2)
    st = O.AdamState(P)
    shape = (4, 1, 64, 64)
    rows = ref[name + "__rows"]
    for step in range(3):
        i1, i2 = O.closed_form_image(shape, 0.21 + step), O.closed_form_image(shape, 1.43 + step)
        r = O.train_step(m, P, st, i1, i2)
        if step == 0:
            close(r["imgf"], ref[name + "__imgf0"], 5e-5, "imgf")
        got = list(r["losses"]) + [r["grad_norm"]]
        np.testing.assert_allclose(got, rows[step], rtol=2e-4, atol=2e-6, err_msg=f"step {step}")
    for k in P:
        close_digest(P[k], ref[f"{name}__w_{k}"], 2e-5, k)


def test_f7_metric_calc_ssim():
    """core/metric.py calc_ssim (test.py's per-image SSIM) -- oracle vs the reference's values."""
    ref = json.load(open(os.path.join(G, "f7_metric_ssim.json")))
    for tag, r in ref.items():
        shape = tuple(r["shape"])
        a = O.closed_form_image(shape, 0.37) * np.float32(r["scale"])
        b = O.closed_form_image(shape, 1.91) * np.float32(r["scale"])
        dr = r["kwargs"].get("data_range", 255.0)
        s, cs = O.metric_calc_ssim(a, b, dr, full=True)
        assert abs(float(s) - r["ssim"]) <= 2e-5, (tag, float(s), r["ssim"])
        assert abs(float(cs) - r["cs_full"]) <= 2e-5, (tag, float(cs), r["cs_full"])
        assert abs(float(O.metric_calc_ssim(a, a, dr)) - r["ssim_self"]) <= 1e-6


F9_SSIM = [("w-ssim", (2, 1, 40, 52)), ("w-ssim", (3, 1, 33, 47)), ("msw-ssim", (2, 1, 40, 52)), ("msw-ssim", (1, 1, 33, 47)),
           ("ms-ssim", (1, 1, 192, 208)), ("ms-ssim", (2, 1, 193, 211))]


@pytest.mark.parametrize("mode,shape", F9_SSIM, ids=[f"{m}-{s[0]}x{s[2]}x{s[3]}" for m, s in F9_SSIM])
def test_f9_ssim_modes(mode, shape):
    """SSIMLoss 'w-ssim' / 'ms-ssim' / 'msw-ssim' (weight 0.7): oracle value + explicit gradient vs the reference's autograd."""
    ref = np.load(os.path.join(G, "f9_ssim_modes.npz"))
    tag = f"{mode}_{shape[0]}x{shape[2]}x{shape[3]}"
    i1, i2, f = O.closed_form_image(shape, 0.3), O.closed_form_image(shape, 1.7), O.closed_form_image(shape, 2.9)
    loss, grad = O.ssim_mode_loss(i1, i2, f, mode, weight=0.7)
    assert abs(float(loss) - float(ref[tag + "__loss"])) <= 2e-5, (float(loss), float(ref[tag + "__loss"]))
    close(grad, ref[tag + "__grad"], 2e-4, tag)


@pytest.mark.parametrize("mode", ["w-ssim", "msw-ssim"])
def test_f9_flat_source_clamps(mode):
    ref = np.load(os.path.join(G, "f9_ssim_modes.npz"))
    shape = (2, 1, 24, 24)
    i1, i2, f = np.full(shape, 0.4, np.float32), O.closed_form_image(shape, 1.1), O.closed_form_image(shape, 2.2)
    loss, grad = O.ssim_mode_loss(i1, i2, f, mode)
    assert abs(float(loss) - float(ref[f"{mode}_flat__loss"])) <= 2e-5
    close(grad, ref[f"{mode}_flat__grad"], 2e-4, mode)


@pytest.mark.parametrize("mode", ["l1", "l2"])
def test_f9_tv_loss(mode):
    ref = np.load(os.path.join(G, "f9_ssim_modes.npz"))
    x = O.closed_form_image((2, 1, 21, 34), 0.77)
    loss, grad = O.tv_loss(x, mode, weight=0.3)
    assert abs(float(loss) - float(ref[f"tv_{mode}__loss"])) <= 1e-6
    close(grad, ref[f"tv_{mode}__grad"], 1e-5, mode)


@pytest.mark.parametrize("shape", [(2, 1, 32, 32), (1, 1, 37, 53)], ids=["2x32x32", "1x37x53"])
def test_f10_vifnet(shape):
    """VIFNet (shared encoder + concat + PFNetv1 decoder): oracle forward / explicit backward vs the reference (golden F10)."""
    ref = np.load(os.path.join(G, "f10_vifnet.npz"))
    man = json.load(open(os.path.join(G, "f10_manifest.json")))
    tag = f"VIFNet_{shape[0]}x{shape[2]}x{shape[3]}"
    m = O.VIFNet()
    assert [[k, list(v)] for k, v in m.param_shapes().items()] == man["VIFNet"]
    P = m.init_params(seed=1)
    y = m.forward(P, O.closed_form_image(shape, 0.3), O.closed_form_image(shape, 1.7))
    close(y, ref[tag + "__y"], 2e-5, "imgf")
    Gd = m.backward(P, O.closed_form_signed(shape, 0.9, 1.0))
    for k in m.param_shapes():
        close_digest(Gd[k], ref[f"{tag}__dp_{k}"], 5e-5, k)


# ------------------------------------------------------------------ F11: general ConvLayer forms (k 5/7, stride 2, zero padding, ConvTranspose2d)
#            name            cin cout k  stride transposed padding_mode relu  N  H   W
F11_CASES = [("k5_1_16", 1, 16, 5, 1, False, "reflect", True, 2, 13, 17), ("k7_16_32", 16, 32, 7, 1, False, "reflect", True, 1, 12, 20),
             ("k7_tiny", 8, 8, 7, 1, False, "reflect", True, 1, 4, 5), ("k5_16_1_lin", 16, 1, 5, 1, False, "reflect", False, 2, 9, 11),
             ("s2_32_64", 32, 64, 3, 2, False, "reflect", True, 2, 13, 18), ("s2_even", 24, 16, 3, 2, False, "reflect", True, 1, 16, 32),
             ("zeros_k3", 16, 24, 3, 1, False, "zeros", True, 1, 10, 9), ("convT_24_16", 24, 16, 3, 2, True, "zeros", True, 2, 7, 9),
             ("convT_lin", 8, 12, 3, 2, True, "zeros", False, 1, 5, 4)]


def f11_tensors(case):
    name, cin, cout, k, stride, transposed, pmode, relu, N, H, W = case
    w = O.closed_form_param(0, "layers.0.weight", (cin, cout, k, k) if transposed else (cout, cin, k, k), 11)
    b = O.closed_form_param(1, "layers.0.bias", (cout,), 11)
    x = O.closed_form_signed((N, cin, H, W), 0.5, 1.0)
    return w, b, x


@pytest.mark.parametrize("case", F11_CASES, ids=[c[0] for c in F11_CASES])
def test_f11_general_conv_oracle_vs_reference(case):
    """oracle conv2d_general_* / conv_transpose2d_* == the reference's ConvLayer (nn.Conv2d / nn.ConvTranspose2d autograd)."""
    name, cin, cout, k, stride, transposed, pmode, relu, N, H, W = case
    g = np.load(os.path.join(G, "f11_general_conv.npz"))
    w, b, x = f11_tensors(case)
    if transposed:
        y = O.conv_transpose2d_fwd(x, w, b, stride, k // 2, 1, relu)
    else:
        y = O.conv2d_general_fwd(x, w, b, stride, k // 2, pmode == "reflect", relu)
    assert y.shape == g[name + "_y"].shape
    gy = O.closed_form_signed(y.shape, 1.5, 1.0)
    if transposed:
        dx, dw, db = O.conv_transpose2d_bwd(x, w, y, gy, stride, k // 2, 1, relu)
    else:
        dx, dw, db = O.conv2d_general_bwd(x, w, y, gy, stride, k // 2, pmode == "reflect", relu)
    for got, key in ((y, "_y"), (dx, "_dx"), (dw, "_dw"), (db, "_db")):
        ref = g[name + key]
        assert np.abs(got - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), (name, key)


# ------------------------------------------------------------------ F13: norm / activation epilogues of ConvLayer
#             name        cin cout k stride transposed norm act  train  N  H   W
F13_CASES = [("bn_relu", 16, 24, 3, 1, False, "bn", "relu", True, 3, 10, 12), ("bn_eval", 16, 24, 3, 1, False, "bn", "relu", False, 2, 9, 8),
             ("bn_lin", 8, 16, 3, 1, False, "bn", None, True, 2, 7, 9), ("bn_leaky_k5", 3, 16, 5, 1, False, "bn", "leaky", True, 2, 12, 11),
             ("bn_leaky_k1", 32, 16, 1, 1, False, "bn", "leaky", True, 2, 6, 7), ("gn_relu", 1, 64, 3, 1, False, "gn", "relu", True, 2, 10, 10),
             ("gn_s2", 24, 32, 3, 2, False, "gn", "relu", True, 2, 11, 14), ("gn_convT", 32, 16, 3, 2, True, "gn", "relu", True, 2, 5, 6),
             ("tanh_k1", 40, 1, 1, 1, False, None, "tanh", True, 2, 8, 9), ("leaky_k3", 16, 16, 3, 1, False, None, "leaky", True, 1, 9, 9)]


def f13_params(case):
    name, cin, cout, k, stride, transposed, norm, act, train, N, H, W = case
    keys = ["layers.0.weight", "layers.0.bias"]
    shapes = [(cin, cout, k, k) if transposed else (cout, cin, k, k), (cout,)]
    if norm:
        keys += ["layers.1.weight", "layers.1.bias"]
        shapes += [(cout,), (cout,)]
    if norm == "bn":
        keys += ["layers.1.running_mean", "layers.1.running_var", "layers.1.num_batches_tracked"]
        shapes += [(cout,), (cout,), ()]
    P = {kk: O.closed_form_param(i, kk, sh, 13) for i, (kk, sh) in enumerate(zip(keys, shapes))}
    if norm == "bn":
        P["layers.1.running_var"] = np.abs(P["layers.1.running_var"]) + 0.5
    return P


@pytest.mark.parametrize("case", F13_CASES, ids=[c[0] for c in F13_CASES])
def test_f13_norm_act_oracle_vs_reference(case):
    """oracle conv + norm_act_fwd/bwd == the reference's ConvLayer(norm=BatchNorm2d | GroupNorm, act=ReLU | LeakyReLU | Tanh):
    output, input / weight / affine gradients, running statistics after the step."""
    name, cin, cout, k, stride, transposed, norm, act, train, N, H, W = case
    g = np.load(os.path.join(G, "f13_n4_norm.npz"))
    P = f13_params(case)
    w, b = P["layers.0.weight"], P["layers.0.bias"]
    x = O.closed_form_signed((N, cin, H, W), 0.5, 1.0)
    p = k // 2
    z = O.conv_transpose2d_fwd(x, w, b, stride, p, 1, False) if transposed else O.conv2d_general_fwd(x, w, b, stride, p, True, False)
    running = None
    if norm:
        gamma, beta = P["layers.1.weight"], P["layers.1.bias"]
        kind = "gn" if norm == "gn" else ("bn" if train else "bn_eval")
        if norm == "bn":
            running = [P["layers.1.running_mean"].copy(), P["layers.1.running_var"].copy()]
        y, cache = O.norm_act_fwd(z, gamma, beta, kind, act, 1e-5, running)
    else:
        y = O._act(z, act)
    gy = O.closed_form_signed(y.shape, 1.5, 1.0)
    if norm:
        dz, dg, dbt = O.norm_act_bwd(cache, y, gy, gamma)
    else:
        dz = gy * O._act_dydz(y, act)
    dx, dw, db = (O.conv_transpose2d_bwd(x, w, z, dz, stride, p, 1, False) if transposed else O.conv2d_general_bwd(x, w, z, dz, stride, p, True, False))
    pairs = [(y, "_y"), (dx, "_dx"), (dw, "_dp_layers.0.weight"), (db, "_dp_layers.0.bias")]
    if norm:
        pairs += [(dg, "_dp_layers.1.weight"), (dbt, "_dp_layers.1.bias")]
    if norm == "bn":
        pairs += [(running[0], "_buf_layers.1.running_mean"), (running[1], "_buf_layers.1.running_var")]
    for got, key in pairs:
        ref = g[name + key]
        # (the conv bias in front of a norm has a mathematically zero gradient: both sides hold rounding noise of ~1e-5 there)
        tol = 3e-5 if (norm and key == "_dp_layers.0.bias") else 3e-6
        assert np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), (name, key, np.abs(got - ref).max())


# ------------------------------------------------------------------ F15: depth-wise ConvLayer / ReLU6
F15_LAYERS = [("dw_k3", dict(in_ch=16, out_ch=16, ksize=3, groups=16, bias=False, act=None), (2, 16, 9, 11)),
              ("dw_k1", dict(in_ch=24, out_ch=24, ksize=1, groups=24, bias=False, act=None), (1, 24, 5, 6)),
              ("dw_k3_bias", dict(in_ch=8, out_ch=8, ksize=3, groups=8, act=None), (2, 8, 2, 7)),
              ("relu6_k1", dict(in_ch=16, out_ch=64, ksize=1, bias=False, act="relu6"), (2, 16, 6, 7))]


@pytest.mark.parametrize("case", F15_LAYERS, ids=[c[0] for c in F15_LAYERS])
def test_f15_depthwise_and_relu6_oracle_vs_reference(case):
    name, kw, shape = case
    g = np.load(os.path.join(G, "f15_n4_res2.npz"))
    cin, cout, k = kw["in_ch"], kw["out_ch"], kw["ksize"]
    has_bias = kw.get("bias", True)
    dw = kw.get("groups", 1) > 1
    w = O.closed_form_param(0, "layers.0.weight", (cout, 1 if dw else cin, k, k), 15)
    b = O.closed_form_param(1, "layers.0.bias", (cout,), 15) if has_bias else None
    x = O.closed_form_signed(shape, 0.5, 8.0 if name == "relu6_k1" else 1.0)
    if dw:
        y = O.dwconv_fwd(x, w, b, True)
        gy = O.closed_form_signed(y.shape, 1.5, 1.0)
        dx, gw, gb = O.dwconv_bwd(x, w, gy, True)
    else:
        z = O.conv2d_general_fwd(x, w, b, 1, 0, False, False)
        y = O._act(z, kw["act"])
        gy = O.closed_form_signed(y.shape, 1.5, 1.0)
        dx, gw, gb = O.conv2d_general_bwd(x, w, z, gy * O._act_dydz(y, kw["act"]), 1, 0, False, False)
        assert float((y == 6).mean()) > 0.01 and float((y == 0).mean()) > 0.01   # both ReLU6 bounds are exercised
    pairs = [(y, "_y"), (dx, "_dx"), (gw, "_dp_layers.0.weight")] + ([(gb, "_dp_layers.0.bias")] if has_bias else [])
    for got, key in pairs:
        ref = g[name + key]
        assert np.abs(got - ref).max() <= 3e-6 * max(1.0, np.abs(ref).max()), (name, key, np.abs(got - ref).max())
