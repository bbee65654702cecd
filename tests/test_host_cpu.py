"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/mmif.h
declares, the Python mirror reproduces the reference's module tree / state_dict layout and error
behaviour, and the training plumbing (meters, warm-up, flags) behaves like the reference's common.py."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_library_exports_every_declared_symbol():
    import mmif
    from mmif._lib import LIB_PATH, SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mmif.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mmif_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 25
    lib = ctypes.CDLL(LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/mmif.h but not exported by {LIB_PATH}"
        assert name in SIGNATURES, f"{name} has no ctypes prototype in mmif/_lib.py"
    assert "gfx950" in mmif.version()


def test_c_abi_argument_validation_without_gpu():
    """Validation runs before any launch, so error paths are testable on CPU."""
    from mmif._lib import MmifTensor, lib
    t = MmifTensor(None, 0, 1, 8, 8, 0, 1, 0, 1, 0)
    assert lib.mmif_zero(ctypes.byref(t), None) == -1
    assert b"null tensor" in lib.mmif_last_error()
    buf = (ctypes.c_float * 64)()
    t = MmifTensor(ctypes.addressof(buf), 0, 1, 8, 8, 0, 1, 0, 2, 0)   # view wider than the allocation
    assert lib.mmif_zero(ctypes.byref(t), None) == -1
    assert lib.mmif_packed_weight_bytes(128, 128, 3) == 9 * 16 * 128 * 16
    assert lib.mmif_conv2d_wgrad_workspace(128, 128, 3) > 0 and lib.mmif_loss_workspace(2, 64, 64) > 0


def test_c_abi_validation_of_the_widened_entry_points_without_gpu():
    """pair conv / SSIM modes / TV / patch feed: bad arguments are rejected before anything is launched (no GPU needed),
    with the reference's messages where it has one."""
    from mmif._lib import MmifTensor, lib
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    ok = MmifTensor(base, 1, 1, 4, 4, 0, 1, 0, 1, 0)            # bf16 [1][1 block][4][4][8] = 256 B
    h1 = MmifTensor(base, 1, 1, 4, 4, 1, 1, 0, 1, 0)            # halo-1 view, NOT folded
    w = (ctypes.c_float * 36)()
    r = ctypes.byref
    assert lib.mmif_pairconv_fwd(r(ok), r(ok), w, None, 3, r(ok), r(ok), 1, None, None, None) == -1
    assert b"nout must be 1 or 2" in lib.mmif_last_error()
    assert lib.mmif_pairconv_fwd(r(ok), r(ok), None, None, 2, r(ok), r(ok), 1, None, None, None) == -1
    assert lib.mmif_pairconv_dgrad(r(h1), None, w, 1, None, None, r(h1), r(h1), 0, None, None) == -1
    assert b"folded first" in lib.mmif_last_error()
    assert lib.mmif_pairconv_wgrad(r(ok), r(ok), r(ok), None, 1, w, w, 0, None, 0, None) == -3            # workspace
    assert lib.mmif_pairconv_wgrad_workspace() > 0
    assert lib.mmif_pairconv_bwd(r(ok), None, w, 1, r(ok), r(ok), r(h1), r(h1), 0, None, w, w, 0, None, 0, None) == -3   # workspace
    assert lib.mmif_pairconv_bwd(r(ok), None, w, 2, r(ok), r(ok), r(h1), r(h1), 0, None, w, w, 0, None, 0, None) == -1   # gb missing
    # ---- the pair-conv family's edge shapes and gradient states (tests/pair_cases.py defines everything these calls accept)
    big = (ctypes.c_char * (1 << 20))()
    ws, nws = ctypes.addressof(big), 1 << 20

    def t(h, wd, halo=0, flags=0, cb=1, dtype=1):
        return MmifTensor(base, dtype, 1, h, wd, halo, cb, 0, cb, flags)
    for h, wd in ((1, 4), (4, 1), (1, 1)):      # reflect padding by 1 has no source below 2 x 2: all four refuse, with and without a mask
        x, g, gx = t(h, wd), t(h, wd), t(h, wd, 1)
        calls = [lambda: lib.mmif_pairconv_fwd(r(x), r(x), w, None, 1, r(x), None, 1, None, None, None),
                 lambda: lib.mmif_pairconv_dgrad(r(g), None, w, 1, r(x), r(x), r(gx), r(gx), 1, None, None),
                 lambda: lib.mmif_pairconv_dgrad(r(g), None, w, 1, None, None, r(gx), r(gx), 0, None, None),
                 lambda: lib.mmif_pairconv_wgrad(r(x), r(x), r(g), None, 1, w, w, 0, ws, nws, None),
                 lambda: lib.mmif_pairconv_bwd(r(g), None, w, 1, r(x), r(x), r(gx), r(gx), 0, None, w, w, 0, ws, nws, None)]
        for call in calls:
            assert call() == -1
            assert b"reflect padding needs h, w >= 2" in lib.mmif_last_error()
    g4, gx4, f4 = t(4, 4), t(4, 4, 1), t(4, 4, 1, 1)
    # `add`: shape and dtype must be g's in both calls; an unfolded halo-1 add is mmif_pairconv_dgrad's to fold, mmif_pairconv_bwd refuses it
    for bad in (t(4, 5), t(5, 4), t(4, 4, cb=2), t(4, 4, dtype=0), t(4, 5, 1), t(4, 4, 1, 1, dtype=0)):
        assert lib.mmif_pairconv_dgrad(r(g4), None, w, 1, None, None, r(gx4), r(gx4), 0, r(bad), None) == -1
        assert b"pairconv_dgrad: add shape mismatch" in lib.mmif_last_error()
        assert lib.mmif_pairconv_bwd(r(g4), None, w, 1, r(g4), r(g4), r(gx4), r(gx4), 0, r(bad), w, w, 0, ws, nws, None) == -1
        assert b"pairconv_bwd: add shape mismatch" in lib.mmif_last_error()
    assert lib.mmif_pairconv_bwd(r(g4), None, w, 1, r(g4), r(g4), r(gx4), r(gx4), 0, r(gx4), w, w, 0, ws, nws, None) == -1
    assert b"pairconv_bwd: a halo-1 residual gradient must be folded first" in lib.mmif_last_error()
    assert lib.mmif_pairconv_bwd(r(gx4), None, w, 1, r(g4), r(g4), r(gx4), r(gx4), 0, None, w, w, 0, ws, nws, None) == -1
    assert b"pairconv_bwd: a halo-1 gradient must be folded first" in lib.mmif_last_error()
    assert lib.mmif_pairconv_bwd(r(g4), r(f4), w, 2, r(g4), r(g4), r(gx4), r(gx4), 0, None, w, w, 0, ws, nws, None) == -1
    assert b"ga and gb must have the same halo" in lib.mmif_last_error()
    # activations are halo 0 everywhere; gx is halo 1
    assert lib.mmif_pairconv_wgrad(r(f4), r(f4), r(g4), None, 1, w, w, 0, ws, nws, None) == -1
    assert lib.mmif_pairconv_dgrad(r(g4), None, w, 1, r(f4), r(f4), r(gx4), r(gx4), 1, None, None) == -1
    assert b"xa/xb shape mismatch" in lib.mmif_last_error()
    assert lib.mmif_pairconv_dgrad(r(g4), None, w, 1, None, None, r(g4), r(g4), 0, None, None) == -1
    assert b"gx must be halo-1 views" in lib.mmif_last_error()
    f = (ctypes.c_float * 16)()
    assert lib.mmif_ssim_loss_mode(f, f, f, 1, 32, 32, 1.0, 1.0, 7, f, None, f, 1 << 20, None) == -1
    assert b"only supported ['ssim', 'w-ssim', 'ms-ssim', 'msw-ssim'] mode" in lib.mmif_last_error()
    assert lib.mmif_ssim_loss_mode(f, f, f, 1, 8, 8, 1.0, 1.0, 1, f, None, f, 1 << 20, None) == -1        # < 11x11
    assert lib.mmif_ssim_loss_mode(f, f, f, 1, 32, 32, 1.0, 1.0, 1, f, None, f, 16, None) == -3
    assert lib.mmif_ssim_loss_mode_workspace(2, 256, 256, 2) > lib.mmif_ssim_loss_mode_workspace(2, 256, 256, 1) > 0
    assert lib.mmif_tv_loss(f, 1, 1, 8, 1.0, 0, f, None, f, 1 << 16, None) == -1                          # needs 2x2
    assert lib.mmif_tv_loss(f, 1, 8, 8, 1.0, 0, f, None, f, 16, None) == -3
    assert lib.mmif_patch_feed(f, 4, 8, f, None, 2, 5, f, None) == -1
    assert b"only supported ['min-max', 'z-score'] mode" in lib.mmif_last_error()
    assert lib.mmif_patch_feed(None, 4, 8, f, None, 2, 0, f, None) == -1
    assert lib.mmif_fuse_attn_workspace(2, 64) > 0
    assert lib.mmif_gconv_fwd(f, f, None, f, 1, 8, 8, 16, 16, 4, 1, 2, 1, 0, None) == -1
    assert b"ksize must be 1, 3, 5 or 7" in lib.mmif_last_error()
    assert lib.mmif_gconv_fwd(f, f, None, f, 1, 8, 8, 16, 16, 3, 3, 1, 1, 0, None) == -1
    assert b"stride must be 1 or 2" in lib.mmif_last_error()
    assert lib.mmif_gconv_fwd(f, f, None, f, 1, 8, 8, 3, 16, 7, 1, 3, 1, 0, None) == -1           # reflect 3 on a 3-row image
    assert lib.mmif_gconv_dgrad(f, f, f, 1, 8, 8, 16, 16, 5, 1, 2, 1, None, 0, None) == -3
    assert lib.mmif_gconv_dgrad_workspace(2, 8, 16, 16, 2, 1) == 2 * 8 * 20 * 20 * 4 and lib.mmif_gconv_dgrad_workspace(2, 8, 16, 16, 2, 0) == 0
    assert lib.mmif_gconv_wgrad(f, f, f, None, 1, 8, 8, 16, 16, 5, 1, 2, 1, f, 64, None) == -3
    assert lib.mmif_gconvt_fwd(f, f, None, f, 1, 8, 8, 4, 4, 3, 2, 1, 2, 0, None) == -1           # output_padding >= stride
    # depth-wise reflect padding by 1 has no source below 2 x 2: the forward and both gradients refuse it alike (k = 1 pads nothing)
    for h, wd in ((1, 4), (4, 1), (1, 1)):
        for call, what in ((lambda: lib.mmif_dwconv_fwd(f, f, None, f, 1, 1, h, wd, 3, 1, None), b"dwconv_fwd"),
                           (lambda: lib.mmif_dwconv_dgrad(f, f, f, 1, 1, h, wd, 3, 1, None), b"dwconv_dgrad"),
                           (lambda: lib.mmif_dwconv_wgrad(f, f, f, None, 1, 1, h, wd, 3, 1, None), b"dwconv_wgrad")):
            assert call() == -1
            assert what + b": reflect padding needs h,w >= 2" in lib.mmif_last_error()
    assert lib.mmif_dwconv_dgrad(f, f, f, 1, 1, 4, 4, 5, 1, None) == -1 and b"dwconv_dgrad: ksize must be 1 or 3" in lib.mmif_last_error()
    assert lib.mmif_dwconv_wgrad(f, f, f, None, 1, 1, 4, 4, 2, 0, None) == -1 and b"dwconv_wgrad: ksize must be 1 or 3" in lib.mmif_last_error()
    assert lib.mmif_relu_bwd(None, f, f, 4, None) == -1 and lib.mmif_channel_sum(f, f, 0, 1, 1, None) == -1
    assert lib.mmif_reflect_pad_fwd(f, f, 1, 4, 4, 4, 0, 0, 0, None) == -1      # padding must be smaller than the input
    assert lib.mmif_maxpool_nchw_fwd(f, f, f, 1, 3, 8, 4, None) == -1 and lib.mmif_nearest_up_fwd(f, f, 1, 2, 2, 0, None) == -1
    # each plane-wise resampler and its backward refuse the same geometries
    for fwd, bwd, bad in ((lambda *a: lib.mmif_bilinear_up_fwd(f, f, *a, None), lambda *a: lib.mmif_bilinear_up_bwd(f, f, *a, None),
                           ((1, 4, 4, 3, 4), (1, 4, 4, 4, 3), (0, 2, 2, 2, 2), (1, 0, 2, 2, 2))),
                          (lambda *a: lib.mmif_maxpool_nchw_fwd(f, f, f, *a, None), lambda *a: lib.mmif_maxpool_nchw_bwd(f, f, f, *a, None),
                           ((1, 3, 8, 4), (1, 8, 3, 4), (1, 16, 16, 16), (1, 4, 4, 0), (0, 4, 4, 2))),
                          (lambda *a: lib.mmif_nearest_up_fwd(f, f, *a, None), lambda *a: lib.mmif_nearest_up_bwd(f, f, *a, None),
                           ((1, 2, 2, 0), (0, 2, 2, 2), (1, 0, 2, 2))),
                          (lambda *a: lib.mmif_reflect_pad_fwd(f, f, *a, None), lambda *a: lib.mmif_reflect_pad_bwd(f, f, *a, None),
                           ((1, 4, 4, 4, 0, 0, 0), (1, 4, 4, 0, 0, 0, 4), (1, 4, 4, -2, -2, 0, 0), (1, 4, 4, 0, 0, -4, 0), (0, 4, 4, 1, 1, 1, 1)))):
        for a in bad:
            assert fwd(*a) == -1 and bwd(*a) == -1, a
    from mmif._lib import MmifPackJob
    jobs = (MmifPackJob * 1)()
    assert lib.mmif_pack_weights_multi(jobs, 0, None) == -1
    jobs[0].w, jobs[0].cout, jobs[0].cin, jobs[0].ksize = base, 16, 16, 5
    assert lib.mmif_pack_weights_multi(jobs, 1, None) == -1
    assert b"ksize must be 1 or 3" in lib.mmif_last_error()


def test_c_abi_validation_of_the_blocked_glue_entry_points_without_gpu():
    """csrc/nest.hip and the element-fusion / layout kernels of csrc/misc.hip (tests/nest_cases.py defines everything these calls accept): every
    shape, halo, dtype, mode and workspace refusal comes before any launch"""
    from mmif._lib import MmifTensor, lib
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    r = ctypes.byref
    err = lib.mmif_last_error

    def t(h, wd, halo=0, flags=0, cb=1, dtype=1, n=1):
        return MmifTensor(base, dtype, n, h, wd, halo, cb, 0, cb, flags)
    # ---- nearest x2 + reflect pad: the target is at least 2x the source and less than 4x (one reflection), forward and both backwards
    x2 = t(2, 2)
    for H, W in ((8, 4), (4, 8), (9, 5), (8, 8), (3, 4), (4, 3)):
        assert lib.mmif_upsample2x_fwd(r(x2), r(t(H, W)), None) == -1
        assert b"upsample2x_fwd: target shape" in err()
        for g in (t(H, W), t(H, W, 1), t(H, W, 1, 1)):
            assert lib.mmif_upsample2x_bwd(r(g), r(t(2, 2, 1)), 0, None) == -1
            assert b"upsample2x_bwd: shape mismatch" in err()
            assert lib.mmif_upsample2x_bwd_relu(r(g), r(t(2, 2, 1)), 1, r(x2), None) == -1
            assert b"upsample2x_bwd: shape mismatch" in err()
    assert lib.mmif_upsample2x_fwd(r(t(2, 2, 1)), r(t(4, 4)), None) == -1 and lib.mmif_upsample2x_fwd(r(x2), r(t(4, 4, 1)), None) == -1      # halo
    assert lib.mmif_upsample2x_fwd(r(x2), r(t(4, 4, cb=2)), None) == -1 and lib.mmif_upsample2x_fwd(r(x2), r(t(4, 4, dtype=0)), None) == -1
    assert lib.mmif_upsample2x_bwd(r(t(4, 4, n=2)), r(t(2, 2, 1)), 0, None) == -1 and lib.mmif_upsample2x_bwd(r(t(4, 4, dtype=0)), r(t(2, 2, 1)), 0, None) == -1
    assert lib.mmif_upsample2x_bwd_relu(r(t(4, 4)), r(t(2, 2, 1)), 0, None, None) == -1
    assert b"upsample2x_bwd_relu: x is NULL" in err()
    for bad in (t(2, 3), t(2, 2, 1), t(2, 2, cb=2), t(2, 2, dtype=0)):
        assert lib.mmif_upsample2x_bwd_relu(r(t(4, 4)), r(t(2, 2, 1)), 0, r(bad), None) == -1
        assert b"upsample2x_bwd_relu: x does not match gx" in err()
    # ---- 2x2 max-pool
    x5 = t(5, 4)
    for y in (t(3, 2), t(2, 3), t(2, 2, 1), t(2, 2, cb=2), t(2, 2, dtype=0)):
        assert lib.mmif_maxpool2x2_fwd(r(x5), r(y), None) == -1
        assert b"maxpool2x2_fwd: shape mismatch" in err()
    assert lib.mmif_maxpool2x2_fwd(r(t(5, 4, 1)), r(t(2, 2)), None) == -1
    assert lib.mmif_maxpool2x2_fwd(r(t(1, 4)), r(t(1, 2)), None) == -1          # a one-row image has no 2x2 window
    for fn in (lib.mmif_maxpool2x2_bwd, lib.mmif_maxpool2x2_bwd_relu):
        for x, g, gx in ((x5, t(3, 2), t(5, 4, 1)), (x5, t(2, 2), t(4, 4, 1)), (x5, t(2, 2), t(5, 5, 1)), (t(5, 4, 1), t(2, 2), t(5, 4, 1)),
                         (x5, t(2, 2, dtype=0), t(5, 4, 1)), (x5, t(2, 2), t(5, 4, 1, cb=2))):
            assert fn(r(x), r(g), r(gx), 0, None) == -1
            assert b"maxpool2x2_bwd: shape mismatch" in err()
        assert fn(r(x5), None, r(t(5, 4, 1)), 0, None) == -1
        assert b"null tensor" in err()
    # ---- in-place ReLU mask
    for x, g in ((t(4, 4), t(4, 5, 1)), (t(4, 4, 1), t(4, 4, 1)), (t(4, 4), t(4, 4, 1, cb=2)), (t(4, 4, dtype=0), t(4, 4))):
        assert lib.mmif_relu_mask(r(x), r(g), None) == -1
        assert b"relu_mask: shape mismatch" in err()
    # ---- attention fusion: mode, shapes, activations at halo 0, workspace
    a, g1 = t(4, 4), t(4, 4, 1)
    big = (ctypes.c_char * (1 << 16))()
    ws, nws = ctypes.addressof(big), 1 << 16
    assert lib.mmif_fuse_attn_workspace(1, 8) <= nws
    assert lib.mmif_fuse_attn_fwd(r(a), r(a), r(a), 3, ws, nws, None) == -1
    assert b"only supported ['sa', 'ca', 'sca', 'wavg'] mode" in err()
    for x, y, o in ((a, t(4, 5), a), (a, a, t(5, 4)), (g1, a, a), (a, a, g1), (a, t(4, 4, cb=2), a), (a, a, t(4, 4, dtype=0))):
        assert lib.mmif_fuse_attn_fwd(r(x), r(y), r(o), 2, ws, nws, None) == -1
        assert b"fuse_attn_fwd: shape mismatch" in err()
    assert lib.mmif_fuse_attn_fwd(r(a), r(a), r(a), 2, ws, 16, None) == -3
    for fn in (lib.mmif_fuse_attn_bwd, lib.mmif_fuse_attn_bwd_cached):
        assert fn(r(a), r(a), r(g1), r(g1), r(g1), -1, 0, ws, nws, None) == -1
        assert b"only supported ['sa', 'ca', 'sca', 'wavg'] mode" in err()
        for x, y, g, ga, gb in ((g1, a, g1, g1, g1), (a, g1, g1, g1, g1), (a, a, t(4, 5, 1), g1, g1), (a, a, g1, t(5, 4, 1), g1), (a, a, g1, g1, t(4, 5, 1)),
                                (a, a, g1, t(4, 4, 1, cb=2), g1), (a, a, t(4, 4, 1, dtype=0), g1, g1)):
            assert fn(r(x), r(y), r(g), r(ga), r(gb), 0, 0, ws, nws, None) == -1
            assert b"fuse_attn_bwd: shape mismatch" in err()
        assert fn(r(a), r(a), r(g1), r(g1), r(g1), 1, 0, ws, 16, None) == -3
        assert fn(r(a), r(a), r(g1), None, r(g1), 1, 0, ws, nws, None) == -1
    # ---- element fusion: a / b are only looked at when the mode or the mask needs them
    assert lib.mmif_fuse_elem_fwd(r(a), r(a), r(a), 3, None) == -1
    assert b"only supported ['sum', 'mean', 'max'] mode" in err()
    for x, y, o in ((a, g1, a), (g1, g1, g1), (a, a, g1), (a, t(4, 5), a), (a, a, t(4, 4, dtype=0))):
        assert lib.mmif_fuse_elem_fwd(r(x), r(y), r(o), 0, None) == -1
        assert b"fuse_elem_fwd: shape/halo mismatch" in err()
    assert lib.mmif_fuse_elem_bwd(None, None, r(g1), r(g1), r(g1), -1, 0, None) == -1
    assert b"only supported ['sum', 'mean', 'max'] mode" in err()
    for g, ga, gb in ((g1, a, g1), (g1, g1, a), (a, g1, g1), (g1, t(4, 5, 1), g1), (g1, g1, t(4, 4, 1, cb=2))):
        assert lib.mmif_fuse_elem_bwd(None, None, r(g), r(ga), r(gb), 0, 0, None) == -1
        assert b"fuse_elem_bwd: gradient shape/halo mismatch" in err()
    for mode, mask in ((2, 0), (0, 1), (1, 1)):
        assert lib.mmif_fuse_elem_bwd(None, r(a), r(g1), r(g1), r(g1), mode, mask, None) == -1
        assert b"null tensor" in err()
        for x, y in ((g1, a), (a, g1), (t(4, 5), a), (a, t(4, 4, dtype=0))):
            assert lib.mmif_fuse_elem_bwd(r(x), r(y), r(g1), r(g1), r(g1), mode, mask, None) == -1
            assert b"fuse_elem_bwd: a/b mismatch" in err()
    # ---- layout conversions: the logical channel count fits the view
    f = (ctypes.c_float * 16)()
    for c in (0, -1, 9):
        assert lib.mmif_nchw_to_blocked(f, c, r(a), None) == -1
        assert b"nchw_to_blocked: c=" in err()
        assert lib.mmif_blocked_to_nchw(r(a), f, c, None) == -1
        assert b"blocked_to_nchw: c=" in err()
    assert lib.mmif_nchw_to_blocked(f, 8, None, None) == -1 and lib.mmif_blocked_to_nchw(None, f, 8, None) == -1


def test_c_abi_validation_of_the_image_layer_entry_points_without_gpu():
    """csrc/conv_image.hip and csrc/image_bwd.hip (tests/image_cases.py defines everything these calls accept): every refusal comes before any
    launch.  The two weight gradients refuse a view whose channel blocks do not match the channels' 16-channel groups -- their kernels lay the
    partial sums out by the grid's channel blocks, the reduce and the workspace by the channels."""
    from mmif._lib import MmifTensor, lib
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    big = (ctypes.c_char * (1 << 20))()
    ws, nws = ctypes.addressof(big), 1 << 20
    f = (ctypes.c_float * 1024)()
    r, err = ctypes.byref, lib.mmif_last_error

    def t(h=8, w=8, halo=0, cb=2, dtype=1, flags=0):
        return MmifTensor(base, dtype, 1, h, w, halo, cb, 0, cb, flags)
    a, g1 = t(), t(halo=1)
    for dtype in (0, 1):
        assert lib.mmif_conv2d_image_wgrad_workspace(16, 3) <= nws
        # ---- the weight gradients: channels against the view's blocks (a 16-channel call on a 3-block view would write partials past the workspace)
        for c, cb in ((0, 2), (-8, 2), (17, 2), (33, 4), (24, 2), (40, 4), (64, 7), (8, 3), (16, 3), (16, 4)):
            x = t(cb=cb, dtype=dtype)
            assert lib.mmif_conv2d_image_in_wgrad(f, r(x), f, f, c, 3, 0, ws, nws, None) == -1, (c, cb)
            assert b"image_in_wgrad: " in err(), err()
            assert lib.mmif_conv2d_image_out_wgrad(r(x), f, None, f, f, c, 3, 0, ws, nws, None) == -1, (c, cb)
            assert b"image_out_wgrad: " in err(), err()
        assert b"16-channel groups" in err()
        # ---- ksize
        x, gx = t(dtype=dtype), t(halo=1, dtype=dtype)
        for k in (0, 2, 5):
            calls = [lib.mmif_conv2d_image_in_fwd(f, f, None, r(x), 16, k, 0, None),
                     lib.mmif_conv2d_image_in_wgrad(f, r(x), f, f, 16, k, 0, ws, nws, None),
                     lib.mmif_conv2d_image_out_fwd(r(x), f, None, f, 16, k, 0, None),
                     lib.mmif_conv2d_image_out_dgrad(f, None, f, None, r(gx), 16, k, 0, 0, None),
                     lib.mmif_conv2d_image_out_wgrad(r(x), f, None, f, f, 16, k, 0, ws, nws, None),
                     lib.mmif_conv2d_image_out_bwd(r(x), f, None, f, r(gx), f, f, 16, k, 0, ws, nws, None)]
            assert calls == [-1] * 6, (k, calls)
            assert lib.mmif_conv2d_image_out_bwd_supported(dtype, 16, k, 8, 8) == 0
        assert lib.mmif_conv2d_image_in_fwd(f, f, None, r(x), 16, 5, 0, None) == -1 and b"image_in_fwd: ksize must be 1 or 3" in err()
        # ---- activations are halo 0; gx needs halo >= k / 2; masks need x
        h1 = t(halo=1, dtype=dtype)
        assert lib.mmif_conv2d_image_in_fwd(f, f, None, r(h1), 16, 3, 0, None) == -1 and b"image_in_fwd: bad output view" in err()
        assert lib.mmif_conv2d_image_out_fwd(r(h1), f, None, f, 16, 3, 0, None) == -1 and b"image_out_fwd: bad input view" in err()
        assert lib.mmif_conv2d_image_out_wgrad(r(h1), f, None, f, f, 16, 3, 0, ws, nws, None) == -1 and b"image_out_wgrad: x must be an activation" in err()
        assert lib.mmif_conv2d_image_out_bwd(r(h1), f, None, f, r(gx), f, f, 16, 3, 0, ws, nws, None) == -1
        assert lib.mmif_conv2d_image_out_bwd(r(x), f, None, f, r(x), f, f, 16, 3, 0, ws, nws, None) == -1        # gx without a halo
        assert lib.mmif_conv2d_image_out_dgrad(f, None, f, None, r(x), 16, 3, 0, 0, None) == -1 and b"gx needs halo >= ksize/2" in err()
        assert lib.mmif_conv2d_image_out_dgrad(f, None, f, None, r(gx), 16, 3, 1, 0, None) == -1 and b"mask_bits set but x is NULL" in err()
        assert lib.mmif_conv2d_image_out_dgrad(f, None, f, r(h1), r(gx), 16, 3, 1, 0, None) == -1 and b"x / gx mismatch" in err()
        assert lib.mmif_conv2d_image_out_dgrad(f, None, f, None, r(gx), 17, 3, 0, 0, None) == -1 and b"gx view too small" in err()
        for c in (0, 17):
            assert lib.mmif_conv2d_image_in_fwd(f, f, None, r(x), c, 3, 0, None) == -1 and lib.mmif_conv2d_image_out_fwd(r(x), f, None, f, c, 3, 0, None) == -1
        # ---- reflect padding by 1 has no source below 2 x 2: all seven refuse at k = 3
        for h, w in ((1, 8), (8, 1), (1, 1)):
            x, gx = t(h, w, dtype=dtype), t(h, w, halo=1, dtype=dtype)
            calls = [lib.mmif_conv2d_image_in_fwd(f, f, None, r(x), 16, 3, 0, None),
                     lib.mmif_conv2d_image_in_wgrad(f, r(x), f, f, 16, 3, 0, ws, nws, None),
                     lib.mmif_conv2d_image_out_fwd(r(x), f, None, f, 16, 3, 0, None),
                     lib.mmif_conv2d_image_out_dgrad(f, None, f, None, r(gx), 16, 3, 0, 0, None),
                     lib.mmif_conv2d_image_out_wgrad(r(x), f, None, f, f, 16, 3, 0, ws, nws, None),
                     lib.mmif_conv2d_image_out_bwd(r(x), f, None, f, r(gx), f, f, 16, 3, 0, ws, nws, None)]
            assert calls == [-1] * 6, (h, w, calls)
            assert lib.mmif_conv2d_image_out_bwd_supported(dtype, 16, 3, h, w) == 0
        assert lib.mmif_conv2d_image_out_wgrad(r(t(1, 8, dtype=dtype)), f, None, f, f, 16, 3, 0, ws, nws, None) == -1 and b"reflect padding needs h,w >= 2" in err()
        # ---- a short workspace
        x = t(dtype=dtype)
        assert lib.mmif_conv2d_image_in_wgrad(f, r(x), f, f, 16, 3, 0, ws, 64, None) == -3 and b"image_in_wgrad: workspace too small" in err()
        assert lib.mmif_conv2d_image_out_wgrad(r(x), f, None, f, f, 16, 3, 0, ws, 64, None) == -3 and b"image_out_wgrad: workspace too small" in err()
        assert lib.mmif_conv2d_image_in_wgrad(f, r(x), f, f, 16, 1, 0, None, 0, None) == -3
    assert lib.mmif_conv2d_image_out_bwd(r(a), f, None, f, r(g1), f, f, 16, 3, 0, ws, 64, None) == -3 and b"image_out_bwd: workspace too small" in err()
    # ---- the fused backward: bf16, 16 channels, 3x3, h, w >= 4
    assert lib.mmif_conv2d_image_out_bwd_supported(1, 16, 3, 4, 4) == 1 and lib.mmif_conv2d_image_out_bwd_supported(1, 16, 3, 256, 256) == 1
    for args in ((0, 16, 3, 8, 8), (1, 8, 3, 8, 8), (1, 24, 3, 8, 8), (1, 16, 1, 8, 8), (1, 16, 3, 3, 8), (1, 16, 3, 8, 3)):
        assert lib.mmif_conv2d_image_out_bwd_supported(*args) == 0, args
    assert lib.mmif_conv2d_image_out_bwd(r(t(dtype=0)), f, None, f, r(t(halo=1, dtype=0)), f, f, 16, 3, 0, ws, nws, None) == -1 and b"image_out_bwd: bf16" in err()
    assert lib.mmif_conv2d_image_out_bwd(r(t(3, 8)), f, None, f, r(t(3, 8, halo=1)), f, f, 16, 3, 0, ws, nws, None) == -1
    assert lib.mmif_conv2d_image_out_bwd(r(t(cb=3)), f, None, f, r(t(halo=1, cb=3)), f, f, 16, 3, 0, ws, nws, None) == -1
    assert lib.mmif_conv2d_image_out_bwd(r(a), f, None, f, r(t(8, 9, halo=1)), f, f, 16, 3, 0, ws, nws, None) == -1


def test_c_abi_validation_of_the_norm_and_optimiser_entry_points_without_gpu():
    """csrc/norm.hip's nine entry points and mmif_clip_adam_step (tests/norm_cases.py and tests/optim_cases.py define everything these calls
    accept): every refusal comes before any launch, with its return code and message.  None of these calls may ever reach a device."""
    from mmif._lib import lib
    err = lib.mmif_last_error
    fbuf = (ctypes.c_float * 4096)()
    f = ctypes.addressof(fbuf)
    big = (ctypes.c_char * (1 << 16))()
    ws, nws = ctypes.addressof(big), 1 << 16
    n, c, hw = 2, 3, 5
    need = lib.mmif_norm_workspace(n, c)
    assert need == (n * c + c) * 2 * 8 and lib.mmif_norm_workspace(3, 257) == (3 * 257 + 257) * 16 and lib.mmif_norm_workspace(1, 1) == 32
    assert lib.mmif_clip_adam_workspace(1) == lib.mmif_clip_adam_workspace(3 * 262144 + 17) == (1024 + 8) * 4

    def refused(call, msg, code=-1):
        assert call() == code, msg
        assert msg in err(), (msg, err())

    # ---- mmif_norm_act_fwd(x, gamma, beta, y, stats, running_mean, running_var, n, c, hw, kind, eps, momentum, act, slope, ws, bytes, stream)
    def fwd(x=f, y=f, stats=f, rm=None, rv=None, n=n, c=c, hw=hw, kind=0, act=1, ws=ws, nws=nws):
        return lambda: lib.mmif_norm_act_fwd(x, f, f, y, stats, rm, rv, n, c, hw, kind, 1e-5, 0.1, act, 0.2, ws, nws, None)
    for kw in (dict(x=None), dict(y=None), dict(stats=None), dict(n=0), dict(c=0), dict(hw=0), dict(n=-1)):
        refused(fwd(**kw), b"norm_act_fwd: bad arguments")
    for kw in (dict(kind=-1), dict(kind=3), dict(act=-1), dict(act=5)):
        refused(fwd(**kw), b"norm_act_fwd: bad kind / activation")
    for kw in (dict(kind=1), dict(kind=1, rm=f), dict(kind=1, rv=f)):
        refused(fwd(**kw), b"norm_act_fwd: eval mode needs the running statistics")
    for kw in (dict(rm=f), dict(rv=f)):          # kind 0 updates both buffers or none: a lone one would be a write through NULL
        refused(fwd(**kw), b"norm_act_fwd: running_mean and running_var come together")
    for kind in (0, 2):
        for kw in (dict(ws=None), dict(nws=need - 1), dict(nws=0)):
            refused(fwd(kind=kind, **kw), b"norm_act_fwd: workspace too small", -3)
    # ---- mmif_norm_act_bwd(x, y, gy, stats, gamma, dx, dgamma, dbeta, n, c, hw, kind, act, slope, ws, bytes, stream)
    def bwd(x=f, y=f, gy=f, stats=f, dx=f, n=n, c=c, hw=hw, kind=0, act=1, ws=ws, nws=nws):
        return lambda: lib.mmif_norm_act_bwd(x, y, gy, stats, None, dx, None, None, n, c, hw, kind, act, 0.2, ws, nws, None)
    for kw in (dict(x=None), dict(y=None), dict(gy=None), dict(stats=None), dict(dx=None), dict(n=0), dict(c=0), dict(hw=0)):
        refused(bwd(**kw), b"norm_act_bwd: bad arguments")
    for kw in (dict(kind=-1), dict(kind=3), dict(act=-1), dict(act=5)):
        refused(bwd(**kw), b"norm_act_bwd: bad kind / activation")
    for kind in (0, 1, 2):
        for kw in (dict(ws=None), dict(nws=need - 1)):
            refused(bwd(kind=kind, **kw), b"norm_act_bwd: workspace too small", -3)
    # ---- mmif_bn_moments(x, chan_sums, n, c, hw, ws, bytes, stream)
    for a in ((None, f, n, c, hw), (f, None, n, c, hw), (f, f, 0, c, hw), (f, f, n, 0, hw), (f, f, n, c, 0)):
        refused(lambda: lib.mmif_bn_moments(*a, ws, nws, None), b"bn_moments: bad arguments")
    for w_, nb in ((None, nws), (ws, need - 1)):
        refused(lambda: lib.mmif_bn_moments(f, f, n, c, hw, w_, nb, None), b"bn_moments: workspace too small", -3)
    # ---- mmif_bn_apply_fwd(x, chan_sums, gamma, beta, y, stats, running_mean, running_var, n, c, hw, eps, momentum, act, slope, stream)
    def apply_fwd(x=f, chan=f, y=f, stats=f, rm=None, rv=None, n=n, c=c, hw=hw, act=1):
        return lambda: lib.mmif_bn_apply_fwd(x, chan, None, None, y, stats, rm, rv, n, c, hw, 1e-5, 0.1, act, 0.2, None)
    for kw in (dict(x=None), dict(chan=None), dict(y=None), dict(stats=None), dict(n=0), dict(c=0), dict(hw=0)):
        refused(apply_fwd(**kw), b"bn_apply_fwd: bad arguments")
    for act in (-1, 5):
        refused(apply_fwd(act=act), b"bn_apply_fwd: bad activation")
    for kw in (dict(rm=f), dict(rv=f)):
        refused(apply_fwd(**kw), b"bn_apply_fwd: running_mean and running_var come together")
    # ---- mmif_bn_bwd_sums(x, y, gy, stats, chan_sums, dgamma, dbeta, n, c, hw, act, slope, ws, bytes, stream)
    def bwd_sums(x=f, y=f, gy=f, stats=f, chan=f, n=n, c=c, hw=hw, act=1, ws=ws, nws=nws):
        return lambda: lib.mmif_bn_bwd_sums(x, y, gy, stats, chan, None, None, n, c, hw, act, 0.2, ws, nws, None)
    for kw in (dict(x=None), dict(y=None), dict(gy=None), dict(stats=None), dict(chan=None), dict(n=0), dict(c=0), dict(hw=0)):
        refused(bwd_sums(**kw), b"bn_bwd_sums: bad arguments")
    for act in (-1, 5):
        refused(bwd_sums(act=act), b"bn_bwd_sums: bad activation")
    for kw in (dict(ws=None), dict(nws=need - 1)):
        refused(bwd_sums(**kw), b"bn_bwd_sums: workspace too small", -3)
    # ---- mmif_bn_apply_bwd(x, y, gy, stats, gamma, chan_sums, count, dx, n, c, hw, act, slope, stream)
    def apply_bwd(x=f, y=f, gy=f, stats=f, chan=f, count=f, dx=f, n=n, c=c, hw=hw, act=1):
        return lambda: lib.mmif_bn_apply_bwd(x, y, gy, stats, None, chan, count, dx, n, c, hw, act, 0.2, None)
    for kw in (dict(x=None), dict(y=None), dict(gy=None), dict(stats=None), dict(chan=None), dict(count=None), dict(dx=None), dict(n=0), dict(c=0),
               dict(hw=0)):
        refused(apply_bwd(**kw), b"bn_apply_bwd: bad arguments")
    for act in (-1, 5):
        refused(apply_bwd(act=act), b"bn_apply_bwd: bad activation")
    # ---- mmif_act_fwd(x, y, count, act, slope, stream), mmif_act_bwd(gy, y, dx, count, act, slope, stream); count 0 is accepted and does nothing
    for a in ((None, f, 4, 1), (f, None, 4, 1), (f, f, -1, 1), (f, f, 4, -1), (f, f, 4, 5)):
        refused(lambda: lib.mmif_act_fwd(*a, 0.2, None), b"act_fwd: bad arguments")
    for a in ((None, f, f, 4, 1), (f, None, f, 4, 1), (f, f, None, 4, 1), (f, f, f, -1, 1), (f, f, f, 4, -1), (f, f, f, 4, 5)):
        refused(lambda: lib.mmif_act_bwd(*a, 0.2, None), b"act_bwd: bad arguments")
    assert lib.mmif_act_fwd(f, f, 0, 3, 0.2, None) == 0 and lib.mmif_act_bwd(f, f, f, 0, 3, 0.2, None) == 0
    # ---- mmif_clip_adam_step(params, grads, exp_avg, exp_avg_sq, numel, lr, b1, b2, eps, step, max_norm, grad_scale, norm_out, ws, bytes, stream)
    aneed = lib.mmif_clip_adam_workspace(16)

    def adam(p=f, g=f, m=f, v=f, numel=16, step=1, ws=ws, nws=nws):
        return lambda: lib.mmif_clip_adam_step(p, g, m, v, numel, 1e-4, 0.9, 0.999, 1e-8, step, 5.0, 1.0, None, ws, nws, None)
    refused(adam(numel=0), b"clip_adam_step: numel=0 step=1")
    refused(adam(numel=-3), b"clip_adam_step: numel=-3 step=1")
    refused(adam(step=0), b"clip_adam_step: numel=16 step=0")
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None)):
        refused(adam(**kw), b"clip_adam_step: params, grads, exp_avg and exp_avg_sq must not be NULL")
    for kw in (dict(nws=aneed - 1), dict(nws=0), dict(ws=None, nws=0)):
        refused(adam(**kw), b"clip_adam_step: workspace too small", -3)
    refused(adam(ws=None), b"clip_adam_step: workspace is NULL")          # enough bytes claimed, no buffer behind them


@pytest.mark.parametrize("name", ["PFNetv1", "PFNetv2", "DenseFuse", "VIFNet", "NestFuse", "RFNNest", "DeepFuse", "DBNet", "SEDRFuse", "IFCNN",
                                  "DIFNet", "PMGI", "UNFusion", "MAFusion", "Res2Fusion"])
def test_state_dict_manifest_and_init(name):
    import core.model as M
    man = json.load(open(os.path.join(G, {"VIFNet": "f10_manifest.json", "DeepFuse": "f12_manifest.json", "DBNet": "f12_manifest.json",
                                          "SEDRFuse": "f13_manifest.json", "IFCNN": "f13_manifest.json", "DIFNet": "f13_manifest.json",
                                          "PMGI": "f13_manifest.json", "UNFusion": "f14_manifest.json", "MAFusion": "f14_manifest.json", "Res2Fusion": "f15_manifest.json"}.get(name, "f5_manifest.json"))))
    torch.manual_seed(0)
    m = getattr(M, name)()
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == man[name]
    # reference init (core/block.py:101-118): zero biases; kaiming-normal weights for ReLU layers
    for k, v in m.state_dict().items():
        if k.endswith("bias"):
            assert float(v.abs().max()) == 0.0
    if name in ("NestFuse", "RFNNest", "DeepFuse", "SEDRFuse", "IFCNN", "DIFNet", "PMGI", "UNFusion", "MAFusion", "Res2Fusion"):
        return
    w = m.state_dict()["decode.0.layers.0.weight"]
    fan_in = w.shape[1] * 9
    assert abs(float(w.std()) - (2.0 / fan_in) ** 0.5) / (2.0 / fan_in) ** 0.5 < 0.05


def test_reference_init_is_bitwise_reproduced_when_reference_is_present():
    """The mirror's PFNetv1 init after torch.manual_seed(0) is the reference's bit for bit: same keys in the same order, same shapes and
    dtypes, and the sha256 of every tensor's bytes equal to the reference's (golden F17, recorded by tests/golden/make_golden.py)."""
    import hashlib
    import core.model as M
    ref = json.load(open(os.path.join(G, "f17_reference_init.json")))
    assert ref["model"] == "PFNetv1" and ref["seed"] == 0
    torch.manual_seed(0)
    mine = M.PFNetv1().state_dict()
    assert list(mine) == [k for k, _, _, _ in ref["tensors"]]
    for k, shape, dtype, digest in ref["tensors"]:
        v = mine[k]
        assert list(v.shape) == shape and str(v.dtype) == dtype, k
        assert hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() == digest, k


def test_conv_layer_signature_and_fallback_rules():
    from core.block import ConvBlock, ConvLayer, DenseBlock, NestDecoder, RFN
    assert ConvLayer(16, 16)._hip and ConvLayer(8, 64, ksize=1)._hip and ConvLayer(16, 1, act=None)._hip
    # argument combinations outside the hot path stay stock torch modules
    # the general kernels (k 5/7, stride 2, zero padding, ConvTranspose2d) -- still HIP, fp32 NCHW
    for lay in (ConvLayer(16, 16, stride=2), ConvLayer(16, 16, ksize=5), ConvLayer(1, 16, ksize=7), ConvLayer(16, 16, padding_mode='zeros'),
                ConvLayer(16, 8, stride=2, layer=nn.ConvTranspose2d)):
        assert lay._gen and not lay._hip
    # BatchNorm / GroupNorm(c, c) and LeakyReLU / Tanh: HIP conv + the norm / activation epilogue kernels
    for lay in (ConvLayer(16, 16, norm=nn.BatchNorm2d), ConvLayer(16, 16, act=nn.Tanh), ConvLayer(16, 16, norm=nn.GroupNorm, stride=2),
                ConvLayer(3, 16, ksize=5, norm=nn.BatchNorm2d, act=nn.LeakyReLU)):
        assert lay._epilogue and not lay._hip and not lay._gen
    # everything else stays the stock torch modules
    assert ConvLayer(16, 16, groups=16, bias=False, act=None)._depthwise and ConvLayer(16, 64, ksize=1, bias=False, act=nn.ReLU6)._epilogue
    for lay in (ConvLayer(16, 16, dilation=2, padding=2), ConvLayer(16, 16, pre_norm=nn.BatchNorm2d), ConvLayer(16, 16, act=nn.Sigmoid),
                ConvLayer(16, 16, groups=2)):
        assert not lay._hip and not lay._gen and not lay._epilogue
    assert list(DenseBlock(16, 16).state_dict())[0] == "layers.0.layers.0.weight"
    assert sum(p.numel() for p in ConvBlock(16, 64).parameters()) == 16 * 8 * 9 + 8 + 8 * 64 + 64
    assert len(list(RFN(16).parameters())) == 12
    assert "DB1_3.layers.1.layers.0.bias" in NestDecoder(ConvBlock, [8, 16, 24, 32], "nearest").state_dict()


def test_errors_match_reference_behaviour():
    import core.fusion as F
    import core.loss as L
    import core.model as M
    x = torch.zeros(1, 8, 4, 4)
    with pytest.raises(ValueError, match="sum"):
        F.element_fusion(x, x, "nope")
    with pytest.raises(ValueError):
        F.attention_fusion(x, x, "nope")
    with pytest.raises(ValueError):
        F.spatial_pooling(x, "nope")
    with pytest.raises(ValueError):
        F.channel_pooling(x, "nope")
    with pytest.raises(ValueError):
        L.NormLoss("l3")(x)
    with pytest.raises(ValueError):
        M.DenseFuse().fusion(x, x, mode="nope")
    with pytest.raises(NotImplementedError):
        M._FusionModel().fusion(x, x)
    # no silent CPU fallback for the hot path
    with pytest.raises(RuntimeError, match="GPU"):
        M.DenseFuse()(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))
    with pytest.raises(RuntimeError, match="GPU"):
        F.element_fusion(x, x, "sum")


def test_fusion_function_compositions_on_cpu_match_oracle():
    """attention / pooling functions are tensor-level compositions (valid on any device)."""
    import core.fusion as F
    from oracle import fusion_oracle as O
    s = (2, 16, 6, 10)
    a, b = O.closed_form_signed(s, 0.15), O.closed_form_signed(s, 1.25)
    for mode in ("sa", "ca", "sca"):
        got = F.attention_fusion(torch.from_numpy(a), torch.from_numpy(b), mode).numpy()
        np.testing.assert_allclose(got, O.attention_fusion(a, b, mode), rtol=2e-5, atol=2e-6)
    z = torch.zeros(s)
    assert float(F.attention_fusion(z, z, "sca").abs().max()) == 0.0


def test_common_plumbing():
    import common as C
    m = C.AverageMeter()
    assert m.is_empty()
    m.update(2.0, 4)
    m.update(4.0, 4)
    assert m.avg == 3.0 and m.count == 8
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    sch = C.WarmupLR(opt, 0.001, 10)   # the reference's call form (train.py:323): (optimizer, warmup_factor, warmup_iters)
    lrs = []
    for _ in range(12):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    want = [0.001 + 0.999 * i / 10 for i in range(10)] + [1.0, 1.0]   # common.py:156-166 'linear'
    assert np.allclose(lrs, want, atol=1e-12) and lrs == sorted(lrs)
    opt2 = torch.optim.SGD([p], lr=2.0)
    C.WarmupLR(opt2, warmup_factor=0.25, warmup_iters=3, warmup_method="constant")
    assert opt2.param_groups[0]["lr"] == 0.5
    with pytest.raises(ValueError):
        C.WarmupLR(torch.optim.SGD([p], lr=1.0), 0.1, 3, "cosine")
    img = torch.tensor([[[-0.5, 0.0], [0.5, 1.5]]])
    assert C.denorm(img).tolist() == [[[0], [0]], [[127], [255]]]   # truncation, as data/transform.py:32-35
    assert C.save_result(img).tolist() == C.denorm(img).tolist()
    assert abs(float(C.norm(np.array([255.0]))[0]) - 1.0) < 1e-7
    import sys
    argv, sys.argv = sys.argv, ["train.py", "--data", "roadscene", "--bs", "8", "--model", "DenseFuse"]
    try:
        a = C.get_train_args()
    finally:
        sys.argv = argv
    assert a.data == "roadscene" and a.bs == 8 and a.lr == 1e-4 and a.epoch == 12 and a.clip_grad is True and a.model == "DenseFuse"
    argv, sys.argv = sys.argv, ["test.py"]
    try:
        t = C.get_test_args()
    finally:
        sys.argv = argv
    assert t.data == "roadscene" and t.ckpt == "2023-02-26_23-15" and t.use_gpu is True


def test_make_logger_layout(tmp_path):
    """common.py:200-210: <root>/../checkpoints/<time>/train.log, returns (log_dir, logger)"""
    import common as C
    root = tmp_path / "pkg"
    root.mkdir()
    log_dir, logger = C.make_logger(str(root))
    assert os.path.isfile(os.path.join(log_dir, "train.log"))
    assert os.path.normpath(os.path.dirname(log_dir)) == str(tmp_path / "checkpoints")
    logger.info("hello")
    for h in list(logger.handlers):
        h.flush()
        logger.removeHandler(h)
    assert "hello" in open(os.path.join(log_dir, "train.log")).read()


def test_bench_self_launch_refuses_a_smaller_box(monkeypatch):
    """bench.py --gpus N on a box with fewer GPUs must not report an N-GPU line: self_launch exits with the "refusing" message before it
    starts anything (this container has 0 GPUs); the rendezvous port comes from the kernel (bind to port 0), not from the pid."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = bench.parse()
    import torch
    if torch.cuda.device_count() >= 8:
        pytest.skip("this box really has 8 GPUs")
    with pytest.raises(SystemExit) as ei:
        bench.self_launch(args)
    assert "refusing" in str(ei.value) and "--gpus 8" in str(ei.value)
    with pytest.raises(SystemExit) as ei:       # the whole entry point takes that exit too
        bench.main()
    assert "refusing" in str(ei.value)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--one-device"])     # debugging aid: gloo only
    with pytest.raises(SystemExit) as ei:
        bench.main()
    assert "gloo" in str(ei.value)
    p1, p2 = bench.free_port(), bench.free_port()
    assert 1024 < p1 < 65536 and 1024 < p2 < 65536
    # SURVEY 8(d)'s ideal for the headline config: 1 / max(42.8 us, 45.8 us) = 21.8 k pairs/s
    assert abs(bench.ideal_pairs_per_s("PFNetv1", 256, 256, "bf16") - 21850) < 100


def test_bench_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    """bench.py's --dump-outputs writer: float32 files (float64 stays float64), at most 64 MB in all, and an array too large for what is
    left replaced by the same seeded sample of its elements on every call.  A plain run is the default; --full is opt-in."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    args = bench.parse()
    assert args.steps == 7 and args.full is False and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"
    big = torch.arange(17_000_000, dtype=torch.float32)
    arrays = {"big": big, "half": torch.full((5,), 1.5, dtype=torch.bfloat16), "dbl": torch.arange(3, dtype=torch.float64)}
    shapes = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ("a", "b")]
    assert shapes[0] == shapes[1] and shapes[0]["half"] == [5] and shapes[0]["dbl"] == [3] and 0 < shapes[0]["big"][0] < big.numel()
    for d in ("a", "b"):
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= bench.DUMP_LIMIT_BYTES == 64 * 10**6
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b) and np.all(np.diff(a) >= 0)     # the same sorted sample both times
    assert np.load(tmp_path / "a" / "half.npy").dtype == np.float32 and np.load(tmp_path / "a" / "dbl.npy").dtype == np.float64
    small = bench.dump_outputs(str(tmp_path / "c"), {"x": torch.arange(6.0).reshape(2, 3)})
    assert small == {"x": [2, 3]} and np.array_equal(np.load(tmp_path / "c" / "x.npy"), np.arange(6.0, dtype=np.float32).reshape(2, 3))
