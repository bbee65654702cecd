# -*- coding: utf-8 -*-
"""Feature-fusion functions -- API mirror of the reference's core/fusion.py:21-153.

element_fusion runs on the HIP element-fusion kernels (mmif_fuse_elem_{fwd,bwd}); inside the models
concat_fusion is zero-copy (channel-block views) and DenseFuse's 'sum' runs on blocked buffers.
attention_fusion 'sa' / 'ca' / 'sca' with the reference's default pooling (spatial 'l1', channel 'avg') runs on
the HIP attention kernels (mmif_fuse_attn_{fwd,bwd}).  With both poolings 'nl' (Res2Fusion) the whole layer is HIP: the spatial maps on the
streaming non-local kernels (mmif_nonlocal_spatial_{fwd,bwd}, no [B, H*W, H*W/64] energy tensor), the channel maps on
mmif_nonlocal_channel_{fwd,bwd} and the join of the four maps (both weighted_fusion calls, the clamp, the mean) on one launch per direction
(mmif_fuse_join_{fwd,bwd}); $MMIF_NONLOCAL=torch keeps the tensor-level composition for all of it as the cross-check.
Every other combination of the tensor-level poolings (spatial 'sum' / 'mean' / 'l1' / 'l2' / 'linf', channel 'avg' / 'max') in any of the four
modes -- 'wavg', UNFusion's default, among them -- and spatial_fusion / channel_fusion with softmax=False run on the fused kernels of
csrc/attn_fuse.hip (mmif_attn_fuse_{fwd,bwd}: a pooling pass and a join pass forward, a reduction pass and a gradient pass backward, on plain NCHW
fp32), as does SEDRFuse's strategy (softmax_l1_fusion).  $MMIF_ATTN_FUSE=torch keeps the tensor-level composition as the cross-check; the
composition also serves CPU tensors, other dtypes, 'nuclear', softmax=True and mixes of 'nl' with another mode.  One deliberate difference: the
composition's channel 'max' is amax, which splits the gradient of a tied maximum evenly; the kernels follow the reference's max_pool2d and give
it to the first position in row-major order.
"""
import os

import torch

from mmif import _lib
from mmif import engine as E
from mmif import tensor as T
from mmif.tensor import BT

__all__ = ['element_fusion', 'weighted_fusion', 'concat_fusion', 'attention_fusion', 'spatial_fusion', 'channel_fusion',
           'spatial_pooling', 'channel_pooling']

eps = 1e-7

_ELEM_MODES = {'sum': _lib.FUSE_SUM, 'mean': _lib.FUSE_MEAN, 'max': _lib.FUSE_MAX}


class _ElemFusionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mode):
        dtype = E.compute_dtype()
        ab, bb = BT.from_nchw(a.detach(), dtype), BT.from_nchw(b.detach(), dtype)
        ob = BT.alloc(ab.n, a.shape[1], ab.h, ab.w, dtype, a.device)
        T.fuse_elem_fwd(ab, bb, ob, mode)
        ctx.saved = (ab, bb, mode, a.shape[1])
        return ob.to_nchw(a.shape[1])

    @staticmethod
    def backward(ctx, g):
        ab, bb, mode, c = ctx.saved
        gb = BT.from_nchw(g.contiguous(), ab.dtype)
        ga = BT.alloc(ab.n, c, ab.h, ab.w, ab.dtype, g.device)
        gbb = BT.alloc(ab.n, c, ab.h, ab.w, ab.dtype, g.device)
        T.fuse_elem_bwd(ab, bb, gb, ga, gbb, mode, False)
        return ga.to_nchw(c), gbb.to_nchw(c), None


class _AttnFusionFn(torch.autograd.Function):
    """attention_fusion('sa'|'ca'|'sca') with spatial 'l1' / channel 'avg' pooling on the HIP kernels."""

    @staticmethod
    def forward(ctx, a, b, mode):
        dtype = E.compute_dtype()
        ab, bb = BT.from_nchw(a.detach(), dtype), BT.from_nchw(b.detach(), dtype)
        c = a.shape[1]
        ob = BT.alloc(ab.n, c, ab.h, ab.w, dtype, a.device)
        ws = T.attn_workspace(ab.n, c, a.device)
        T.attn_fwd(ab, bb, ob, mode, ws)
        ctx.saved = (ab, bb, mode, c, ws)
        return ob.to_nchw(c)

    @staticmethod
    def backward(ctx, g):
        ab, bb, mode, c, ws = ctx.saved
        gb = BT.from_nchw(g.contiguous(), ab.dtype)
        ga = BT.alloc(ab.n, c, ab.h, ab.w, ab.dtype, g.device)
        gbb = BT.alloc(ab.n, c, ab.h, ab.w, ab.dtype, g.device)
        T.attn_bwd(ab, bb, gb, ga, gbb, mode, False, ws)
        return ga.to_nchw(c), gbb.to_nchw(c), None


class _NonlocalSpatialFn(torch.autograd.Function):
    """spatial_pooling(x, 'nl') on csrc/nonlocal.hip: the energy is recomputed tile by tile in both directions; saved for backward are
    x, y, the softmax row sums l [B, H*W] and the 16-word scalar block (global min / max of the energy and where they sit)."""

    @staticmethod
    def forward(ctx, x):
        x = x.detach().contiguous()
        y, l, scal = T.nonlocal_spatial_fwd(x)
        ctx.save_for_backward(x, y, l, scal)
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, l, scal = ctx.saved_tensors
        return T.nonlocal_spatial_bwd(x, y, l, scal, g.contiguous())


class _NonlocalChannelFn(torch.autograd.Function):
    """channel_pooling(x, 'nl') on csrc/nonlocal_channel.hip; saved for backward are x, the energy and the attention matrix [B, C, C] and
    the 16-word scalar block (global min / max of the energy and where they sit)."""

    @staticmethod
    def forward(ctx, x):
        x = x.detach().contiguous()
        y, e, attn, scal = T.nonlocal_channel_fwd(x)
        ctx.save_for_backward(x, e, attn, scal)
        return y

    @staticmethod
    def backward(ctx, g):
        x, e, attn, scal = ctx.saved_tensors
        return T.nonlocal_channel_bwd(x, e, attn, scal, g.contiguous())


class _FusionJoinFn(torch.autograd.Function):
    """attention_fusion's join of the two features with their pooled maps (s1, s2 spatial, c1, c2 channel; the pair a mode does not use is
    None): one launch per direction, nothing saved but the operands, which the 'nl' functions keep anyway."""

    @staticmethod
    def forward(ctx, t1, t2, s1, s2, c1, c2, mode):
        ops = tuple(t.detach().contiguous() if t is not None else None for t in (t1, t2, s1, s2, c1, c2))
        ctx.save_for_backward(*(t for t in ops if t is not None))
        ctx.have = tuple(t is not None for t in ops)
        ctx.mode = mode
        return T.fuse_join_fwd(*ops, mode)

    @staticmethod
    def backward(ctx, g):
        it = iter(ctx.saved_tensors)
        ops = tuple(next(it) if h else None for h in ctx.have)
        return (*T.fuse_join_bwd(*ops, g.contiguous(), ctx.mode), None)


class _AttnFuseFn(torch.autograd.Function):
    """attention_fusion on csrc/attn_fuse.hip (codes: T.JOIN_MODES, T.AF_SPATIAL, T.AF_CHANNEL); saved for backward are the operands and the
    pools of the mode: s1, s2 [B, H*W], c1, c2 [B, C] and, for channel 'max', the positions of the maxima."""

    @staticmethod
    def forward(ctx, t1, t2, mode, spatial_mode, channel_mode):
        t1, t2 = t1.detach().contiguous(), t2.detach().contiguous()
        out, pools = T.attn_fuse_fwd(t1, t2, mode, spatial_mode, channel_mode)
        ctx.save_for_backward(t1, t2, *(t for t in pools if t is not None))
        ctx.have = tuple(t is not None for t in pools)
        ctx.codes = (mode, spatial_mode, channel_mode)
        return out

    @staticmethod
    def backward(ctx, g):
        t1, t2, *rest = ctx.saved_tensors
        it = iter(rest)
        pools = tuple(next(it) if h else None for h in ctx.have)
        return (*T.attn_fuse_bwd(t1, t2, pools, g.contiguous(), *ctx.codes), None, None, None)


def _nonlocal_impl():
    """$MMIF_NONLOCAL = hip (default) | torch: the streaming kernels, or the tensor-level composition everywhere (cross-check)"""
    v = os.environ.get("MMIF_NONLOCAL", "hip")
    if v not in ("hip", "torch"):
        raise ValueError(f"MMIF_NONLOCAL must be 'hip' or 'torch', got {v!r}")
    return v


_SPATIAL_NAMES = ('sum', 'mean', 'l1', 'l2', 'linf', 'nl')
_CHANNEL_NAMES = ('avg', 'max', 'nuclear', 'nl')


def _attn_fuse_impl():
    """$MMIF_ATTN_FUSE = hip (default) | torch: the fused kernels of csrc/attn_fuse.hip, or the tensor-level composition everywhere (cross-check)"""
    v = os.environ.get("MMIF_ATTN_FUSE", "hip")
    if v not in ("hip", "torch"):
        raise ValueError(f"MMIF_ATTN_FUSE must be 'hip' or 'torch', got {v!r}")
    return v


def _attn_fuse(tensor1, tensor2, mode, spatial_code, channel_code):
    """the fused route if it applies, else None"""
    if spatial_code is None or channel_code is None or _attn_fuse_impl() != 'hip' or not T.attn_fuse_supported(tensor1, tensor2):
        return None
    return _AttnFuseFn.apply(tensor1, tensor2, T.JOIN_MODES[mode], spatial_code, channel_code)


def element_fusion(tensor1, tensor2, mode='sum'):
    if mode not in _ELEM_MODES:
        raise ValueError("only supported ['sum', 'mean', 'max'] mode")
    if tensor1.is_cuda and tensor1.dim() == 4 and tensor1.shape == tensor2.shape:
        return _ElemFusionFn.apply(tensor1, tensor2, _ELEM_MODES[mode])
    T.require_device(tensor1, "element_fusion input")
    raise ValueError("element_fusion expects two [B,C,H,W] tensors of equal shape")


def weighted_fusion(tensor1, tensor2, w1, w2):
    w = w1 / (w1 + w2).clamp_(min=eps)
    return w * tensor1 + (1.0 - w) * tensor2


def concat_fusion(tensors, dim=1):
    return torch.cat(tensors, dim)


def _nonlocal(t, spatial):
    """Res2Fusion's non-local attention maps (reference core/fusion.py:96-113 spatial, :137-150 channel): softmax over a min-max
    normalised energy, applied to the features, plus the identity.  Tensor-level composition (two batched matmuls), used only where the
    kernels do not apply (CPU, C > 256; spatial: H or W < 8; channel: B * C < 2) or under $MMIF_NONLOCAL=torch."""
    b, c, h, w = t.shape
    flat = t.reshape(b, c, -1)
    if spatial:   # queries: every pixel; keys / values: the 8x8 average-pooled map
        pooled = torch.nn.functional.avg_pool2d(t, 8, 8).reshape(b, c, -1)
        q, k, v = flat.permute(0, 2, 1), pooled, pooled.permute(0, 2, 1)
    else:         # channel x channel
        q, k, v = flat, flat.permute(0, 2, 1), flat
    energy = q @ k
    lo, hi = torch.min(energy), torch.max(energy)
    attn = torch.softmax((energy - lo) / (hi - lo), dim=-1) @ v
    return (attn.permute(0, 2, 1) if spatial else attn).reshape(b, c, h, w) + t


def spatial_pooling(tensor, mode='l1'):
    if mode == 'sum':
        return tensor.sum(dim=1, keepdim=True)
    if mode == 'mean':
        return tensor.mean(dim=1, keepdim=True)
    if mode == 'l1':
        return tensor.norm(p=1, dim=1, keepdim=True)
    if mode == 'l2':
        return tensor.norm(p=2, dim=1, keepdim=True)
    if mode == 'linf':
        return tensor.max(dim=1, keepdim=True)[0]
    if mode == 'nl':
        if _nonlocal_impl() == 'hip' and T.nonlocal_spatial_supported(tensor):
            return _NonlocalSpatialFn.apply(tensor)
        return _nonlocal(tensor, spatial=True)
    raise ValueError("only supported ['sum', 'mean', 'l1', 'l2', 'linf', 'nl'] mode")


def channel_pooling(tensor, mode='avg'):
    if mode == 'avg':
        return tensor.mean(dim=(2, 3), keepdim=True)
    if mode == 'max':
        return tensor.amax(dim=(2, 3), keepdim=True)
    if mode == 'nl':
        if _nonlocal_impl() == 'hip' and T.nonlocal_channel_supported(tensor):
            return _NonlocalChannelFn.apply(tensor)
        return _nonlocal(tensor, spatial=False)
    if mode == 'nuclear':
        from ._stock import nuclear_pooling
        return nuclear_pooling(tensor)
    raise ValueError("only supported ['avg', 'max', 'nuclear', 'nl'] mode")


def spatial_fusion(tensor1, tensor2, mode='l1', softmax=True):
    if not softmax:
        fused = _attn_fuse(tensor1, tensor2, 'sa', T.AF_SPATIAL.get(mode), 0)
        if fused is not None:
            return fused
    s1, s2 = spatial_pooling(tensor1, mode), spatial_pooling(tensor2, mode)
    if softmax:
        s1, s2 = torch.exp(s1), torch.exp(s2)
    return weighted_fusion(tensor1, tensor2, s1, s2)


def channel_fusion(tensor1, tensor2, mode='avg', softmax=True):
    if not softmax:
        fused = _attn_fuse(tensor1, tensor2, 'ca', 0, T.AF_CHANNEL.get(mode))
        if fused is not None:
            return fused
    c1, c2 = channel_pooling(tensor1, mode), channel_pooling(tensor2, mode)
    if softmax:
        c1, c2 = torch.exp(c1), torch.exp(c2)
    return weighted_fusion(tensor1, tensor2, c1, c2)


def attention_fusion(tensor1, tensor2, mode='sca', spatial_mode='l1', channel_mode='avg'):
    if mode not in ('sa', 'ca', 'sca', 'wavg'):
        raise ValueError("only supported ['sa', 'ca', 'sca', 'wavg'] mode")
    if (tensor1.is_cuda and mode in T.ATTN_MODES and spatial_mode == 'l1' and channel_mode == 'avg' and tensor1.dim() == 4
            and tensor1.shape == tensor2.shape):
        return _AttnFusionFn.apply(tensor1, tensor2, T.ATTN_MODES[mode])
    if (spatial_mode == 'nl' and channel_mode == 'nl' and _nonlocal_impl() == 'hip' and tensor1.is_cuda and tensor2.is_cuda
            and tensor1.dtype == tensor2.dtype == torch.float32 and tensor1.dim() == 4 and tensor1.shape == tensor2.shape):
        s1 = s2 = c1 = c2 = None
        if mode != 'ca':
            s1, s2 = spatial_pooling(tensor1, 'nl'), spatial_pooling(tensor2, 'nl')
        if mode != 'sa':
            c1, c2 = channel_pooling(tensor1, 'nl'), channel_pooling(tensor2, 'nl')
        return _FusionJoinFn.apply(tensor1, tensor2, s1, s2, c1, c2, T.JOIN_MODES[mode])
    # a pooling the mode does not use only has to be a valid name (the composition below would evaluate it and throw the result away)
    sp_code = T.AF_SPATIAL.get(spatial_mode) if mode != 'ca' else (0 if spatial_mode in _SPATIAL_NAMES else None)
    ch_code = T.AF_CHANNEL.get(channel_mode) if mode != 'sa' else (0 if channel_mode in _CHANNEL_NAMES else None)
    fused = _attn_fuse(tensor1, tensor2, mode, sp_code, ch_code)
    if fused is not None:
        return fused
    f_spatial = spatial_fusion(tensor1, tensor2, spatial_mode, softmax=False)
    f_channel = channel_fusion(tensor1, tensor2, channel_mode, softmax=False)
    if mode == 'sa':
        return f_spatial
    if mode == 'ca':
        return f_channel
    if mode == 'sca':
        return (f_spatial + f_channel) / 2.0
    return weighted_fusion(f_spatial, f_channel, f_spatial, f_channel)


def softmax_l1_fusion(tensor1, tensor2):
    """SEDRFuse's strategy (reference core/model.py:271-281): per-pixel weights from the channel-softmax-weighted L1 activity
    sum_c softmax_c(|x|) |x| of each source -- spatial_fusion with the kernels' internal pooling code 5"""
    fused = _attn_fuse(tensor1, tensor2, 'sa', T.AF_SPATIAL_SOFTMAX_L1, 0)
    if fused is not None:
        return fused
    a1, a2 = torch.abs(tensor1), torch.abs(tensor2)
    s1 = spatial_pooling(torch.softmax(a1, dim=1) * a1, mode='sum')
    s2 = spatial_pooling(torch.softmax(a2, dim=1) * a2, mode='sum')
    return weighted_fusion(tensor1, tensor2, s1, s2)
