"""Res2Fusion on the streaming non-local kernels: the full 1224 x 1024 frame under no_grad, and forward + backward captured into a
hipGraph after eager steps (the pattern of test_gpu_models.py's graph tests)."""
import pytest
import torch

from gpu_util import dtype_ctx

pytestmark = pytest.mark.gpu


def test_res2fusion_full_frame_inference(monkeypatch):
    """1 x 1 x 1024 x 1224 (BASELINE config 5): one energy tensor of the composition would be N * M * 4 = 98 GB per source"""
    import core.model as M
    monkeypatch.delenv("MMIF_NONLOCAL", raising=False)
    dev = torch.device("cuda", 0)
    h, w = 1024, 1224
    n, m = h * w, (h // 8) * (w // 8)
    with dtype_ctx("fp32"):
        torch.manual_seed(11)
        model = M.Res2Fusion().to(dev).eval()
        g = torch.Generator(device="cpu").manual_seed(12)
        a, b = torch.rand(1, 1, h, w, generator=g).to(dev), torch.rand(1, 1, h, w, generator=g).to(dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            y = model(a, b)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    print(f"Res2Fusion 1x1x{h}x{w}: peak extra memory {peak / 2**30:.2f} GiB (one energy tensor: {n * m * 4 / 2**30:.1f} GiB)")
    assert y.shape == (1, 1, h, w)
    assert torch.isfinite(y).all()
    assert float(y.max() - y.min()) > 0
    assert peak < n * m * 4


def test_res2fusion_graph_replay_equals_eager_gradients(monkeypatch):
    """Forward + losses + backward of Res2Fusion captured after two eager optimiser steps; a replay gives the eager step's gradients bit
    for bit.  Res2Fusion is a layer-wise model (core/block.py: its parameters are the autograd leaves), so the rule of mmif/graph.py
    holds: no autograd graph of an earlier DEFAULT-stream step may be alive at capture time (its AccumulateGrad nodes would pull the
    null stream into the capture).  The eager optimiser steps therefore run on a stream of their own, and nothing they return keeps a
    graph."""
    import gc

    import core.model as M
    from core.loss import FusionLoss, GradLoss, PixelLoss, SSIMLoss
    from mmif.graph import GraphedStep
    from mmif.optim import FusedClipAdam
    monkeypatch.delenv("MMIF_NONLOCAL", raising=False)
    dev = torch.device("cuda", 0)
    with dtype_ctx("fp32"):
        torch.manual_seed(4)
        model = M.Res2Fusion().to(dev)
        opt = FusedClipAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.999), max_norm=5.0)
        fl = FusionLoss(SSIMLoss('ssim', weight=1.0), PixelLoss('l1', weight=0.01), GradLoss('l1', weight=0.1).to(dev), 'max', 'max')

        def losses(a, b, f):
            tot = fl(a, b, f)
            return (tot,) + tuple(fl.values[1:4].unbind(0))

        def eager_step(a, b, step):
            opt.zero_grad(set_to_none=True)
            ls = losses(a, b, model(a, b))
            ls[0].backward()
            if step:
                opt.step(scalars=[v.detach() for v in ls])
            return [float(v.detach()) for v in ls]
        g = torch.Generator(device="cpu").manual_seed(6)
        a, b = torch.rand(2, 1, 64, 96, generator=g).to(dev), torch.rand(2, 1, 64, 96, generator=g).to(dev)
        pre = torch.cuda.Stream()
        pre.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(pre):
            for _ in range(2):
                eager_step(a, b, True)
        torch.cuda.current_stream().wait_stream(pre)
        fl.values = None            # the last eager graph hangs off the loss module's value vector
        opt.zero_grad(set_to_none=True)
        gc.collect()
        torch.cuda.synchronize()
        gs = GraphedStep(model, losses, opt, a, b)
        outs = gs(a, b, step_optimizer=False)
        torch.cuda.synchronize()
        got = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
        got_l = [float(o.detach()) for o in outs]
        want_l = eager_step(a, b, False)
        torch.cuda.synchronize()
        assert got_l == want_l
        nz = 0
        for p, q in zip(model.parameters(), got):
            assert (p.grad is None) == (q is None)
            if q is not None:
                assert torch.equal(p.grad, q)
                nz += int(q.abs().max() > 0)
        assert nz > 10
