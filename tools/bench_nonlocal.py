"""Times spatial_pooling(x, 'nl') -- forward, and forward + backward -- with device events at the training shapes (1 x and 2 x 112 x 256
x 256) under both $MMIF_NONLOCAL settings, alternating them, and the 1224 x 1024 inference frame under 'hip' only (the composition's
energy tensor would be 98 GB there).  Prints one JSON line per measurement: median and min / max of REPEATS windows of ITERS calls.
--op channel times channel_pooling(x, 'nl') and --op fusion the whole layer attention_fusion(a, b, 'sca', 'nl', 'nl') the same way (the
frame under both settings there: the channel energy is [B, C, C]; the fusion layer's frame under 'hip' only, because of its spatial maps).

    python tools/bench_nonlocal.py [--op spatial|channel|fusion] [--frame 0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi-modal-image-fusion_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from core.fusion import attention_fusion, channel_pooling, spatial_pooling  # noqa: E402


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=1, help="0: skip the 1224 x 1024 inference frame")
    ap.add_argument("--op", choices=("spatial", "channel", "fusion"), default="spatial")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nonlocal needs a GPU"
    gen = torch.Generator(device="cpu").manual_seed(1)
    jobs = [((b, 112, 256, 256), impls, True) for b, impls in ((1, ("hip", "torch")), (2, ("hip", "torch")))]
    if args.frame:
        jobs.append(((1, 112, 1024, 1224), ("hip", "torch") if args.op == "channel" else ("hip",), False))
    if args.op == "spatial":
        op = lambda t, u: spatial_pooling(t, 'nl')
    elif args.op == "channel":
        op = lambda t, u: channel_pooling(t, 'nl')
    else:
        op = lambda t, u: attention_fusion(t, u, 'sca', 'nl', 'nl')
    for shape, impls, train in jobs:
        x = (torch.rand(shape, generator=gen) ** 2).cuda()
        g = torch.randn(shape, generator=gen).cuda()
        x2 = (torch.rand(shape, generator=gen) ** 2).cuda() if args.op == "fusion" else None

        def fwd():
            with torch.no_grad():
                op(x, x2)

        def fwdbwd():
            xr = x.detach().requires_grad_(True)
            op(xr, x2.detach().requires_grad_(True) if x2 is not None else None).backward(g)

        iters = args.iters if train else 2
        times = {}
        for what, fn in (("fwd", fwd),) + ((("fwd+bwd", fwdbwd),) if train else ()):
            for impl in impls:                     # warm-up of every (shape, path)
                os.environ["MMIF_NONLOCAL"] = impl
                window(fn, 2)
            for _ in range(args.repeats):          # alternate the paths inside every repeat
                for impl in impls:
                    os.environ["MMIF_NONLOCAL"] = impl
                    times.setdefault((what, impl), []).append(window(fn, iters))
        n, m, c = shape[2] * shape[3], (shape[2] // 8) * (shape[3] // 8), shape[1]
        for (what, impl), ts in times.items():
            med = statistics.median(ts)
            flop = shape[0] * 2.0 * n * m * c * (3 if what == "fwd" else 3 + 7)   # hip path: min/max + energy + apply; bwd: 3 + 4 products
            if args.op == "channel":
                flop = shape[0] * 2.0 * n * c * c * (2 if what == "fwd" else 2 + 3)   # energy + apply; bwd: dA + two products in the apply pass
            elif args.op == "fusion":
                flop = 0.0                                                           # two spatial + two channel maps + the join: no single figure
            print(json.dumps({"op": args.op, "shape": list(shape), "what": what, "impl": impl, "ms_median": round(med, 4), "ms_min": round(min(ts), 4),
                              "ms_max": round(max(ts), 4), "hip_path_tflops": round(flop / med / 1e9, 1) if impl == "hip" and flop else None}), flush=True)
        del x, g, x2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
