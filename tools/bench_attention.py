"""Times forward + backward of Attention (core/block.py) at the four level shapes of a 256 x 256 input -- 16 x 256^2, 32 x 128^2,
64 x 64^2, 128 x 32^2 at batch 8 -- under both $MMIF_SRA settings, alternating them; the attention core alone (sra_core on pre-computed
q, k, v) the same way; and the pooling conv alone, ConvLayer's HIP route against the stock modules it holds.  Device events after a
warm-up of every (shape, path); prints one JSON line per measurement: median and min / max of REPEATS windows of ITERS calls.  The core's
FLOP count is that of the products the kernels issue on valid data: 2 N M d per head for each of the 2 forward and 7 backward products
(score and dP twice, dq, dk, dv).

    python tools/bench_attention.py [--batch 8]
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

from core import block as B  # noqa: E402

LEVELS = ((16, 256), (32, 128), (64, 64), (128, 32))
FP32_MATRIX_TFLOPS = 157.3


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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attention needs a GPU"
    torch.manual_seed(1)
    for ch, size in LEVELS:
        mod = B.Attention(ch, ch).cuda()
        x = torch.randn(args.batch, ch, size, size, device="cuda")
        g = torch.randn(args.batch, ch, size, size, device="cuda")
        n, m = size * size, (size // mod.sr_ratio) ** 2
        with torch.no_grad():
            q = torch.randn(args.batch, ch, n, device="cuda")
            k, v = torch.randn(args.batch, ch, m, device="cuda"), torch.randn(args.batch, ch, m, device="cuda")
        go = g.reshape(args.batch, ch, n)

        def module():
            xr = x.detach().requires_grad_(True)
            mod(xr).backward(g)

        def core():
            qr, kr, vr = (t.detach().requires_grad_(True) for t in (q, k, v))
            B.sra_core(qr, kr, vr, mod.num_heads, mod.scale).backward(go)

        def core_fwd():
            with torch.no_grad():
                B.sra_core(q, k, v, mod.num_heads, mod.scale)

        def pool():
            xr = x.detach().requires_grad_(True)
            mod.pool(xr).backward(gp)

        def pool_stock():
            xr = x.detach().requires_grad_(True)
            mod.pool.layers(xr).backward(gp)

        with torch.no_grad():
            gp = torch.randn_like(mod.pool(x))
        times = {}
        for _ in range(2):                                 # the pooling conv: the HIP route of ConvLayer against the stock modules it holds
            window(pool, 2), window(pool_stock, 2)
        for _ in range(args.repeats):
            times.setdefault(("pool fwd+bwd", "hip"), []).append(window(pool, args.iters))
            times.setdefault(("pool fwd+bwd", "torch"), []).append(window(pool_stock, args.iters))
        for what, fn in (("Attention fwd+bwd", module), ("core fwd+bwd", core), ("core fwd", core_fwd)):
            for impl in ("hip", "torch"):              # warm-up of every (shape, path)
                os.environ["MMIF_SRA"] = impl
                window(fn, 2)
            for _ in range(args.repeats):              # alternate the paths inside every repeat
                for impl in ("hip", "torch"):
                    os.environ["MMIF_SRA"] = impl
                    times.setdefault((what, impl), []).append(window(fn, args.iters))
        for (what, impl), ts in times.items():
            med = statistics.median(ts)
            rec = {"shape": [args.batch, ch, size, size], "heads": mod.num_heads, "N": n, "M": m, "what": what, "impl": impl, "ms_median": round(med, 4),
                   "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}
            if impl == "hip" and what.startswith("core"):
                flop = args.batch * 2.0 * n * m * ch * (2 if what == "core fwd" else 9)
                rec["core_tflops"] = round(flop / med / 1e9, 2)
                rec["share_of_fp32_matrix_peak"] = round(flop / med / 1e9 / FP32_MATRIX_TFLOPS, 4)
            print(json.dumps(rec), flush=True)
        del mod, x, g, q, k, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
