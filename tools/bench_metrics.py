"""Milliseconds per triple of core.metric.fusion_metrics (the 16 metrics of eval.py) at B = 1 and B = 16 on 256x256 and 1024x1224
integer-valued random triples: HIP events around `iters` calls after warm-up; prints one JSON line.

    python tools/bench_metrics.py [--iters 20 --warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-modal-image-fusion_amd"))

import torch  # noqa: E402

from core.metric import fusion_metrics  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    res = {"metric": "fusion_metrics_ms_per_triple"}
    with torch.no_grad():
        for h, w in ((256, 256), (1024, 1224)):
            for b in (1, 16):
                a, c, f = (torch.randint(0, 256, (b, 1, h, w), generator=g).float().cuda() for _ in range(3))
                for _ in range(args.warmup):
                    fusion_metrics(a, c, f)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fusion_metrics(a, c, f)
                e1.record()
                torch.cuda.synchronize()
                res[f"{h}x{w}_b{b}"] = round(e0.elapsed_time(e1) / args.iters / b, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
