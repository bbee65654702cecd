"""Times value + gradient of SSIMLoss(mode, use_padding=True) in its four modes on the reflect-padded kernels of csrc/loss_modes.hip
(mmif_ssim_loss_pad: the statistics pass with reflected reads, the gradient pass with the border taps folded) against the composition
that ran the same option before these kernels existed -- core/_stock.py: F.pad plus five conv2d per pair per window, and autograd's graph
of per-pixel tensors for the backward -- in the same process, alternating the two, at the train batch 32 x 256^2 and at the full frame
1 x 1024 x 1224.

Device events around windows of back-to-back calls (the window length is calibrated to about 0.1 s), every shape and path warmed up
first; the figure is the median of REPEATS windows, with min and max.  Beside the times: the peak device memory each path allocates on
top of the three images (torch.cuda.max_memory_allocated around one call).

    python tools/bench_ssim_pad.py [--out profiles/ssim_pad_bench.txt] [--repeats 5] [--no-full-frame]
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

from core import _stock  # noqa: E402
from core.loss import SSIMLoss  # noqa: E402

SHAPES = ((32, 256, 256), (1, 1024, 1224))
MODES = ('ssim', 'w-ssim', 'ms-ssim', 'msw-ssim')
WINDOW_MS = 100.0
WEIGHT = 0.7


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def calibrate(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = max(window(fn, 3), 1e-3)
    return int(min(max(WINDOW_MS / ms, 3), 5000))


class Stage:
    """operands of one shape and mode; `new` is the module on the padded kernels, `old` the stock composition it replaces"""

    def __init__(self, mode, n, h, w):
        self.mode = mode
        self.a, self.b = torch.rand(n, 1, h, w, device="cuda"), torch.rand(n, 1, h, w, device="cuda")
        self.f = (0.5 * (self.a + self.b) + 0.1 * torch.rand(n, 1, h, w, device="cuda")).requires_grad_(True)
        self.loss = SSIMLoss(mode, use_padding=True, weight=WEIGHT)

    def _step(self, fn):
        self.f.grad = None
        loss = fn()
        loss.backward()
        return loss.detach(), self.f.grad

    def new(self):
        return self._step(lambda: self.loss(self.a, self.b, self.f))

    def old(self):
        return self._step(lambda: _stock.ssim_loss(self.mode, self.a, self.b, self.f, 1.0, True, WEIGHT))

    def peak_extra_mib(self, fn):
        fn()
        self.f.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def agree(st):
    """the two paths compute the same thing (fp32 rounding apart) on the operands that are timed"""
    (l1, g1), (l0, g0) = st.new(), st.old()
    g1, g0 = g1.clone(), g0.clone()
    dv, dg = abs(l1.item() - l0.item()), float((g1 - g0).abs().max() / g0.abs().max())
    assert dv < 1e-4 and dg < 1e-3, (st.mode, dv, dg)
    return dv, dg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_pad_bench.txt"))
    ap.add_argument("--no-full-frame", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ssim_pad needs a GPU"
    torch.manual_seed(1)
    lines = [f"# tools/bench_ssim_pad.py: {torch.cuda.get_device_name(0)}; value + gradient of SSIMLoss(mode, use_padding=True), ms per call, "
             f"median [min, max] of {args.repeats} windows of ~{WINDOW_MS:.0f} ms",
             "# 'new' = mmif_ssim_loss_pad; 'old' = core/_stock.py (F.pad + conv2d + autograd); MiB = peak device memory on top of the images",
             f"{'n x h x w':>16} {'mode':>9} {'new ms':>26} {'old ms':>29} {'old / new':>9} {'new MiB':>8} {'old MiB':>9} {'grad rel diff':>13}"]
    for n, h, w in SHAPES:
        if args.no_full_frame and h > 256:
            continue
        for mode in MODES:
            st = Stage(mode, n, h, w)
            _, dg = agree(st)
            paths = {"new": st.new, "old": st.old}
            mem = {k: st.peak_extra_mib(fn) for k, fn in paths.items()}
            iters = {k: calibrate(fn) for k, fn in paths.items()}
            times = {k: [] for k in paths}
            for _ in range(args.repeats):          # alternate the paths window by window
                for k, fn in paths.items():
                    times[k].append(window(fn, iters[k]))
            med = {k: statistics.median(v) for k, v in times.items()}
            fmt = lambda k: f"{med[k]:.4f} [{min(times[k]):.4f}, {max(times[k]):.4f}]"
            lines.append(f"{f'{n} x {h} x {w}':>16} {mode:>9} {fmt('new'):>26} {fmt('old'):>29} {med['old'] / med['new']:9.2f} {mem['new']:8.1f} "
                         f"{mem['old']:9.1f} {dg:13.1e}")
            print(json.dumps(dict(shape=[n, h, w], mode=mode, new_ms=med["new"], old_ms=med["old"], speedup=med["old"] / med["new"],
                                  new_mib=mem["new"], old_mib=mem["old"], iters=iters)), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:            # rewritten row by row: a run that is cut short leaves what it measured
                f.write("\n".join(lines) + "\n")
            del st
            torch.cuda.empty_cache()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
