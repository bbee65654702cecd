"""Times the three launches of csrc/mixdw.hip (forward, input gradient, weight gradient; k = 1, 3, 5, 7 in one launch each) at the depth-wise
stage of MixConvBlock on MyFusion's four levels -- batch 8, 256 x 256 input: 64 channels at 256^2, 128 at 128^2, 256 at 64^2, 512 at 32^2 --
against the composition that ran the same stage before these kernels existed, in the same process, alternating the two:

    forward   4 chunk copies, mmif_dwconv_fwd for k = 1, 3, stock torch (reflection pad + grouped conv2d) for k = 5, 7, the concatenation
    dgrad     4 chunk copies of gy, mmif_dwconv_dgrad for k = 1, 3, stock torch's conv input gradient + pad backward for k = 5, 7, the concatenation
    wgrad     mmif_dwconv_wgrad (k = 1, 3) / stock torch's conv weight gradient (k = 5, 7) on the chunk copies of x and gy

Device events around windows of back-to-back calls (the window length is calibrated to about 0.1 s), every shape and path warmed up first; the
figure is the median of REPEATS windows, with min and max.  Beside each time of the new launches: the fraction of the byte floor, 8 B per
element (forward: x read, y written; dgrad: gy read, dx written; wgrad: x and gy read) at the 6.3 TB/s that a plain copy reaches on this chip.

    python tools/bench_mixdw.py [--out profiles/mixdw_bench.txt] [--batch 8] [--no-baseline]
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
import torch.nn.functional as F  # noqa: E402

from mmif import tensor as T  # noqa: E402

LEVELS = ((64, 256), (128, 128), (256, 64), (512, 32))
KS = (1, 3, 5, 7)
COPY_TBPS = 6.3
WINDOW_MS = 100.0


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
    ms = max(window(fn, 10), 1e-3)
    return int(min(max(WINDOW_MS / ms, 10), 5000))


class Stage:
    """operands of one level; `new_*` are the one-launch calls, `old_*` the composition they replace"""

    def __init__(self, batch, ch, size):
        self.c = ch // 4
        self.x = torch.randn(batch, ch, size, size, device="cuda")
        self.gy = torch.randn(batch, ch, size, size, device="cuda")
        self.ws = [torch.randn(self.c, 1, k, k, device="cuda") / k for k in KS]
        self.wp = torch.cat([w.reshape(-1) for w in self.ws])
        self.elements = self.x.numel()

    def new_fwd(self):
        return T.mixdw_fwd(self.x, self.wp, None, 4, 1, True)

    def new_dgrad(self):
        return T.mixdw_dgrad(self.gy, self.wp, 4, 1, True)

    def new_wgrad(self):
        return T.mixdw_wgrad(self.x, self.gy, 4, 1, True, False)[0]

    def old_fwd(self):
        outs = []
        for xs, w, k in zip(torch.chunk(self.x, 4, dim=1), self.ws, KS):
            xs = xs.contiguous()
            outs.append(T.dwconv_fwd(xs, w, None, k > 1) if k <= 3 else F.conv2d(F.pad(xs, (k // 2, ) * 4, mode="reflect"), w, groups=self.c))
        return torch.cat(outs, dim=1)

    def old_dgrad(self):
        outs = []
        for gs, w, k in zip(torch.chunk(self.gy, 4, dim=1), self.ws, KS):
            gs = gs.contiguous()
            if k <= 3:
                outs.append(T.dwconv_dgrad(gs, w, k > 1))
            else:
                p, (n, c, h, wd) = k // 2, gs.shape
                gp = torch.ops.aten.convolution_backward(gs, self._padded(k), w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], c, [True, False, False])[0]
                outs.append(torch.ops.aten.reflection_pad2d_backward(gp, gs, [p, p, p, p]))
        return torch.cat(outs, dim=1)

    def _padded(self, k):
        if not hasattr(self, "_pad"):
            self._pad = {kk: F.pad(xs.contiguous(), (kk // 2, ) * 4, mode="reflect") for xs, kk in zip(torch.chunk(self.x, 4, dim=1), KS) if kk > 3}
        return self._pad[k]

    def old_wgrad(self):
        outs = []
        for xs, gs, w, k in zip(torch.chunk(self.x, 4, dim=1), torch.chunk(self.gy, 4, dim=1), self.ws, KS):
            gs = gs.contiguous()
            if k <= 3:
                outs.append(T.dwconv_wgrad(xs.contiguous(), gs, k, k > 1, False)[0])
            else:
                outs.append(torch.ops.aten.convolution_backward(gs, self._padded(k), w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], self.c,
                                                                [False, True, False])[1])
        return outs


def agree(st):
    """the two paths compute the same thing (fp32 rounding apart) on the operands that are timed"""
    pairs = (("fwd", st.new_fwd(), st.old_fwd()), ("dgrad", st.new_dgrad(), st.old_dgrad()),
             ("wgrad", st.new_wgrad(), torch.cat([w.reshape(-1) for w in st.old_wgrad()])))
    out = {}
    for name, a, b in pairs:
        out[name] = float((a - b).abs().max() / b.abs().max())
        assert out[name] < 1e-4, (name, out[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixdw_bench.txt"))
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixdw needs a GPU"
    torch.manual_seed(1)
    lines = [f"# tools/bench_mixdw.py --batch {args.batch}: {torch.cuda.get_device_name(0)}; ms per call, median [min, max] of {args.repeats} windows of ~{WINDOW_MS:.0f} ms",
             "# floor = 8 B per element at 6.3 TB/s; 'of floor' = floor / time of the one-launch kernel; 'old' = chunk copies + mmif_dwconv_* (k = 1, 3) + stock torch (k = 5, 7) + cat",
             f"{'level':>14} {'pass':>6} {'new ms':>24} {'floor ms':>9} {'of floor':>9} {'old ms':>24} {'old / new':>9} {'max rel diff':>12}"]
    for ch, size in LEVELS:
        st = Stage(args.batch, ch, size)
        floor_ms = st.elements * 8 / (COPY_TBPS * 1e12) * 1e3
        diff = agree(st) if not args.no_baseline else {}
        for name in ("fwd", "dgrad", "wgrad"):
            paths = {"new": getattr(st, "new_" + name)}
            if not args.no_baseline:
                paths["old"] = getattr(st, "old_" + name)
            iters = {k: calibrate(fn) for k, fn in paths.items()}
            times = {k: [] for k in paths}
            for _ in range(args.repeats):          # alternate the paths window by window
                for k, fn in paths.items():
                    times[k].append(window(fn, iters[k]))
            med = {k: statistics.median(v) for k, v in times.items()}
            fmt = lambda k: f"{med[k]:.4f} [{min(times[k]):.4f}, {max(times[k]):.4f}]"
            old = fmt("old") if "old" in med else "not measured"
            ratio = f"{med['old'] / med['new']:.2f}" if "old" in med else "-"
            lines.append(f"{f'{ch} x {size}^2':>14} {name:>6} {fmt('new'):>24} {floor_ms:9.4f} {floor_ms / med['new']:9.2f} {old:>24} {ratio:>9} "
                         f"{diff.get(name, float('nan')):12.1e}")
            print(json.dumps(dict(level=[ch, size], batch=args.batch, op=name, new_ms=med["new"], old_ms=med.get("old"), floor_ms=floor_ms,
                                  of_floor=floor_ms / med["new"], iters=iters)), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:            # rewritten level by level: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
