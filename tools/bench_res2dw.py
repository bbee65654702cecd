"""Times the three passes of csrc/res2dw.hip (forward, input gradient, weight gradient of Res2ConvBlock's hierarchical depth-wise chain, one
launch per direction) at Res2Fusion's two blocks with --batch 2 -- 2 x (4 * 16) x 256^2 and 2 x (8 * 48) x 256^2 -- and the forward at the
full frame 1 x (8 * 48) x 1024 x 1224, against the composition that ran the same stage before these kernels existed, in the same process,
alternating the two:

    forward   Res2ConvBlock._mix_layers itself: chunk, a copy per group, a layout-converting add per group from the third on, one mmif_dwconv_fwd
              per group, the concatenation
    dgrad     what its backward runs for the input: a copy of each gy chunk, the add of the next group's dx, one mmif_dwconv_dgrad per group, the
              concatenation
    wgrad     what its backward runs for the weights: one mmif_dwconv_wgrad per group on the operands the forward saved (not timed: forming them)

Device events around windows of back-to-back calls (the window length is calibrated to about 0.1 s), every shape and path warmed up first; the
figure is the median of REPEATS windows, with min and max.  Beside each time of the new launches: the fraction of the byte floor -- 8 B per
element forward and dgrad (one tensor read, one written), 20 B for wgrad -- at the 6.3 TB/s that a plain copy reaches on this chip.

    python tools/bench_res2dw.py [--out profiles/res2dw_bench.txt] [--repeats 5] [--no-full-frame]
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

import core.block as B  # noqa: E402
from mmif import tensor as T  # noqa: E402

# (n, c, nseg, h, w, passes)
SHAPES = ((2, 16, 4, 256, 256, ("fwd", "dgrad", "wgrad")), (2, 48, 8, 256, 256, ("fwd", "dgrad", "wgrad")), (1, 48, 8, 1024, 1224, ("fwd", )))
BYTES = dict(fwd=8, dgrad=8, wgrad=20)
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
    ms = max(window(fn, 5), 1e-3)
    return int(min(max(WINDOW_MS / ms, 3), 5000))


class Stage:
    """operands of one shape; `new_*` are the one-launch calls, `old_*` the composition they replace"""

    def __init__(self, n, c, nseg, h, w, backward):
        self.c, self.nseg = c, nseg
        self.blk = B.Res2ConvBlock(c, c, scale=nseg).cuda()
        self.convs = [d.layers[0] for d in self.blk.dwconvs]
        with torch.no_grad():
            for m in self.convs:
                m.weight.copy_(torch.randn_like(m.weight) / (2 * m.kernel_size[0]))
        self.ws = [m.weight.detach() for m in self.convs]
        self.wp = torch.cat([w_.reshape(-1) for w_ in self.ws])
        self.x = torch.randn(n, nseg * c, h, w, device="cuda")
        self.elements = self.x.numel()
        if backward:
            self.gy = torch.randn_like(self.x)
            self.y = T.res2dw_fwd(self.x, self.wp, None, nseg, True)
            self.dx = T.res2dw_dgrad(self.gy, self.wp, nseg, True)
            # the operands the per-layer path saves in its forward / forms in its backward
            xs, ys = torch.chunk(self.x, nseg, dim=1), torch.chunk(self.y, nseg, dim=1)
            gs, ds = torch.chunk(self.gy, nseg, dim=1), torch.chunk(self.dx, nseg, dim=1)
            self.ins = [(xs[i] + ys[i - 1]) if i >= 2 else xs[i].contiguous() for i in range(nseg)]
            self.Gs = [(gs[i] + ds[i + 1]) if 1 <= i <= nseg - 2 else gs[i].contiguous() for i in range(nseg)]

    def new_fwd(self):
        return T.res2dw_fwd(self.x, self.wp, None, self.nseg, True)

    def new_dgrad(self):
        return T.res2dw_dgrad(self.gy, self.wp, self.nseg, True)

    def new_wgrad(self):
        return T.res2dw_wgrad(self.x, self.y, self.gy, self.dx, self.nseg, True, False)[0]

    def old_fwd(self):
        with torch.no_grad():
            return self.blk._mix_layers(self.x)

    def old_dgrad(self):
        outs, nxt = [None] * self.nseg, None
        for i in range(self.nseg - 1, -1, -1):
            G = torch.chunk(self.gy, self.nseg, dim=1)[i].contiguous()
            if 1 <= i <= self.nseg - 2:
                G = G + nxt
            nxt = outs[i] = T.dwconv_dgrad(G, self.ws[i], i > 0)
        return torch.cat(outs, dim=1)

    def old_wgrad(self):
        return torch.cat([T.dwconv_wgrad(self.ins[i], self.Gs[i], 3 if i else 1, i > 0, False)[0].reshape(-1) for i in range(self.nseg)])


def agree(st, passes):
    """the two paths compute the same thing (fp32 rounding apart) on the operands that are timed"""
    out = {}
    for name in passes:
        a, b = getattr(st, "new_" + name)(), getattr(st, "old_" + name)()
        out[name] = float((a - b).abs().max() / b.abs().max())
        assert out[name] < 1e-4, (name, out[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "res2dw_bench.txt"))
    ap.add_argument("--no-full-frame", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_res2dw needs a GPU"
    torch.manual_seed(1)
    lines = [f"# tools/bench_res2dw.py: {torch.cuda.get_device_name(0)}; ms per call, median [min, max] of {args.repeats} windows of ~{WINDOW_MS:.0f} ms",
             "# floor = 8 B per element (fwd, dgrad) / 20 B (wgrad) at 6.3 TB/s; 'of floor' = floor / time of the one-launch kernel; "
             "'old' = Res2ConvBlock._mix_layers (chunk copies + adds + mmif_dwconv_* per group + cat)",
             f"{'n x (nseg c) x h x w':>26} {'pass':>6} {'new ms':>24} {'floor ms':>9} {'of floor':>9} {'old ms':>27} {'old / new':>9} {'max rel diff':>12}"]
    for n, c, nseg, h, w, passes in SHAPES:
        if args.no_full_frame and h > 256:
            continue
        st = Stage(n, c, nseg, h, w, "wgrad" in passes)
        diff = agree(st, passes)
        for name in passes:
            floor_ms = st.elements * BYTES[name] / (COPY_TBPS * 1e12) * 1e3
            paths = {"new": getattr(st, "new_" + name), "old": getattr(st, "old_" + name)}
            iters = {k: calibrate(fn) for k, fn in paths.items()}
            times = {k: [] for k in paths}
            for _ in range(args.repeats):          # alternate the paths window by window
                for k, fn in paths.items():
                    times[k].append(window(fn, iters[k]))
            med = {k: statistics.median(v) for k, v in times.items()}
            fmt = lambda k: f"{med[k]:.4f} [{min(times[k]):.4f}, {max(times[k]):.4f}]"
            lines.append(f"{f'{n} x ({nseg} {c}) x {h} x {w}':>26} {name:>6} {fmt('new'):>24} {floor_ms:9.4f} {floor_ms / med['new']:9.2f} {fmt('old'):>27} "
                         f"{med['old'] / med['new']:9.2f} {diff[name]:12.1e}")
            print(json.dumps(dict(shape=[n, nseg, c, h, w], op=name, new_ms=med["new"], old_ms=med["old"], floor_ms=floor_ms,
                                  of_floor=floor_ms / med["new"], iters=iters)), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:            # rewritten shape by shape: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del st
        torch.cuda.empty_cache()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
