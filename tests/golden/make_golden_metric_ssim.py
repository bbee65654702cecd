"""Golden F21 (metric SSIM): the reference's calc_ssim / calc_msssim / create_window (core/metric.py) on the cases of
tests/ssim_metric_cases.py, run on float64 tensors.  Needs a checkout of the reference, named by $MMIF_REFERENCE; never imported by a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_metric_ssim.py   ->   tests/golden/F21_metric_ssim.npz

Keys: 'taps|k', 'window|k' (k = 1..11, float32); per 'ssim' case '<case>|means' = (ssim, cs) of size_average=True, '<case>|shape' = the
map shape and, for maps of at most 1500 pixels, '<case>|ssim' / '<case>|cs' (size_average=False, full=True); per 'ms' case
'<case>|pooled' = calc_msssim of the batch and '<case>|value' = calc_msssim of every sample alone.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssim_metric_cases as SC  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")
OUT = os.path.join(HERE, "F21_metric_ssim.npz")
MAP_LIMIT = 1500


def load_ref():
    assert os.path.isfile(os.path.join(REF, "core", "metric.py")), "set MMIF_REFERENCE to a checkout of the reference"
    spec = importlib.util.spec_from_file_location("ref_metric", os.path.join(REF, "core", "metric.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    R = load_ref()
    out = {}
    for k in range(1, 12):
        out[f"taps|{k}"] = R._gaussian_kernel(k).numpy()
        out[f"window|{k}"] = R.create_window(k).numpy()[0, 0]
    with torch.no_grad():
        for name, (kind, h, w, n, win, pad, dist) in SC.CASES.items():
            a, b = (torch.from_numpy(np.array(x)).double() for x in SC.build(name))
            dr = SC.data_range(dist)
            if kind == 'ssim':
                s, c = R.calc_ssim(a, b, win, dr, bool(pad), size_average=False, full=True)
                ms, mc = R.calc_ssim(a, b, win, dr, bool(pad), size_average=True, full=True)
                out[f"{name}|means"] = np.array([float(ms), float(mc)])
                out[f"{name}|shape"] = np.array(s.shape, np.int64)
                if s.numel() <= MAP_LIMIT:
                    out[f"{name}|ssim"], out[f"{name}|cs"] = s.numpy(), c.numpy()
            else:
                out[f"{name}|pooled"] = np.array([float(R.calc_msssim(a, b, win, dr, bool(pad)))])
                out[f"{name}|value"] = np.array([float(R.calc_msssim(a[i:i + 1], b[i:i + 1], win, dr, bool(pad))) for i in range(n)])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
