"""Golden F21: the reference's spatial_pooling(x, 'nl') (core/fusion.py:96-113) evaluated in float64 -- output and the autograd gradient
of sum(y * upstream) w.r.t. x -- on the case table of tests/nonlocal_cases.py (inputs rebuilt by the tests from seeds: the fixture holds
results only).  Needs a checkout of the reference, named by $MMIF_REFERENCE; never imported by a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_nonlocal.py   ->   tests/golden/f21_nonlocal.npz

Keys: '<case>|y', '<case>|dx' (flat, at nonlocal_cases.sample_index(size)), '<case>|lo', '<case>|hi' (0-dim: the global energy extrema).
The generator asserts the tie guard: torch splits the gradient across tied extrema, and such inputs are left out of the table on purpose.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nonlocal_cases as NC  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")


def load_ref():
    assert os.path.isfile(os.path.join(REF, "core", "fusion.py")), "set MMIF_REFERENCE to a checkout of the reference"
    spec = importlib.util.spec_from_file_location("ref_fusion", os.path.join(REF, "core", "fusion.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    R = load_ref()
    torch.set_num_threads(8)
    out = {}
    for name in NC.CASES:
        x = torch.from_numpy(NC.inputs(name).astype(np.float64)).requires_grad_(True)
        g = torch.from_numpy(NC.upstream(name).astype(np.float64))
        y = R.spatial_pooling(x, 'nl')
        (y * g).sum().backward()
        with torch.no_grad():   # the tie guard, on the reference's own energy
            b, c, h, w = x.shape
            e = (x.reshape(b, c, -1).permute(0, 2, 1) @ torch.nn.functional.avg_pool2d(x, 8, 8).reshape(b, c, -1)).reshape(-1).sort()[0]
        lo, hi = e[0].item(), e[-1].item()
        assert hi - lo > 1e-3 * abs(hi), (name, lo, hi)
        assert (e[1] - e[0]).item() > NC.TIE_GAP * (hi - lo) and (e[-1] - e[-2]).item() > NC.TIE_GAP * (hi - lo), (name, "tied extremum")
        yv, dx = y.detach().numpy().reshape(-1), x.grad.numpy().reshape(-1)
        assert np.isfinite(yv).all() and np.isfinite(dx).all() and np.abs(yv).max() > 0 and np.abs(dx).max() > 0, name
        idx = NC.sample_index(yv.size)
        out[f"{name}|y"], out[f"{name}|dx"] = yv[idx].astype(np.float64), dx[idx].astype(np.float64)
        out[f"{name}|lo"], out[f"{name}|hi"] = np.float64(lo), np.float64(hi)
        print(name, tuple(x.shape), "lo", lo, "hi", hi, "stored", idx.size, "of", yv.size)
    np.savez_compressed(NC.F21, **out)
    print("wrote", NC.F21, os.path.getsize(NC.F21), "bytes")


if __name__ == "__main__":
    main()
