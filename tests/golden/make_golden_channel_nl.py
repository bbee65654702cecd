"""Golden F26: the reference's channel_pooling(x, 'nl') (core/fusion.py:137-150) and attention_fusion(a, b, mode, 'nl', 'nl') (:42-59) evaluated in
float64 -- outputs and the autograd gradients of sum(y * upstream) -- on the tables of tests/channel_nl_cases.py (inputs rebuilt by the tests
from seeds: the fixture holds results only).  Needs a checkout of the reference, named by $MMIF_REFERENCE; never imported by a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_channel_nl.py   ->   tests/golden/f26_channel_nl.npz

Keys: '<case>|y', '<case>|dx' (flat, at channel_nl_cases.sample_index(size)), '<case>|lo', '<case>|hi' (0-dim: the global energy extrema);
'fusion_<mode>|out', '|d1', '|d2' for the four modes at channel_nl_cases.FUSION_SHAPE.
The generator asserts the extremum gaps of the model-level cases, ignoring each element's transpose twin: torch splits the gradient across tied
extrema (immaterial between twins, because E and its gradient path are symmetric), and other ties are left out of the table on purpose.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import channel_nl_cases as CC  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")


def load_ref():
    assert os.path.isfile(os.path.join(REF, "core", "fusion.py")), "set MMIF_REFERENCE to a checkout of the reference"
    spec = importlib.util.spec_from_file_location("ref_fusion", os.path.join(REF, "core", "fusion.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def gaps(x):
    """(lo, hi, gap_lo, gap_hi) of the reference's own energy, the runner-up taken without the extremum's transpose twin"""
    b, c = x.shape[:2]
    flat = x.reshape(b, c, -1)
    e = (flat @ flat.permute(0, 2, 1)).detach().numpy()
    out = []
    for sign in (1.0, -1.0):
        v = (sign * e).reshape(-1).copy()
        k0 = int(np.argmin(v))
        bb, i, j = np.unravel_index(k0, e.shape)
        first = v[k0]
        v[k0] = np.inf
        v[np.ravel_multi_index((bb, j, i), e.shape)] = np.inf
        out.append((sign * first, v.min() - first))
    (lo, glo), (hi, ghi) = out
    return lo, hi, glo / (hi - lo), ghi / (hi - lo)


def main():
    R = load_ref()
    torch.set_num_threads(8)
    out = {}
    for name in CC.CASES:
        x = torch.from_numpy(CC.inputs(name).astype(np.float64)).requires_grad_(True)
        g = torch.from_numpy(CC.upstream(name).astype(np.float64))
        y = R.channel_pooling(x, 'nl')
        (y * g).sum().backward()
        lo, hi, glo, ghi = gaps(x)
        assert hi - lo > 1e-3 * abs(hi), (name, lo, hi)
        assert glo >= CC.MIN_GAP and ghi >= CC.MIN_GAP, (name, "tied extremum", glo, ghi)
        yv, dx = y.detach().numpy().reshape(-1), x.grad.numpy().reshape(-1)
        assert np.isfinite(yv).all() and np.isfinite(dx).all() and np.abs(yv).max() > 0 and np.abs(dx).max() > 0, name
        idx = CC.sample_index(yv.size)
        out[f"{name}|y"], out[f"{name}|dx"] = yv[idx].astype(np.float64), dx[idx].astype(np.float64)
        out[f"{name}|lo"], out[f"{name}|hi"] = np.float64(lo), np.float64(hi)
        print(name, tuple(x.shape), "lo", lo, "hi", hi, "gaps", glo, ghi, "stored", idx.size, "of", yv.size)
    t1, t2, g = CC.fusion_inputs()
    for mode in CC.FUSION_MODES:
        a = torch.from_numpy(t1.astype(np.float64)).requires_grad_(True)
        b = torch.from_numpy(t2.astype(np.float64)).requires_grad_(True)
        o = R.attention_fusion(a, b, mode, 'nl', 'nl')
        (o * torch.from_numpy(g.astype(np.float64))).sum().backward()
        idx = CC.sample_index(t1.size)
        for key, v in (("out", o.detach()), ("d1", a.grad), ("d2", b.grad)):
            v = v.numpy().reshape(-1)
            assert np.isfinite(v).all() and np.abs(v).max() > 0, (mode, key)
            out[f"fusion_{mode}|{key}"] = v[idx].astype(np.float64)
        print("fusion", mode, tuple(t1.shape), "stored", idx.size, "of", t1.size)
    np.savez_compressed(CC.F26, **out)
    print("wrote", CC.F26, os.path.getsize(CC.F26), "bytes")


if __name__ == "__main__":
    main()
