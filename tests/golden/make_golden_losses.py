"""Golden F20: the reference's loss modules (core/loss.py) evaluated in float64 -- value and autograd gradient w.r.t. the fused image --
for the modes goldens F2 / F9 do not hold: PixelLoss / GradLoss in {l1, l2} x {avg, max}, SSIMLoss 'ssim' / 'w-ssim' / 'msw-ssim' at
data_range = 255, 'ms-ssim' with an active 1e-7 clamp, TVLoss on a [2,3,h,w] input.  Inputs are the builders of tests/loss_cases.py
(rebuilt by the tests: the fixture holds results only).  Needs a checkout of the reference, named by $MMIF_REFERENCE; never imported by
a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_losses.py   ->   tests/golden/f20_loss_modes.npz, f20_manifest.json

Keys: '<entry>|<case>|loss' (0-dim) and '<entry>|<case>|grad', 'window|<k>' (the k x k window's float32
values); the manifest lists entries and cases (tests/loss_cases.f20_entries()).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loss_cases as LC  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")


def load_ref():
    assert os.path.isfile(os.path.join(REF, "core", "loss.py")), "set MMIF_REFERENCE to a checkout of the reference"
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(REF, "core", "loss.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def evaluate(R, entry, arrays):
    """(loss, d loss / d fused) of one F20 entry on float64 tensors"""
    kind, a = entry["kind"], entry["args"]
    ts = [torch.from_numpy(np.asarray(x, np.float64)) for x in arrays]
    f = ts[-1].requires_grad_(True)
    if kind == "pixel":
        loss = R.PixelLoss(a["norm"], weight=a["weight"])(ts[0], ts[1], f, mode=a["mode"])
    elif kind == "grad":
        loss = R.GradLoss(a["norm"], weight=a["weight"])(ts[0], ts[1], f, mode=a["mode"])
    elif kind == "ssim":
        loss = R.SSIMLoss(a["mode"], data_range=a["data_range"], weight=a["weight"])(ts[0], ts[1], f)
    elif kind == "tv":
        loss = R.TVLoss(a["norm"], weight=a["weight"])(f)
    else:
        raise KeyError(kind)
    loss.backward()
    return loss.detach().numpy(), f.grad.numpy()


def main():
    R = load_ref()
    torch.set_num_threads(8)
    out, manifest = {}, {}
    for k in LC.WIN_SIZES:      # the 2-D window of every size the kernels take: float32 values, stored as float64
        out[f"window|{k}"] = R.create_window(k).numpy()[0, 0].astype(np.float64)
    for name, entry in LC.f20_entries().items():
        manifest[name] = {"kind": entry["kind"], "args": entry["args"], "cases": list(entry["cases"])}
        for case in entry["cases"]:
            loss, grad = evaluate(R, entry, LC.f20_inputs(entry["kind"], case))
            assert np.isfinite(loss) and loss != 0.0 and np.isfinite(grad).all() and np.abs(grad).max() > 0.0, (name, case)
            out[f"{name}|{case}|loss"] = np.float64(loss)
            out[f"{name}|{case}|grad"] = grad.astype(np.float64)
            print(name, case, float(loss), float(np.abs(grad).max()))
    np.savez_compressed(LC.F20, **out)
    with open(LC.F20_MANIFEST, "w") as fh:
        json.dump(manifest, fh, indent=1)
    print("wrote", LC.F20, os.path.getsize(LC.F20), "bytes")


if __name__ == "__main__":
    main()
