"""Golden F27: the reference's attention_fusion(a, b, mode, spatial_mode, channel_mode) (core/fusion.py:42-126) for every tensor-level pooling
combination, and SEDRFuse.fusion (core/model.py:271-281), evaluated in float64 -- outputs and the autograd gradients of sum(out * upstream) -- on
the "gold" case of tests/attn_fuse_cases.py (planted: a tied 'linf' maximum, a plane maximum at three positions, all-zero pixel vectors, an
all-zero plane).  The inputs are rebuilt by the tests from seeds: the fixture holds results only.  Needs a checkout of the reference, named by
$MMIF_REFERENCE; never imported by a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_attn_fusion.py   ->   tests/golden/f27_attn_fusion.npz, f27_manifest.json

Keys: '<mode>|<spatial>|<channel>|out', '|d1', '|d2' (flat float64); SEDRFuse's strategy is 'sa|softmax_l1|avg'.  The manifest lists the keys with
their sizes and the case they were computed on.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attn_fuse_cases as AC  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")


def load_ref(name):
    path = os.path.join(REF, "core", name + ".py")
    assert os.path.isfile(path), "set MMIF_REFERENCE to a checkout of the reference"
    sys.path.insert(0, os.path.join(REF, "core"))      # (model.py falls back to plain `from fusion import *`)
    spec = importlib.util.spec_from_file_location("ref_" + name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    RF, RM = load_ref("fusion"), load_ref("model")
    t1, t2, g = AC.inputs("gold")
    out = {}
    for combo in AC.COMBOS:
        mode, sm, cm = combo
        a = torch.from_numpy(t1.astype(np.float64)).requires_grad_(True)
        b = torch.from_numpy(t2.astype(np.float64)).requires_grad_(True)
        o = RM.SEDRFuse.fusion(None, a, b) if sm == AC.SEDR else RF.attention_fusion(a, b, mode, sm, cm)
        (o * torch.from_numpy(g.astype(np.float64))).sum().backward()
        for key, v in (("out", o.detach()), ("d1", a.grad), ("d2", b.grad)):
            v = v.numpy().reshape(-1)
            assert np.isfinite(v).all() and np.abs(v).max() > 0, (combo, key)
            out["|".join(combo) + "|" + key] = v.astype(np.float64)
        print(combo, "out", float(np.abs(out["|".join(combo) + "|out"]).max()))
    np.savez_compressed(AC.F27, **out)
    manifest = {"fixture": os.path.basename(AC.F27), "case": "gold", "shape": list(AC.BY_NAME["gold"].shape),
                "sizes": {k: int(v.size) for k, v in sorted(out.items())}}
    with open(os.path.join(HERE, "f27_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", AC.F27, os.path.getsize(AC.F27), "bytes")
    assert os.path.getsize(AC.F27) < 100 * 1024


if __name__ == "__main__":
    main()
