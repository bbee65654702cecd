"""Golden F19: the reference's fusion-quality metrics (core/metric.py) on the cases of tests/metric_cases.py, each run in fp64
(what the tests compare against) and in fp32.  Needs a checkout of the reference, named by $MMIF_REFERENCE; never imported by a test.

    MMIF_REFERENCE=<reference checkout> python tests/golden/make_golden_metrics.py   ->   tests/golden/f19_metrics.npz

Keys: nat_vis / nat_ir (the uint8 crops); per case and precision (64 | 32) the vector '<case>|mirror|<bits>' of every mirror
function's value and the [B, 16] table '<case>|eval|<bits>' of eval.py's values per sample, names in f19_manifest.json.  NaN values
are stored as 0 with a '<key>|nan' mask next to them (no fixture array may be all-zero or NaN); tests/metric_cases.load_f19()
restores them.
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
sys.path.insert(0, os.path.join(ROOT, "multi-modal-image-fusion_amd"))
import metric_cases as MC  # noqa: E402
from data._io import imread_gray  # noqa: E402

REF = os.environ.get("MMIF_REFERENCE", "")


def load_ref():
    assert os.path.isfile(os.path.join(REF, "core", "metric.py")), "set MMIF_REFERENCE to a checkout of the reference"
    spec = importlib.util.spec_from_file_location("ref_metric", os.path.join(REF, "core", "metric.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def eval_table(R, a, b, f):
    """the 16 values eval.py reports for one triple, combined as its eval_metrics does"""
    mse = (R.calc_mse(a, f) + R.calc_mse(b, f)) * 0.5
    qabf, nabf, labf = R.calc_Qabf(a, b, f, L=1.5, full=True)
    return {
        'sd': R.calc_std(f), 'ag': R.calc_ag(f), 'sf': R.calc_sf(f), 'mse': mse, 'psnr': R.calc_psnr(mse),
        'cc': (R.calc_cc(a, f) + R.calc_cc(b, f)) * 0.5, 'scd': R.calc_scd(a, b, f), 'en': R.calc_entropy(f),
        'ce': R.calc_cross_ent(a, f) + R.calc_cross_ent(b, f),
        'mi': R.calc_mul_info(a, f, normalized=True) + R.calc_mul_info(b, f, normalized=True),
        'qabf': qabf, 'nabf': nabf, 'labf': labf, 'ssim': (R.calc_ssim(a, f) + R.calc_ssim(b, f)) * 0.5,
        'msssim': (R.calc_msssim(a, f) + R.calc_msssim(b, f)) * 0.5, 'viff': R.calc_viff(a, b, f, simple=False),
    }


def mirror_values(R, a, b, f):
    """every mirror function and option on one (possibly pooled) triple"""
    v = {
        'mean': R.calc_mean(f), 'std': R.calc_std(f), 'ag': R.calc_ag(f), 'sf': R.calc_sf(f), 'mse': R.calc_mse(a, f),
        'psnr': R.calc_psnr(R.calc_mse(a, f)), 'psnr_root': R.calc_psnr(R.calc_mse(a, f), L=1.0, root=True),
        'cc': R.calc_cc(a, f), 'scd': R.calc_scd(a, b, f), 'en': R.calc_entropy(f), 'en_a': R.calc_entropy(a),
        'ce': R.calc_cross_ent(a, f), 'mi': R.calc_mul_info(a, f), 'mi_norm': R.calc_mul_info(a, f, normalized=True),
        'qabf': R.calc_Qabf(a, b, f), 'qabf_L1': R.calc_Qabf(a, b, f, L=1.0),
        'nabf': R.calc_Nabf(a, b, f), 'nabf_orig': R.calc_Nabf(a, b, f, modified=False), 'labf': R.calc_Labf(a, b, f),
        'ssim': R.calc_ssim(a, f), 'msssim': R.calc_msssim(a, f), 'msssim_pad': R.calc_msssim(a, f, use_padding=True),
    }
    v['qabf_full_q'], v['qabf_full_n'], v['qabf_full_l'] = R.calc_Qabf(a, b, f, full=True)
    if min(a.shape[-2:]) >= 41:
        v['viff'] = R.calc_viff(a, b, f)
        v['viff_full'] = R.calc_viff(a, b, f, simple=False)
    return v


def store(out, key, arr):
    nan = np.isnan(arr)
    out[key] = np.where(nan, 0.0, arr)
    if nan.any():
        out[key + "|nan"] = nan.astype(np.uint8)


def main():
    R = load_ref()
    sample = os.path.join(REF, "data", "samples", "infrared", "test")
    vis = imread_gray(os.path.join(sample, "vis", "00633D.png"))
    ir = imread_gray(os.path.join(sample, "ir", "00633D.png"))
    y0, x0 = (vis.shape[0] - 256) // 2, (vis.shape[1] - 320) // 2
    out = {"nat_vis": np.ascontiguousarray(vis[y0:y0 + 256, x0:x0 + 320]), "nat_ir": np.ascontiguousarray(ir[y0:y0 + 256, x0:x0 + 320])}
    torch.set_num_threads(8)
    manifest = {}
    with torch.no_grad():
        for name in MC.CASES:
            a, b, f = MC.build(name, out)
            for bits, dt in (("64", torch.float64), ("32", torch.float32)):
                ta, tb, tf = (torch.from_numpy(x).to(dt) for x in (a, b, f))
                vals = {k: float(v) for k, v in mirror_values(R, ta, tb, tf).items()}
                manifest.setdefault(name, {})["mirror"] = list(vals)
                store(out, f"{name}|mirror|{bits}", np.array(list(vals.values())))
                if min(a.shape[-2:]) >= 41:
                    tab = [{k: float(v) for k, v in eval_table(R, ta[s:s + 1], tb[s:s + 1], tf[s:s + 1]).items()} for s in range(a.shape[0])]
                    manifest[name]["eval"] = list(tab[0])
                    store(out, f"{name}|eval|{bits}", np.array([list(t.values()) for t in tab]))
                if bits == "64":
                    print(name, {k: round(v, 5) for k, v in vals.items()})
    np.savez_compressed(MC.F19, **out)
    with open(MC.F19_MANIFEST, "w") as fh:
        json.dump(manifest, fh, indent=1)
    print("wrote", MC.F19, os.path.getsize(MC.F19), "bytes")


if __name__ == "__main__":
    main()
