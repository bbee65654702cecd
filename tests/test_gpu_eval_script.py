"""eval.py end to end on a tiny dataset made of golden F19's integer images (lossless PNG sources, BMP fused images), in the
'tno' layout (vis/ and ir/ at the dataset root) and the 'test/' layout -- as a subprocess, the way a user runs it."""
import csv
import math
import os
import shutil
import subprocess
import sys
import uuid

import numpy as np
import pytest
from PIL import Image

import metric_cases as MC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-modal-image-fusion_amd")
CASES = ["cf256_int", "nat256x320", "cf181x203_int"]
TOL = {'SSIM': 1e-4, 'MSSSIM': 1e-4, 'VIFF': 2e-4}
KEYS = dict(zip(['SD', 'AG', 'SF', 'MSE', 'PSNR', 'CC', 'SCD', 'EN', 'CE', 'MI', 'Qabf', 'Nabf', 'Labf', 'SSIM', 'MSSSIM', 'VIFF'],
                ['sd', 'ag', 'sf', 'mse', 'psnr', 'cc', 'scd', 'en', 'ce', 'mi', 'qabf', 'nabf', 'labf', 'ssim', 'msssim', 'viff']))


def _save(path, arr):
    Image.fromarray(arr[0, 0].astype(np.uint8)).save(path)


@pytest.mark.parametrize("data", ["tno", "roadscene"])
def test_eval_py_writes_the_metric_table(data):
    f19 = MC.load_f19()
    tag = "evaltest_" + uuid.uuid4().hex[:10]
    dset = os.path.join(ROOT, "datasets", tag)
    ckpt = os.path.join(ROOT, "checkpoints", tag)
    try:
        src = dset if data == "tno" else os.path.join(dset, "test")
        for d in ("vis", "ir"):
            os.makedirs(os.path.join(src, d))
        os.makedirs(os.path.join(ckpt, tag))
        names = [f"{i * 5 + 2}.png" for i in range(len(CASES))]   # 2, 7, 12: natural order differs from the lexical one
        for i, (case, name) in enumerate(zip(CASES, names)):
            a, b, f = MC.build(case, f19)
            _save(os.path.join(src, "vis", name), a)
            _save(os.path.join(src, "ir", name), b)
            _save(os.path.join(ckpt, tag, f"{i + 1:0>2}.bmp"), f)
        # the dataset folder name decides the layout in eval.py; link the unique name under the layout's name
        link = os.path.join(ROOT, "datasets", data)
        made_link = not os.path.exists(link)
        if made_link:
            os.symlink(dset, link)
        try:
            if not os.path.samefile(link, dset):
                pytest.skip(f"datasets/{data} exists already")
            env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            # the fused images live under <ckpt>/<data>/
            os.rename(os.path.join(ckpt, tag), os.path.join(ckpt, data))
            r = subprocess.run([sys.executable, "eval.py", "--data", data, "--ckpt", tag, "--model", "PFNetv1"], cwd=PKG, env=env,
                               capture_output=True, text=True, timeout=600)
        finally:
            if made_link:
                os.unlink(link)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "done, cost" in r.stdout
        rows = list(csv.reader(open(os.path.join(ckpt, f"metrics_{data}_PFNetv1.csv"))))
        assert rows[0] == [''] + list(KEYS)
        assert [r_[0] for r_ in rows[1:]] == ['mean', 'std'] + names
        per = np.array([[float(v) for v in r_[1:]] for r_ in rows[3:]])
        for i, case in enumerate(CASES):
            for j, k in enumerate(KEYS):
                ref = float(f19[f"{case}|eval_{KEYS[k]}|0|64"])
                assert abs(per[i, j] - ref) <= TOL.get(k, 1e-5) * max(abs(ref), 1e-3), (case, k, per[i, j], ref)
        mean = np.array([float(v) for v in rows[1][1:]])
        std = np.array([float(v) for v in rows[2][1:]])
        for j in range(len(KEYS)):
            col = list(per[:, j])
            col.insert(0, np.mean(col))
            assert math.isclose(mean[j], col[0], rel_tol=1e-12, abs_tol=1e-15)
            assert math.isclose(std[j], np.std(col), rel_tol=1e-9, abs_tol=1e-12)
    finally:
        shutil.rmtree(dset, ignore_errors=True)
        shutil.rmtree(ckpt, ignore_errors=True)
