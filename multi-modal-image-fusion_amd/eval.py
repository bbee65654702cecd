# -*- coding: utf-8 -*-
"""Image evaluation -- entry point mirroring the reference's eval.py (eval_metrics :29-76, main :100-361): the 16 fusion-quality
metrics of every fused image against its two sources, on the HIP metric kernels (core/metric.py: fusion_metrics), one line per
image, the total time, and the table <checkpoint>/metrics_<data>_<model>.csv in the layout of the reference's 'method' sheet.

    python eval.py --data roadscene --ckpt 2023-02-26_23-15 [--model PFNetv1]
    python eval.py --synthetic 8          # 8 random integer-valued 1024x1224 triples, no dataset / checkpoint needed

Sources: <datasets>/<data>/[test/]vis and .../ir (.../po for 'polar'); fused images: <checkpoints>/<ckpt>/<data>/NN.bmp in natural
order of the source names, as test.py writes them.  Differences, deliberate: CSV instead of .xlsx, --model names the method
(the reference edits a list), images are read through data/_io.py (cv2 when present).
"""
import csv
import os
import sys
import time

BASE_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, BASE_DIR)

import numpy as np
import torch

from common import get_test_args
from core.metric import FUSION_METRICS, fusion_metrics
from data._io import IMG_EXT, imread_gray, natural_sorted

device = torch.device('cuda:0')
HEADER = ['SD', 'AG', 'SF', 'MSE', 'PSNR', 'CC', 'SCD', 'EN', 'CE', 'MI', 'Qabf', 'Nabf', 'Labf', 'SSIM', 'MSSSIM', 'VIFF']


def eval_metrics(img1, img2, imgf):
    """the 16 metrics of one [1,1,H,W] triple as Python floats (reference eval.py:29-76)"""
    with torch.no_grad():
        r = fusion_metrics(img1, img2, imgf)
    return {k: v.item() for k, v in r.items()}


def test_set_name(data):
    """reference eval.py:120-128: 'tno' keeps vis/ and ir/ at the dataset root, the others under test/ (as test.py)"""
    return None if data in ['tno'] else 'test'


def source_dirs(data):
    data_dir = os.path.join(BASE_DIR, '..', 'datasets', data)
    root = data_dir if test_set_name(data) is None else os.path.join(data_dir, 'test')
    return os.path.join(root, 'vis'), os.path.join(root, 'po' if data == 'polar' else 'ir')


def _load(path):
    return torch.from_numpy(imread_gray(path).astype(np.float32))[None, None].to(device, non_blocking=True)


def write_table(path, names, rows):
    """the reference's 'method' sheet as CSV: header, mean, std, one row per image"""
    cols = [[r[k] for r in rows] for k in FUSION_METRICS]
    for c in cols:
        c.insert(0, np.mean(c))
        # the reference's quirk, kept: its std is np.std (ddof 0) of the list AFTER the mean was inserted, i.e. over the
        # n per-image values plus their mean
        c.insert(1, np.std(c))
    labels = ['mean', 'std'] + list(names)
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow([''] + HEADER)
        for i, label in enumerate(labels):
            w.writerow([label] + [repr(float(c[i])) for c in cols])


if __name__ == '__main__':
    args = get_test_args()
    assert torch.cuda.is_available(), 'the HIP engine needs a GPU'
    torch.cuda.set_device(device)

    ckpt_dir = os.path.join(BASE_DIR, '..', 'checkpoints', args.ckpt)
    if args.synthetic > 0:
        g = torch.Generator().manual_seed(0)
        triples = [tuple(torch.randint(0, 256, (1, 1, 1024, 1224), generator=g).float() for _ in range(3)) for _ in range(args.synthetic)]
        names = [f'{i + 1:0>2}' for i in range(args.synthetic)]
        save_path = None
    else:
        img1_dir, img2_dir = source_dirs(args.data)
        assert os.path.isdir(img1_dir), f'{img1_dir} is not a dir (use --synthetic N)'
        imgf_dir = os.path.join(ckpt_dir, args.data)
        names = [n for n in natural_sorted(os.listdir(img1_dir)) if n.endswith(IMG_EXT)]
        triples = [(os.path.join(img1_dir, n), os.path.join(img2_dir, n), os.path.join(imgf_dir, f'{i + 1:0>2}.bmp')) for i, n in enumerate(names)]
        save_path = os.path.join(ckpt_dir, f'metrics_{args.data}_{args.model}.csv')

    print(f'evaluating {args.model} ...')
    start = time.time()
    rows = []
    for name, (p1, p2, pf) in zip(names, triples):
        if isinstance(p1, str):
            img1, img2, imgf = _load(p1), _load(p2), _load(pf)
            if imgf.shape != img1.shape or img2.shape != img1.shape:
                raise ValueError(f'{pf}: fused image {tuple(imgf.shape[-2:])} and sources {tuple(img1.shape[-2:])}, '
                                 f'{tuple(img2.shape[-2:])} differ in size')
        else:
            img1, img2, imgf = (t.to(device) for t in (p1, p2, pf))
        rows.append(eval_metrics(img1, img2, imgf))
        print(f'evaluating {name} ... ' + ', '.join(f'{k}: {rows[-1][k]:.4f}' for k in FUSION_METRICS))
    torch.cuda.synchronize(device)
    print(f'evaluating {args.model} done, cost {time.time() - start:.3f}s')
    if save_path is not None:
        write_table(save_path, names, rows)
        print(f'metrics written to {save_path}')
