"""The entry points end to end on the device, on a small image dataset written to disk: train.py (whole-image mode through
data/dataset.py, and patch mode through the on-device feed) and test.py (reference test.py:72-188: dataset -> checkpoint ->
per-image SSIM + NN.bmp outputs + result lines appended to the checkpoint's train.log)."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-modal-image-fusion_amd")
DATA = "_gputest_data"


def _img(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    return ((np.sin(y * 0.11 + seed) + np.cos(x * 0.07 + seed * 0.5)) * 60 + 128 + ((y * x + seed) % 17)).clip(0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def dataset():
    root = os.path.join(ROOT, "datasets", DATA)
    shutil.rmtree(root, ignore_errors=True)
    before = set(os.listdir(os.path.join(ROOT, "checkpoints"))) if os.path.isdir(os.path.join(ROOT, "checkpoints")) else set()
    for split, sizes in (("train", [(272, 300)] * 4 + [(200, 260)] + [(256, 256)] * 5), ("test", [(120, 136), (97, 131), (64, 64)])):
        for sub in ("vis", "ir"):
            os.makedirs(os.path.join(root, split, sub))
        for i, (h, w) in enumerate(sizes):
            Image.fromarray(_img(h, w, i)).save(os.path.join(root, split, "vis", f"{i + 1}.png"))
            Image.fromarray(_img(h, w, 50 + i)).save(os.path.join(root, split, "ir", f"{i + 1}.png"))
    yield root
    shutil.rmtree(root, ignore_errors=True)
    ck = os.path.join(ROOT, "checkpoints")
    if os.path.isdir(ck):
        for d in set(os.listdir(ck)) - before:
            shutil.rmtree(os.path.join(ck, d), ignore_errors=True)


def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"{script} {' '.join(args)} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout + r.stderr


def _newest_ckpt():
    dirs = sorted(glob.glob(os.path.join(ROOT, "checkpoints", "*")), key=os.path.getmtime)
    assert dirs, "train.py wrote no checkpoint folder"
    return dirs[-1]


def test_train_whole_images_then_test(dataset):
    out = _run("train.py", "--data", DATA, "--use_patches", "", "--bs", "2", "--epoch", "2", "--model", "PFNetv1", "--warmup", "1")
    assert "training done" in out and "train loss" in out
    ck = _newest_ckpt()
    for f in ("epoch_best.pth", "epoch_last.pth", "train.log", os.path.join("train", "01.png"), os.path.join("valid", "02.png")):
        assert os.path.isfile(os.path.join(ck, f)), f
    w, h = Image.open(os.path.join(ck, "train", "01.png")).size
    assert (w, h) == (3 * 256, 256)                       # img1 | img2 | fused side by side (common.save_result)
    out = _run("test.py", "--data", DATA, "--ckpt", os.path.basename(ck), "--model", "PFNetv1")
    assert out.count("iter: ") == 3 and "fps:" in out
    for i, (hh, ww) in enumerate([(120, 136), (97, 131), (64, 64)]):
        im = Image.open(os.path.join(ck, DATA, f"{i + 1:0>2}.bmp"))
        assert im.size == (ww, hh)
    log = open(os.path.join(ck, "train.log")).read()
    assert "iter: 03, ssim:" in log and "fps:" in log


def test_train_patches_on_device_feed(dataset):
    out = _run("train.py", "--data", DATA, "--bs", "8", "--epoch", "1", "--model", "DenseFuse", "--dtype", "bf16")
    assert "training done" in out


def test_bench_two_ranks_gloo_one_device():
    """bench.py's N > 1 plumbing end to end before the driver's first SCALE run does it: `--gpus 2` without a launcher environment starts
    a child torch.distributed.run (free rendezvous port), both ranks share cuda:0 over gloo (the only backend that allows it: RCCL wants
    one device per rank, and this box has one), parameters are broadcast, gradients all-reduced early + late, and rank 0's JSON line is
    the LAST thing on stdout (the other ranks' stdout goes to stderr)."""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--one-device", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-parity-path"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, f"bench.py --gpus 2 failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    out = json.loads(lines[-1])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 64 and out["config"]["parallelism"] == "dp2" and out["config"]["backend"] == "gloo"
    assert out["scaling"] == "weak" and out["steps"] == 3 and out["value"] > 0
    assert np.isfinite(out["final_loss"]) and 0.0 < out["final_loss"] < 10.0
    assert out["roofline"] is not None and set(out["roofline_kernels"]) == {"fwd", "dgrad", "wgrad"}
    assert out["parity_path"] is None and out["cpu_baseline"] is None       # N = 1 only


@pytest.mark.parametrize("model,batch,gpus,size", [("PFNetv1", 4, 8, 256), ("DenseFuse", 4, 8, 256), ("NestFuse", 1, 4, 64)])
def test_bench_eight_ranks_gloo_one_device_preflight(model, batch, gpus, size):
    """Pre-flight for the driver's first real `--gpus 8` run (round-4 verdict item 9, round-5 item 10; reference train.py:203-222, 285-297):
    N ranks through the self-launch, one rendezvous port, the stdout discipline (ONE JSON line, last), n_gpus = N, global_batch = N x
    per-rank batch, `dpN` -- configs 2 (PFNetv1) and 3 (DenseFuse, batch split over 8 ranks) on 8 ranks, config 4 (NestFuse) on its 4.
    One GPU here, so the ranks share cuda:0 over gloo; nothing is measured, everything must not break."""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--backend", "gloo", "--one-device", "--model", model, "--batch", str(batch),
                        "--size", str(size), "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-parity-path"], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, f"bench.py --gpus {gpus} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert sum(1 for l in lines if l.lstrip().startswith("{")) == 1, lines[-5:]      # exactly one JSON line on stdout
    out = json.loads(lines[-1])
    assert out["n_gpus"] == gpus and out["config"]["global_batch"] == gpus * batch and out["config"]["parallelism"] == f"dp{gpus}"
    assert out["config"]["backend"] == "gloo"
    assert out["scaling"] == "weak" and out["steps"] == 2 and out["value"] > 0 and model in out["config"]["workload"]
    assert np.isfinite(out["final_loss"]) and 0.0 < out["final_loss"] < 10.0
    assert out["parity_path"] is None and out["cpu_baseline"] is None and out["other_configs"] is None     # N = 1 only


def test_bench_other_configs_block_small_shapes(monkeypatch):
    """`other_configs` of bench.py's line (verdict r5 item 1d): the leg that times BASELINE configs 3, 4, 5 after the headline, run here on
    small stand-ins of the four configs (same models / modes / step function): every entry carries value, ms_per_step and -- where SURVEY
    8(d) has a row -- the fraction of ideal; losses finite; the compute dtype is restored."""
    import argparse
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from mmif import engine as E
    monkeypatch.setattr(bench, "OTHER_CONFIGS", (("DenseFuse_small", "DenseFuse", "train", 2, 64, 64, "t"), ("NestFuse_small", "NestFuse", "train", 1, 64, 64, "t"),
                                                 ("RFNNest_small", "RFNNest", "train", 1, 64, 64, "t"), ("infer_small", "PFNetv1", "infer", 1, 72, 104, "t")))
    prev = E.compute_dtype()
    res = bench.other_configs_leg(argparse.Namespace(other_steps=2, other_warmup=1), torch.device("cuda", 0))
    assert E.compute_dtype() == prev
    assert set(res) == {"DenseFuse_small", "NestFuse_small", "RFNNest_small", "infer_small"}
    for k, v in res.items():
        assert v["value"] > 0 and v["ms_per_step"] > 0 and 2 <= v["steps"] <= bench.OTHER_MAX_STEPS and v["warmup"] >= 1 and np.isfinite(v["final_value"]), (k, v)
        assert v["step_frac_of_ideal"] is not None and 0 < v["step_frac_of_ideal"] < 1, (k, v)
    assert [c[0] for c in bench.OTHER_CONFIGS] and {c[1] for c in bench.OTHER_CONFIGS} == {"DenseFuse", "NestFuse", "RFNNest", "PFNetv1"}


def test_bench_single_gpu_line_has_the_contract_fields():
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "2", "--batch", "4", "--size", "64", "--cpu-sample", "2",
                        "--parity-steps", "2"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, f"bench.py failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    out = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "step_frac_of_ideal"):
        assert k in out, k
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert rf["step_share"] == max(v["step_share"] for v in out["roofline_kernels"].values())
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["steps"] >= 3 and cb["cores"] <= 32 and cb["value"] >= cb["median_value"] > 0
    pp = out["parity_path"]
    assert pp["rel_err_vs_oracle"] < 1e-3 and pp["grad_rel_err_vs_oracle"] < 1e-3 and len(pp["oracle_samples"]) == 2
    assert pp["roofline"]["peak"] == 2500.0 and pp["roofline"]["products_per_tap"] == 3 and pp["roofline"]["frac"] < 1.0
    assert abs(pp["roofline"]["executed_mfma_tflops"] - 3 * pp["roofline"]["algorithmic_fp32_tflops"]) < 1e-6 * pp["roofline"]["executed_mfma_tflops"]


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """A plain `bench.py` run (no --full) times exactly --steps steps and measures nothing beyond the headline: no HIP events, no parity
    leg, no other configs, no CPU baseline.  --dump-outputs writes the last timed step's fused image, loss values, gradient norm and
    updated parameters as float32 .npy files; the dumped total loss is the line's final_loss."""
    import json
    out_dir = tmp_path / "outs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "2", "--size", "64",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, f"bench.py failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    out = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["full"] is False and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    for k in ("roofline", "roofline_kernels", "roofline_sampling", "roofline_hbm", "roofline_hbm_bwd", "parity_path", "other_configs", "cpu_baseline"):
        assert out[k] is None, k
    files = {p.name: np.load(p) for p in out_dir.iterdir()}
    assert files["fused_image.npy"].shape == (2, 1, 64, 64) and files["losses.npy"].shape == (4,) and files["grad_norm.npy"].shape == (1,)
    assert sum(1 for n in files if n.startswith("param.")) == 26
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert abs(float(files["losses.npy"][0]) - out["final_loss"]) <= 1e-6 * abs(out["final_loss"])
    assert sum(p.stat().st_size for p in out_dir.iterdir()) <= 64 * 10**6
