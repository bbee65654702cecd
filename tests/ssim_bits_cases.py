"""Golden F24: the BITS of the SSIM family -- every workspace query and every output of the loss-side and metric-side SSIM / MS-SSIM entry
points of csrc/loss.hip, csrc/loss_modes.hip and csrc/metric_ssim.hip.

The oracle tests and the GPU sweeps hold these kernels to fp64 definitions within tolerances; that catches a wrong formula, not a changed
summation order or a differently contracted FMA.  The calls below are run once on a reference build (tests/golden/make_golden_ssim_bits.py
-> tests/golden/f24_ssim_bits.json: a byte count per workspace query, a SHA-256 per output) and again by tests/test_ssim_bits_cpu.py (the
queries: host functions, no GPU) and tests/test_gpu_ssim_bits.py (the outputs).  None of these kernels sizes its grid by the compute-unit
count, so the bits hold on every gfx950 device.

Inputs come from the existing builders (loss_cases.triple, ssim_pad_cases.build, ssim_metric_cases.build); the shapes are the smallest at
which each kernel can still go wrong:
    mmif_ssim_loss, mmif_fusion_loss    11 x 11 (a one-pixel map), 43 x 54 (a 33 x 44 map: ragged second 32-tile on both axes)
    mmif_ssim_loss_mode 1, 3            27 x 38 (two ragged 16-tiles per axis);  mode 2: 161 x 176, its smallest legal size
    mmif_ssim_loss_pad 0, 1, 3          11 x 12 (every row and column folds), 27 x 38 (left and right folds in different tiles);  mode 2: 81 x 83
    mmif_ssim_terms(_pad)               every window 3, 5, 7, 9, 11 at 27 x 38 (the 3-tap window carries the one-ulp normaliser)
    mmif_metric_msssim                  161 x 176, with b and with b == NULL
    mmif_metric_ssim_maps               k = 1, 4, 11 padded and not at 17 x 18 (4 padded: an (h + 1) x (w + 1) map), win_size 11 at 7 x 9 (the
                                        window shrinks to 7); maps and sums
    mmif_metric_msssim_any              9 x 9 and 40 x 37, padded and not, with and without b
"""
import ctypes as C
import hashlib

import numpy as np

import loss_cases as LC
import ssim_metric_cases as SMC
import ssim_pad_cases as SPC

DEV = "cuda:0"

# ------------------------------------------------------------------------------------------------------------------------------
# the workspace queries (host functions)
# ------------------------------------------------------------------------------------------------------------------------------
WS_SHAPES = [(1, 11, 11), (2, 27, 38), (3, 81, 83), (2, 161, 176)]


def workspace_queries(lib):
    """id -> bytes of every *_workspace query of the family at WS_SHAPES"""
    out = {}
    for s in WS_SHAPES:
        tag = "%dx%dx%d" % s
        out[f"mmif_loss_workspace-{tag}"] = lib.mmif_loss_workspace(*s)
        out[f"mmif_fusion_loss_workspace-{tag}"] = lib.mmif_fusion_loss_workspace(*s)
        for mode in (1, 2, 3):
            out[f"mmif_ssim_loss_mode_workspace-{tag}-mode{mode}"] = lib.mmif_ssim_loss_mode_workspace(*s, mode)
        for mode in (0, 1, 2, 3):
            out[f"mmif_ssim_loss_pad_workspace-{tag}-mode{mode}"] = lib.mmif_ssim_loss_pad_workspace(*s, mode)
        out[f"mmif_metric_msssim_workspace-{tag}"] = lib.mmif_metric_msssim_workspace(*s)
        for win in (1, 4, 11):
            for pad in (0, 1):
                out[f"mmif_metric_ssim_maps_workspace-{tag}-k{win}-{'pad' if pad else 'valid'}"] = lib.mmif_metric_ssim_maps_workspace(*s, win, pad)
        out[f"mmif_metric_msssim_any_workspace-{tag}"] = lib.mmif_metric_msssim_any_workspace(*s)
    return {k: int(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# the calls (GPU): id -> (entry, n, h, w, settings)
# ------------------------------------------------------------------------------------------------------------------------------
def _cases():
    cs = {}

    def add(entry, n, h, w, **kw):
        tag = "".join(f"-{k}{v}" for k, v in kw.items())
        cs[f"{entry}-{n}x{h}x{w}{tag}"] = (entry, n, h, w, kw)
    for h, w in ((11, 11), (43, 54)):
        add("ssim_loss", 2, h, w)
        add("fusion_loss", 2, h, w)
    for mode in (1, 3):
        add("ssim_loss_mode", 2, 27, 38, mode=mode)
    add("ssim_loss_mode", 1, 161, 176, mode=2)
    for mode in (0, 1, 3):
        for h, w in ((11, 12), (27, 38)):
            add("ssim_loss_pad", 2, h, w, mode=mode)
    add("ssim_loss_pad", 1, 81, 83, mode=2)
    for entry in ("ssim_terms", "ssim_terms_pad"):
        for win in (3, 5, 7, 9, 11):
            add(entry, 2, 27, 38, win=win)
    for b in (1, 0):
        add("metric_msssim", 2, 161, 176, b=b)
    for win in (1, 4, 11):
        for pad in (0, 1):
            add("metric_ssim_maps", 2, 17, 18, win=win, pad=pad)
    for pad in (0, 1):
        add("metric_ssim_maps", 2, 7, 9, win=11, pad=pad)
    for h, w in ((9, 9), (40, 37)):
        for pad in (0, 1):
            for b in (1, 0):
                add("metric_msssim_any", 2, h, w, pad=pad, b=b)
    return cs


CASES = _cases()


def inputs(name):
    """the float32 images of a case, [n,1,h,w] each, in call order"""
    entry, n, h, w, kw = CASES[name]
    if entry in ("ssim_loss", "fusion_loss", "ssim_loss_mode"):
        return LC.triple('rand', h, w, n)
    if entry in ("ssim_loss_pad", "ssim_terms", "ssim_terms_pad"):
        trip = SPC.build(('rand', h, w, n, 0))
        return trip if entry == "ssim_loss_pad" else trip[:2]
    if entry == "metric_msssim":
        a, f = SMC.build("ms-161x176-b2-k11-valid-blend")           # a fused image against one of its sources, 0..255
        b = SMC.build("ms-161x176-b2-k11-pad-rand255")[1]
        return a, b, f
    trip = LC.triple('r255', h, w, n)
    return trip[:2] if entry == "metric_ssim_maps" else trip


def sha_inputs(arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return m.hexdigest()


def run(name):
    """run the case on the current device; returns (outputs {name: tensor}, SHA-256 of the input images)"""
    import torch
    from mmif import tensor as T
    from mmif._lib import check, lib
    entry, n, h, w, kw = CASES[name]
    arrs = inputs(name)
    x = [torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV) for a in arrs]       # (a copy: the shared builders hand out read-only arrays)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    zeros = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    ws_of = lambda nbytes: torch.zeros(int(nbytes) // 4 + 64, dtype=torch.float32, device=DEV)
    st = T.stream_ptr()
    if entry == "ssim_loss":
        loss, grad, ws = zeros(1), zeros(n, 1, h, w), ws_of(lib.mmif_loss_workspace(n, h, w))
        check(lib.mmif_ssim_loss(p(x[0]), p(x[1]), p(x[2]), n, h, w, 0.7, 1.0, p(loss), p(grad), p(ws), ws.numel() * 4, st), name)
        out = {"loss": loss, "grad": grad}
    elif entry == "fusion_loss":
        vals, grad, ws = zeros(5), zeros(n, 1, h, w), ws_of(lib.mmif_fusion_loss_workspace(n, h, w))
        check(lib.mmif_fusion_loss(p(x[0]), p(x[1]), p(x[2]), n, h, w, 0.7, 1.0, 0.3, 1, 0, 0.5, 1, 0, p(vals), p(grad), p(ws), ws.numel() * 4, st), name)
        out = {"values": vals, "grad": grad}
    elif entry in ("ssim_loss_mode", "ssim_loss_pad"):
        query, fn = (lib.mmif_ssim_loss_mode_workspace, lib.mmif_ssim_loss_mode) if entry == "ssim_loss_mode" else \
            (lib.mmif_ssim_loss_pad_workspace, lib.mmif_ssim_loss_pad)
        loss, grad, ws = zeros(1), zeros(n, 1, h, w), ws_of(query(n, h, w, kw["mode"]))
        check(fn(p(x[0]), p(x[1]), p(x[2]), n, h, w, 0.7, 1.0, kw["mode"], p(loss), p(grad), p(ws), ws.numel() * 4, st), name)
        out = {"loss": loss, "grad": grad}
    elif entry in ("ssim_terms", "ssim_terms_pad"):
        terms, ws = zeros(3, n), ws_of(lib.mmif_ssim_loss_mode_workspace(n, h, w, 1))
        check(getattr(lib, "mmif_" + entry)(p(x[0]), p(x[1]), n, h, w, kw["win"], 1.0, p(terms), p(ws), ws.numel() * 4, st), name)
        out = {"terms": terms}
    elif entry == "metric_msssim":
        rows, ws = zeros(2, 6, n), ws_of(lib.mmif_metric_msssim_workspace(n, h, w))
        check(lib.mmif_metric_msssim(p(x[0]), p(x[1]) if kw["b"] else None, p(x[2]), n, h, w, 255.0, p(rows), p(ws), ws.numel() * 4, st), name)
        out = {"rows": rows}
    elif entry == "metric_ssim_maps":
        k = min(kw["win"], h, w)
        pd = k // 2 if kw["pad"] else 0
        hm, wm = h + 2 * pd - k + 1, w + 2 * pd - k + 1
        ssim, cs, sums = zeros(n, hm, wm), zeros(n, hm, wm), zeros(n, 2, dtype=torch.float64)
        ws = ws_of(lib.mmif_metric_ssim_maps_workspace(n, h, w, kw["win"], kw["pad"]))
        check(lib.mmif_metric_ssim_maps(p(x[0]), p(x[1]), n, h, w, kw["win"], kw["pad"], 255.0, p(ssim), p(cs), p(sums), p(ws), ws.numel() * 4, st), name)
        out = {"ssim_map": ssim, "cs_map": cs, "sums": sums}
    elif entry == "metric_msssim_any":
        rows, ws = zeros(2, 6, n, dtype=torch.float64), ws_of(lib.mmif_metric_msssim_any_workspace(n, h, w))
        check(lib.mmif_metric_msssim_any(p(x[0]), p(x[1]) if kw["b"] else None, p(x[2]), n, h, w, 11, kw["pad"], 255.0, p(rows), p(ws),
                                         ws.numel() * 4, st), name)
        out = {"rows": rows}
    else:
        raise ValueError(entry)
    torch.cuda.synchronize()
    return out, sha_inputs(arrs)


def digest(t):
    """(SHA-256 of the bytes of t + 0.0 in t's own dtype -- the sign of an exact zero is not part of the contract --, fp64 sum)"""
    a = np.ascontiguousarray((t.detach() + 0.0).cpu().numpy())
    return hashlib.sha256(a.tobytes()).hexdigest(), float(a.astype(np.float64).sum())
